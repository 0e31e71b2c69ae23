"""Case table of tests/test_l2_fast_install_gpu.py: rule sets and documents that drive the install path of the flat-tier rule
kernel (struspattern_amd/csrc/l2_fast_kernel.hip: installBatch and what it calls) through its forms and edges.  A case is
(rules, documents, compile, switches per instance, hand-overs expected per instance); a rule is (name, operator, range, terms)
as struspattern_amd.synth.apply_rules takes it.  Nothing here needs a GPU."""
import numpy as np

from struspattern_amd import synth

NOID = 99                     # a lexem id no rule mentions
K, K2, K3 = 20, 21, 22        # key terms: the first term of a sequence keys the program
INSTANCES = {"n": {}, "t": {"SPA_L2_FAST_SIZE": "t"}}


def doc(ids, pos=None):
    ids = np.asarray(ids, np.uint32)
    lex = np.zeros((len(ids), 4), np.uint32)
    lex[:, 0] = ids
    lex[:, 1] = np.arange(1, len(ids) + 1) if pos is None else pos
    lex[:, 2] = np.arange(len(ids)) * 3
    lex[:, 3] = 2
    return lex


def batch(docs):
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    return np.concatenate(docs), offs


def keyed(n, key=K, op="sequence", rg=8, name="k", ops=None):
    """n two-term programs keyed by `key`, in definition order; their second terms go round 1..6; ops: operator by index"""
    return [("%s%d_%d" % (name, key, i), (ops or {}).get(i, op), rg, [key, 1 + i % 6]) for i in range(n)]


def burst_docs(key=K, seed=0):
    """the key, then the six second terms and a delimiter in a changing order, three times; a few lexems no rule mentions"""
    rng = np.random.default_rng(seed)
    docs = []
    for d in range(3):
        ids = []
        for rep in range(3):
            tail = list(rng.permutation([1, 2, 3, 4, 5, 6])) + [NOID]
            if (d + rep) % 2:
                tail.insert(int(rng.integers(1, 6)), synth.DELIM)
            ids += [key] + tail + [NOID] * int(rng.integers(0, 3))
        docs.append(doc(ids))
    return docs


def _list_length(n):
    # key lists of 1, 63, 64 and 65 programs: one batch, a full batch, a second batch of one
    return keyed(n), burst_docs(seed=n), False, INSTANCES, {"n": 0, "t": 0}


def _second_trigger(which):
    # a *_struct program installs two triggers (its term and the delimiter), a plain sequence one
    ops = {"none": {}, "all": {i: "sequence_struct" for i in range(64)}, "first": {0: "sequence_struct"}, "last": {63: "sequence_struct"}}[which]
    return keyed(64, ops=ops), burst_docs(seed=70), False, INSTANCES, {"n": 0, "t": 0}


def _three_triggers():
    # one program of three terms in a key list of two-term programs: the batch leaves the compact form, the third slot is used
    rules = keyed(20) + [("three_w", "within", 6, [K, 2, 5]), ("three_s", "sequence", 6, [K, 3, 4])] + keyed(20, name="m")
    return rules, burst_docs(seed=71), False, INSTANCES, {"n": 0, "t": 0}


def _bucket_fill(n):
    # every key event adds n entries to the bucket of term 1 and the rules live 63 positions: the bucket's size passes through
    # every multiple of n -- with n = 1 through its LDS capacity exactly and through one more, whatever that capacity is
    rules = [("b%d" % i, "sequence", 63, [K, 1]) for i in range(n)]
    reps = 60 if n == 1 else 24
    docs = [doc([K] * reps + [1, NOID, K, 1]), doc([K] * (reps - 7) + [1, 1] + [K] * 5 + [1])]
    return rules, docs, False, INSTANCES, {"n": 0, "t": 0}


def _free_stack():
    # ten rules expire and leave ten free ids; then a key list of ten (exactly the stack) or of eleven (one id more than it holds)
    rules = keyed(10, rg=2) + keyed(10, key=K2, rg=4) + keyed(11, key=K3, rg=4)
    docs = []
    for second in (K2, K3):
        ids = [K, NOID, 1, 2, second, 1, 2, 3, 4, 5, 6, K, 3, second, 4, 5]
        pos = [1, 2, 3, 3, 9, 10, 10, 11, 11, 12, 12, 20, 21, 22, 23, 24]
        docs.append(doc(ids, pos))
    return rules, docs, False, INSTANCES, {"n": 0, "t": 0}


def _dynamic_after_static():
    # optimized rule set: programs keyed by an alternative key replay the logged original key event (dynamic form) while the
    # delimiter sits in the stop-word log; several lexems share a position, so batches of both forms run on the same position
    rules = synth.random_rules(300, 30, 225, "sequence_struct") + synth.random_rules(150, 30, 226, "within") + synth.random_rules(150, 30, 227, "sequence")
    lex, offs = synth.random_documents(4, 200, 30, 2225)
    docs = [lex[int(offs[d]):int(offs[d + 1])] for d in range(len(offs) - 1)]
    return rules, docs, True, INSTANCES, {"n": 0, "t": 0}


def _line_results():
    # `any` completes on its key event: a result straight from the install line, in the first and the last lane of a full batch
    return keyed(64, ops={0: "any", 63: "any"}), burst_docs(seed=72), False, INSTANCES, {"n": 0, "t": 0}


def _hand_over():
    # 300 programs on one key: instance n (256 ids in LDS, none beyond) runs out of ids in the fifth batch of the list, instance
    # t with 64 ids in the second; every document that holds the key goes to the general kernel, the one without it stays
    rules = keyed(300)
    docs = burst_docs(seed=73) + [doc([1, 2, NOID, 3, 4, 5, 6, 1, 2])]
    rules.append(("plain", "sequence", 3, [1, 2]))
    switches = {"n": {"SPA_L2_FAST_MAXRULES": "256"}, "t": {"SPA_L2_FAST_SIZE": "t", "SPA_L2_FAST_MAXRULES": "64"}}
    return rules, docs, False, switches, {"n": 3, "t": 3}


CASES = {
    "list-1": lambda: _list_length(1),
    "list-63": lambda: _list_length(63),
    "list-64": lambda: _list_length(64),
    "list-65": lambda: _list_length(65),
    "second-trigger-none": lambda: _second_trigger("none"),
    "second-trigger-all": lambda: _second_trigger("all"),
    "second-trigger-first": lambda: _second_trigger("first"),
    "second-trigger-last": lambda: _second_trigger("last"),
    "three-triggers": _three_triggers,
    "bucket-fill-1": lambda: _bucket_fill(1),
    "bucket-fill-7": lambda: _bucket_fill(7),
    "free-stack": _free_stack,
    "dynamic-after-static": _dynamic_after_static,
    "line-results": _line_results,
    "hand-over": _hand_over,
}
