"""The dictionary-order rule as include/strus_pattern_amd.h ("dictionary order") states it, in plain Python: the yardstick of the
device-free twin (sp_match_batch_dictionary_order) and, through it, of the device passes.  Written from the header text, not from
the C++: `sorted` over (handle, bytes) tuples -- Python compares bytes as memcmp does, unsigned, a prefix before what it is a prefix
of."""
import numpy as np

FIELDS = ("order", "rank", "prefix_bytes", "handle_offsets")


class Order:
    def __init__(self, order, rank, prefix_bytes, handle_offsets):
        self.order = order                      # (ndict,) u32
        self.rank = rank                        # (ndict,) u32
        self.prefix_bytes = prefix_bytes        # (ndict,) u32
        self.handle_offsets = handle_offsets    # (handle_bound+1,) u64


def shared(a, b):
    """the leading bytes that a and b share"""
    n = 0
    while n < len(a) and n < len(b) and a[n] == b[n]:
        n += 1
    return n


def dictionary_order(entries, handle_terms):
    """entries: (handle, value bytes) per dictionary entry, distinct; handle_terms: the entries per handle"""
    entries = [(int(h), bytes(v)) for h, v in entries]
    assert len(set(entries)) == len(entries)
    order = sorted(range(len(entries)), key=lambda e: entries[e])
    rank = np.zeros(len(entries), np.uint32)
    prefix = np.zeros(len(entries), np.uint32)
    for k, e in enumerate(order):
        rank[e] = k
        if k and entries[order[k - 1]][0] == entries[e][0]:
            prefix[k] = shared(entries[order[k - 1]][1], entries[e][1])
    offsets = np.zeros(len(handle_terms) + 1, np.uint64)
    offsets[1:] = np.cumsum(np.asarray(handle_terms, np.uint64))
    return Order(np.array(order, np.uint32).reshape(-1), rank, prefix, offsets)


def entries_of(mb, terms, d, values=None, text=None):
    """(handle, value bytes) per entry of the MatchDictionary d, in dictionary order"""
    return [(h, bytes(v)) for h, v, _, _, _ in d.entries(mb, terms, values=values, text=text)]


def of_batch(mb, terms, d, values=None, text=None):
    """the model's order of a MatchDictionary and what it was built from"""
    return dictionary_order(entries_of(mb, terms, d, values, text), d.handle_terms)


def assert_same(got, want):
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (name, a, b)
        assert a.tobytes() == b.tobytes(), name


def check_invariants(o, entries, handle_terms):
    """the invariants of the header, from the order and the (handle, value bytes) of the entries"""
    n = len(entries)
    assert len(o.order) == len(o.rank) == len(o.prefix_bytes) == n and len(o.handle_offsets) == len(handle_terms) + 1
    assert np.array_equal(np.sort(o.order), np.arange(n, dtype=np.uint32))             # a permutation
    assert np.array_equal(o.rank[o.order], np.arange(n, dtype=np.uint32))              # rank is its inverse
    offs = o.handle_offsets.astype(np.int64)
    assert int(offs[0]) == 0 and int(offs[-1]) == n and np.array_equal(np.diff(offs), np.asarray(handle_terms, np.int64))
    for h in range(len(handle_terms)):
        assert all(entries[int(e)][0] == h for e in o.order[int(offs[h]):int(offs[h + 1])]), h
    for k in range(1, n):
        (ha, a), (hb, b) = entries[int(o.order[k - 1])], entries[int(o.order[k])]
        assert ha <= hb                                                                # handles do not descend
        p = int(o.prefix_bytes[k])
        if ha != hb:
            assert p == 0
            continue
        assert p <= min(len(a), len(b)) and a[:p] == b[:p]
        assert len(a) == p or (len(b) > p and a[p] < b[p])                             # the next byte ascends strictly, or the left value ends
    if n:
        assert int(o.prefix_bytes[0]) == 0
