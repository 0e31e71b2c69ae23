"""strusPatternMatch-like command line: load a rule program, run documents
through the MI355X lexer + rule automaton, print tokens (-K) and results in the reference tool's
listing format (doc/webpage/introduction_struspattern.htm:178-260).

    python -m struspattern_amd.match -p program.rul [-K] [-o ORIGIN] [--paragraphs] [--frequencies] [--device-values] [--terms] [--dictionary] [--postings] [--positions] [--sorted] [--blocks] [--posting-blocks] [--lookup NAME=VALUE ...] [--lookup-prefix] file [file ...]

Every file is one document (plain UTF-8 text; the reference tool segments XML with strusAnalyzer's
segmenters, which are outside this engine -- pass -o to add the offset of the text inside its original
file to the printed positions).  With --paragraphs every file is a segmented document: its paragraphs
(split at runs of empty lines, which belong to no segment) go to the lexer one by one, are stitched to
the document on the GPU, and positions are printed through the segment position map
(`segmentposmap[seg] + ofs`, as the reference's printResults does; -o adds on top).  With --frequencies the
listing of a file is followed by one line per pattern that matched in it, ascending by pattern handle:
`frequency NAME: count N first ORDPOS last ORDEND` -- how often, the first ordinal position a match starts at
and the last one a match ends at, summed on the GPU (finishedPatternFreqDevice).  With --device-values the values of
the format strings in the listing are built on the GPU (finishedValuesDevice) instead of resultformat.Formatter; the listing
is the same.  With --terms the listing of a file is followed by one line per index term of it -- a distinct pair of pattern
and value, the value of a result being that of its format string, or the text it covers where it has none -- ascending by
pattern handle, then by first occurrence: `term NAME 'VALUE': count N first ORDPOS`, grouped on the GPU
(finishedTermsDevice).  With --dictionary the listing of the last file is followed by one line per distinct index term of
all files, in the order of first occurrence: `dict NAME 'VALUE': docs D count C` -- in how many files the term occurs and how
often over all of them, built on the GPU from the terms (finishedDictionaryDevice).  --postings implies --dictionary; the
dictionary lines are followed by one line per entry, in the same order, with the files that hold the term in the order given:
`post NAME 'VALUE': FILEINDEX:COUNT@FIRSTPOS ...` -- the index of the file among the arguments (from 0), how often the term
occurs in it and the first ordinal position it starts at, built on the GPU from the dictionary (finishedPostingsDevice).
--positions implies --postings; every FILEINDEX:COUNT@FIRSTPOS is followed by the distinct ordinal positions the term starts at
in that file, ascending: `FILEINDEX:COUNT@FIRSTPOS[POS,POS,...]`, built on the GPU from the postings (finishedPositionsDevice).
--sorted implies --dictionary; the `dict` lines, and the `post` lines with them, come by pattern handle and then by value (bytes)
instead of first occurrence, ranked on the GPU from the dictionary (finishedDictionaryOrderDevice): they are then the same in
whatever order the files are named, up to the file indices inside the `post` lines.
--blocks implies --sorted; the sorted dictionary is written as front-coded term blocks on the GPU (finishedTermBlocksDevice) and,
read back from the blocks alone, listed behind the other lines: one line per block, `block J NAME: entries N bytes M head 'VALUE'`
-- the pattern and the value of its head --, and `blocks J bytes M uncoded value bytes U`.  These lines do not depend on the
order of the files.
--posting-blocks implies --blocks and --positions; the posting lists with their positions are written in the sorted order as
delta-coded posting blocks on the GPU (finishedPostingBlocksDevice) and, read back from the blocks alone, listed behind the `block`
lines: one line per block, `postblock J: lists N postings M positions Q bytes X`, and `postblocks J bytes X positions Q`.  List k
of these blocks is the term at position k of the term blocks.  The lines do not depend on the order of the files.
--lookup NAME=VALUE (repeatable) implies --blocks and --posting-blocks; the two block products are copied into a segment on the GPU
(Segment.fromContext) and the terms of pattern NAME with the value VALUE -- with --lookup-prefix: whose value starts with VALUE --
looked up there, all queries in one call (lookupDevice): behind the `postblock` lines one line `lookup NAME 'VALUE': terms N` per
query and per term found its `post` line as --positions prints it, decoded from the segment instead of read from the fetched arrays.
All files go to the GPU as one batch.  There is no CPU fallback.
"""
import argparse
import sys

import numpy as np

import struspattern_amd as spa
from struspattern_amd import rulelang, segments


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m struspattern_amd.match", description=__doc__.split("\n\n")[0])
    ap.add_argument("-p", "--program", required=True, help="rule program file")
    ap.add_argument("-K", "--tokens", action="store_true", help="also print the tokens recognized")
    ap.add_argument("-o", "--origin", type=int, default=0, help="offset added to the printed byte positions")
    ap.add_argument("--paragraphs", action="store_true", help="every file is a document whose segments are its paragraphs")
    ap.add_argument("--frequencies", action="store_true", help="after the listing of a file, one line per pattern that matched in it")
    ap.add_argument("--device-values", action="store_true", help="the values of the format strings are built on the device")
    ap.add_argument("--terms", action="store_true", help="after the listing of a file, one line per distinct (pattern, value) of it")
    ap.add_argument("--dictionary", action="store_true", help="after the last listing, one line per distinct (pattern, value) of all files")
    ap.add_argument("--postings", action="store_true", help="implies --dictionary; after its lines, per distinct (pattern, value) the files that hold it")
    ap.add_argument("--positions", action="store_true", help="implies --postings; after every file of a posting line, the distinct positions of the term in it")
    ap.add_argument("--sorted", action="store_true", help="implies --dictionary; its lines and those of --postings by pattern, then by value")
    ap.add_argument("--blocks", action="store_true", help="implies --sorted; after its lines, the front-coded term blocks of the sorted dictionary")
    ap.add_argument("--posting-blocks", action="store_true", help="implies --blocks and --positions; after the term blocks, the delta-coded posting blocks in the same order")
    ap.add_argument("--lookup", action="append", default=[], metavar="NAME=VALUE", help="implies --blocks and --posting-blocks; the postings of the term, looked up in the segment on the device")
    ap.add_argument("--lookup-prefix", action="store_true", help="the terms of --lookup are those whose value starts with VALUE")
    ap.add_argument("-d", "--device", type=int, default=0)
    ap.add_argument("files", nargs="+")
    args = ap.parse_args(argv)
    args.posting_blocks = args.posting_blocks or bool(args.lookup)
    args.blocks = args.blocks or args.posting_blocks
    args.positions = args.positions or args.posting_blocks
    args.postings = args.postings or args.positions
    args.sorted = args.sorted or args.blocks
    args.dictionary = args.dictionary or args.postings or args.sorted

    with open(args.program, encoding="utf-8") as f:
        program = f.read()
    lx, mt = spa.PatternLexerInstance(), spa.PatternMatcherInstance()
    prg = rulelang.load(program, lx, mt)

    docs = []
    for fn in args.files:
        with open(fn, "rb") as f:
            docs.append(f.read())
    if args.paragraphs:
        return paragraphs(args, prg, lx, mt, docs)
    text = b"".join(docs)
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs])

    lb = lx.createContext(args.device).matchDocs(text, offs)
    mctx = mt.createContext(args.device)
    mb = mctx.matchDocs(lb.lexems, lb.doc_offsets)
    values = device_values(mctx, text, offs) if args.device_values else None
    terms = device_terms(mctx, text, offs) if args.terms or args.dictionary else None
    dictionary = device_dictionary(mctx) if args.dictionary else None
    postings = device_postings(mctx) if args.postings else None
    positions = device_positions(mctx) if args.positions else None
    order = device_dictionary_order(mctx) if args.sorted else None
    blocks = device_term_blocks(mctx) if args.blocks else None
    posting_blocks = device_posting_blocks(mctx) if args.posting_blocks else None
    freq = frequencies(mctx) if args.frequencies else None
    for di, fn in enumerate(args.files):
        print("%s:" % fn)
        doc = docs[di]
        if args.tokens:
            for line in rulelang.format_tokens(prg, doc, lb.doc(di)):
                print(line)
        res = mb.doc(di)
        for line in rulelang.format_results(doc, res, mb.items, mt.patternName, mt.variableName, origin=args.origin,
                                            result_format=mb.result_format, item_format=mb.item_format, format_string=mt.formatString,
                                            first_result=int(mb.doc_offsets[di]), values=values):
            print(line)
        print_frequencies(freq, di, mt)
        print_terms(terms if args.terms else None, di, mt)
    print_dictionary(dictionary, terms, mt, order)
    print_postings(postings, dictionary, terms, mt, positions, order)
    print_blocks(blocks, mt)
    print_posting_blocks(posting_blocks)
    print_lookups(args, mctx, mt)
    print("OK done")
    return 0


def device_dictionary(mctx):
    """--dictionary: the dictionary of the terms that device_terms grouped, built on the device"""
    mctx.finishedDictionaryDevice()
    return mctx.finishedDictionaryFetch()


def device_dictionary_order(mctx):
    """--sorted: the entries of the dictionary that device_dictionary built, ranked by (pattern handle, value) on the device"""
    mctx.finishedDictionaryOrderDevice()
    return mctx.finishedDictionaryOrderFetch()


def device_term_blocks(mctx):
    """--blocks: the dictionary in the order that device_dictionary_order built, front-coded in blocks on the device"""
    mctx.finishedTermBlocksDevice()
    return mctx.finishedTermBlocksFetch()


def block_lines(blocks, pattern_name):
    """the lines of --blocks, from the blocks alone"""
    lines = []
    for j in range(len(blocks.block_handles)):
        entries = blocks.block(j)
        lines.append("block %d %s: entries %d bytes %d head '%s'" % (j, pattern_name(entries[0][0]), len(entries), int(blocks.block_offsets[j + 1] - blocks.block_offsets[j]),
                                                                      entries[0][1].decode("utf-8", "replace")))
    return lines + ["blocks %d bytes %d uncoded value bytes %d" % (len(blocks.block_handles), len(blocks.bytes), int(blocks.totals[3]))]


def device_posting_blocks(mctx):
    """--posting-blocks: the postings and their positions in the order that device_dictionary_order built, delta-coded in the
    blocks of the term blocks on the device"""
    mctx.finishedPostingBlocksDevice()
    return mctx.finishedPostingBlocksFetch()


def posting_block_lines(blocks):
    """the lines of --posting-blocks, from the blocks alone"""
    lines = []
    for j in range(len(blocks.block_offsets) - 1):
        lists = blocks.block(j)
        lines.append("postblock %d: lists %d postings %d positions %d bytes %d" % (j, len(lists), sum(len(q) for q in lists), sum(len(p[2]) for q in lists for p in q),
                                                                                    int(blocks.block_offsets[j + 1] - blocks.block_offsets[j])))
    return lines + ["postblocks %d bytes %d positions %d" % (len(blocks.block_offsets) - 1, len(blocks.bytes), int(blocks.totals[3]))]


def lookup_lines(segment, queries, prefix, pattern_name):
    """the lines of --lookup; queries: (handle, value bytes) each, looked up in one call"""
    segment.lookupDevice(queries, prefix=prefix)
    found = segment.lookupFetch()
    lines = []
    for i, (h, q) in enumerate(queries):
        if int(found.q_status[i]) != 0:
            raise spa.PatternError("lookup of %s '%s' failed: status %d" % (pattern_name(h), q.decode("utf-8", "replace"), int(found.q_status[i])))
        lines.append("lookup %s '%s': terms %d" % (pattern_name(h), q.decode("utf-8", "replace"), int(found.q_count[i])))
        for handle, value, _, _, postings in found.query(i):
            lines.append("post %s '%s': %s" % (pattern_name(handle), value.decode("utf-8", "replace"),
                                               " ".join("%d:%d@%d[%s]" % (doc, count, pos[0], ",".join("%d" % x for x in pos)) for doc, count, pos in postings)))
    return lines


def print_lookups(args, mctx, mt):
    """--lookup: a segment of the blocks built last on the context answers the queries"""
    if not args.lookup:
        return
    queries = []
    for spec in args.lookup:
        name, sep, value = spec.partition("=")
        handle = mt.patternId(name)
        if not sep or not handle:
            raise spa.PatternError("--lookup wants NAME=VALUE with the name of a pattern: '%s'" % spec)
        queries.append((handle, value.encode("utf-8")))
    segment = spa.Segment.fromContext(mctx)
    try:
        for line in lookup_lines(segment, queries, args.lookup_prefix, mt.patternName):
            print(line)
    finally:
        segment.close()


def print_posting_blocks(blocks):
    if blocks is None:
        return
    for line in posting_block_lines(blocks):
        print(line)


def print_blocks(blocks, mt):
    if blocks is None:
        return
    for line in block_lines(blocks, mt.patternName):
        print(line)


def in_order(lines, order):
    """one line per dictionary entry, as they are or in the order of --sorted"""
    return lines if order is None else [lines[int(e)] for e in order.order]


def dictionary_lines(dictionary, found, pattern_name, order=None):
    """the lines of --dictionary; found: (batch, text, values, terms) of the terms call; order: that of --sorted"""
    mb, mt, mv, terms = found
    return in_order(["dict %s '%s': docs %d count %d" % (pattern_name(int(h)), value.decode("utf-8", "replace"), docs, count)
                     for h, value, docs, count, _ in dictionary.entries(mb, terms, values=mv, text=mt)], order)


def print_dictionary(dictionary, found, mt, order=None):
    if dictionary is None:
        return
    for line in dictionary_lines(dictionary, found, mt.patternName, order):
        print(line)


def device_postings(mctx):
    """--postings: the postings of the dictionary that device_dictionary built, partitioned on the device"""
    mctx.finishedPostingsDevice()
    return mctx.finishedPostingsFetch()


def device_positions(mctx):
    """--positions: the positions of the postings that device_postings built, partitioned on the device"""
    mctx.finishedPositionsDevice()
    return mctx.finishedPositionsFetch()


def postings_lines(postings, dictionary, found, pattern_name, positions=None, order=None):
    """the lines of --postings; found: (batch, text, values, terms) of the terms call; positions: those of --positions; order:
    that of --sorted"""
    mb, mt, mv, terms = found

    def where(p):
        return "" if positions is None else "[%s]" % ",".join("%d" % pos for pos in positions.positions(p).tolist())

    return in_order(["post %s '%s': %s" % (pattern_name(int(h)), value.decode("utf-8", "replace"),
                                           " ".join("%d:%d@%d%s" % (doc, count, first, where(int(postings.entry_offsets[e]) + k))
                                                    for k, (doc, _, count, first) in enumerate(postings.entry(e).tolist())))
                     for e, (h, value, _, _, _) in enumerate(dictionary.entries(mb, terms, values=mv, text=mt))], order)


def print_postings(postings, dictionary, found, mt, positions=None, order=None):
    if postings is None:
        return
    for line in postings_lines(postings, dictionary, found, mt.patternName, positions, order):
        print(line)


def uploaded(text, offs):
    """the text source arguments (d_text, nbytes, d_seg_offsets, nseg) of a device call for `text`, every document one segment,
    and the device tensors they point into, which the caller holds until it has fetched"""
    import torch
    d_text = torch.frombuffer(bytearray(text + b"\0" * 16), dtype=torch.uint8).cuda()
    d_so = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64)).cuda()
    return (d_text.data_ptr(), len(text), d_so.data_ptr(), len(offs) - 1), (d_text, d_so)


def device_terms(mctx, text, offs):
    """--terms: the last batch of the context finished on the device, its values and the text of its results built there and
    the results grouped into terms; every document is one segment of `text`.  Returns (batch, text, values, terms)."""
    source, held = uploaded(text, offs)
    mctx.batchFinishDevice()
    mctx.finishedValuesDevice(*source, flags=spa.SP_VALUE_RESULTS)
    mctx.finishedTextDevice(*source, items=False)
    mctx.finishedTermsDevice()
    return mctx.finishedFetch(), mctx.finishedTextFetch(), mctx.finishedValuesFetch(), mctx.finishedTermsFetch()


def term_lines(found, di, pattern_name):
    """the lines of --terms for document di; found: (batch, text, values, terms) of the terms call"""
    mb, mt, mv, terms = found
    if int(terms.status[di]) != 0:
        raise spa.PatternError("no terms of document %d: status %d" % (di, int(terms.status[di])))
    return ["term %s '%s': count %d first %d" % (pattern_name(int(h)), value.decode("utf-8", "replace"), count, first)
            for h, value, count, first, _ in terms.terms(di, mb, values=mv, text=mt)]


def print_terms(found, di, mt):
    if found is None:
        return
    for line in term_lines(found, di, mt.patternName):
        print(line)


def device_values(mctx, text, offs):
    """--device-values: the last batch of the context finished on the device and the values of its format strings built
    there; every document is one segment of `text`"""
    source, held = uploaded(text, offs)
    mctx.batchFinishDevice()
    mctx.finishedValuesDevice(*source)
    values = mctx.finishedValuesFetch()
    if np.any(values.status != 0):
        raise spa.PatternError("no values of document %d: status %d" % (int(np.flatnonzero(values.status)[0]), int(values.status.max())))
    return values


def frequencies(mctx):
    """--frequencies: the last batch of the context finished on the device and its pattern frequencies summed there"""
    mctx.batchFinishDevice()
    mctx.finishedPatternFreqDevice()
    return mctx.finishedPatternFreqFetch()


def print_frequencies(freq, di, mt):
    if freq is None:
        return
    if int(freq.status[di]) != 0:
        raise spa.PatternError("no pattern frequencies of document %d: status %d" % (di, int(freq.status[di])))
    for handle, count, first, last in freq.doc(di):
        print("frequency %s: count %d first %d last %d" % (mt.patternName(int(handle)), count, first, last))


def paragraphs(args, prg, lx, mt, docs):
    """--paragraphs: lexer per segment -> stitch on the device -> matcher; the listing through the segment position map"""
    text, seg_offsets, doc_seg_offsets, posmaps = segments.segmented_batch(docs)
    lctx = lx.createContext(args.device)
    mctx = mt.createContext(args.device)
    # (terms need text and values; every later product implies the ones before it)
    with_terms = args.terms or args.dictionary
    found = spa.matchSegmentedDocs(lctx, mctx, text, seg_offsets, doc_seg_offsets, with_values=args.device_values, with_terms=with_terms,
                                   with_dictionary=args.dictionary, with_postings=args.postings, with_positions=args.positions,
                                   with_dictionary_order=args.sorted, with_term_blocks=args.blocks, with_posting_blocks=args.posting_blocks)
    order = blocks = posting_blocks = None
    if args.posting_blocks:
        found, posting_blocks = found[:-1], found[-1]                           # (the posting blocks come last, behind the term blocks)
    if args.blocks:
        found, blocks = found[:-1], found[-1]                                   # (the blocks come last, behind the order)
    if args.sorted:
        found, order = found[:-1], found[-1]                                    # (the order comes last, whatever else was asked for)
    names = ("batch", "text", "values", "terms", "dictionary", "postings", "positions") if with_terms else ("batch", "values")
    got = dict(zip(names, found if isinstance(found, tuple) else (found,)))     # (the products asked for, a prefix of the names)
    mb, dictionary, postings, positions = got["batch"], got.get("dictionary"), got.get("postings"), got.get("positions")
    terms = (mb, got["text"], got["values"], got["terms"]) if with_terms else None
    values = got.get("values") if args.device_values else None
    if np.any(mb.status != 0):
        bad = int(np.flatnonzero(mb.status)[0])
        raise spa.PatternError("at least one document failed: %s has status %d" % (args.files[bad], int(mb.status[bad])))
    freq = frequencies(mctx) if args.frequencies else None
    lb, origseg = lctx.stitchedFetch()
    items = np.zeros((0, 7), np.int64)
    for di, fn in enumerate(args.files):
        print("%s:" % fn)
        doc, posmap = docs[di], posmaps[di]
        a, b = int(lb.doc_offsets[di]), int(lb.doc_offsets[di + 1])
        if args.tokens:
            for line in rulelang.format_tokens(prg, doc, segments.absolute_lexems(lb.lexems[a:b], origseg[a:b], posmap)):
                print(line)
        res = segments.absolute_records(mb.doc(di), posmap)
        if len(res):
            # (the items of a document are one block in result order)
            ia, ib = int(res[0, 7]), int(res[-1, 7] + res[-1, 8])
            items = np.zeros((ib, 7), np.int64)
            items[ia:ib] = segments.absolute_records(mb.items[ia:ib], posmap)
        for line in rulelang.format_results(doc, res, items, mt.patternName, mt.variableName, origin=args.origin,
                                            result_format=mb.result_format, item_format=mb.item_format, format_string=mt.formatString,
                                            first_result=int(mb.doc_offsets[di]), values=values):
            print(line)
        print_frequencies(freq, di, mt)
        print_terms(terms if args.terms else None, di, mt)
    print_dictionary(dictionary, terms, mt, order)
    print_postings(postings, dictionary, terms, mt, positions, order)
    print_blocks(blocks, mt)
    print_posting_blocks(posting_blocks)
    print_lookups(args, mctx, mt)
    print("OK done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
