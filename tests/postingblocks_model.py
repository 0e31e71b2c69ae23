"""The posting-block rule as include/strus_pattern_amd.h ("posting blocks") states it, in plain Python: the yardstick of the
device-free twin (sp_match_batch_posting_blocks) and, through it, of the device passes.  Written from the header text, not from
the C++: takes the order, the postings and the positions as arrays and B, returns bytes, offsets and totals; and reads them back."""
import numpy as np

FIELDS = ("bytes", "block_offsets", "totals")
SIZES = (1, 2, 4, 8, 16, 32, 64)


class Blocks:
    def __init__(self, bytes, block_offsets, totals, ndict, block_entries):
        self.bytes = bytes                      # (nbytes,) u8
        self.block_offsets = block_offsets      # (nblocks+1,) u64
        self.totals = totals                    # (4,) u64
        self.ndict, self.block_entries = ndict, block_entries


def varint(v):
    """unsigned LEB128 in minimal length"""
    assert 0 <= v < 1 << 64
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def lists_of(order, postings, positions):
    """per sorted position the list [(doc, count, [distinct ordpos ascending])]: what decoding must reproduce.  order: the
    MatchDictionaryOrder, postings: the MatchPostings, positions: the MatchPositions"""
    out = []
    for e in order.order.tolist():
        entry = []
        for p in range(int(postings.entry_offsets[e]), int(postings.entry_offsets[e + 1])):
            occ = positions.occurrences[int(positions.posting_offsets[p]):int(positions.posting_offsets[p + 1]), 0].tolist()
            entry.append((int(postings.records[p, 0]), int(postings.records[p, 2]), sorted(set(occ))))
        out.append(entry)
    return out


def list_code(entry, npos=None):
    """the code of one list [(doc, count, [distinct positions])]; npos: the npos fields where they are not the lengths"""
    body, before = bytearray(), None
    for i, (doc, count, pos) in enumerate(entry):
        body += varint(doc if before is None else doc - before)
        before = doc
        body += varint(count) + varint(len(pos) if npos is None else npos[i])
        prev = None
        for x in pos:
            body += varint(x if prev is None else x - prev)
            prev = x
    return varint(len(body)) + bytes(body)


def posting_blocks(lists, B=16):
    """lists: per sorted position [(doc, count, [distinct positions])]"""
    assert B in SIZES
    out, offsets, gaps = bytearray(), [], 0
    for k, entry in enumerate(lists):
        if k % B == 0:
            offsets.append(len(out))
        out += list_code(entry)
        gaps += sum(len(pos) for _, _, pos in entry)
    offsets.append(len(out))
    totals = [len(offsets) - 1, len(out), B, gaps]
    return Blocks(np.frombuffer(bytes(out), np.uint8).copy(), np.array(offsets, np.uint64), np.array(totals, np.uint64), len(lists), B)


class Malformed(ValueError):
    pass


def read_varint(data, at, end):
    v = 0
    for n in range(10):
        if at >= end:
            raise Malformed("a varint that runs past the block")
        b = data[at]
        at += 1
        v |= (b & 127) << (7 * n)
        if not b & 128:
            if v >> 64:
                raise Malformed("a varint of more than 64 bits")
            return v, at
    raise Malformed("a varint longer than ten bytes")


def decode_block(blocks, j):
    """the lists of block j, from its bytes alone: [[(doc, count, [positions])]]"""
    data = bytes(blocks.bytes)
    at, end = int(blocks.block_offsets[j]), int(blocks.block_offsets[j + 1])
    assert 0 <= at < end <= len(data)
    out = []
    while at < end:
        body, at = read_varint(data, at, end)
        stop = at + body
        assert body and stop <= end
        entry, doc = [], 0
        while at < stop:
            ddelta, at = read_varint(data, at, stop)
            count, at = read_varint(data, at, stop)
            npos, at = read_varint(data, at, stop)
            assert (ddelta or not entry) and 1 <= npos <= count
            doc += ddelta
            pos, x = [], 0
            for i in range(npos):
                gap, at = read_varint(data, at, stop)
                assert gap or not i
                x += gap
                pos.append(x)
            entry.append((doc, count, pos))
        out.append(entry)
    assert len(out) <= blocks.block_entries
    return out


def decode(blocks):
    """all lists in sorted order"""
    return [e for j in range(len(blocks.block_offsets) - 1) for e in decode_block(blocks, j)]


def assert_same(got, want):
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (name, a, b)
        assert a.tobytes() == b.tobytes(), name
    assert got.ndict == want.ndict and got.block_entries == want.block_entries


def check_invariants(blocks, want_lists):
    """the invariants of the header"""
    B, n = int(blocks.block_entries), len(want_lists)
    nblocks = (n + B - 1) // B
    assert blocks.ndict == n and len(blocks.block_offsets) == nblocks + 1
    offs = blocks.block_offsets.astype(np.int64)
    assert int(offs[0]) == 0 and int(offs[-1]) == len(blocks.bytes) and (np.diff(offs) > 0).all()      # ascending, no block empty
    assert blocks.totals.tolist() == [nblocks, len(blocks.bytes), B, sum(len(pos) for entry in want_lists for _, _, pos in entry)]
    assert decode(blocks) == want_lists
    for j in range(nblocks):
        assert len(decode_block(blocks, j)) == min(B, n - j * B)
        assert int(offs[j + 1] - offs[j]) >= 5 * min(B, n - j * B)          # a list is at least body and one posting of four varints
