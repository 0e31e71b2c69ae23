"""The term-block rule as include/strus_pattern_amd.h ("term blocks") states it, in plain Python: the yardstick of the device-free
twin (sp_match_batch_term_blocks) and, through it, of the device passes.  Written from the header text, not from the C++: takes
the sorted (handle, value, doc_freq, count) list and B, returns bytes, offsets, handles and totals; and reads them back."""
import numpy as np

FIELDS = ("bytes", "block_offsets", "block_handles", "totals")
SIZES = (1, 2, 4, 8, 16, 32, 64)


class Blocks:
    def __init__(self, bytes, block_offsets, block_handles, totals, ndict, block_entries):
        self.bytes = bytes                      # (nbytes,) u8
        self.block_offsets = block_offsets      # (nblocks+1,) u64
        self.block_handles = block_handles      # (nblocks,) u32
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


def shared(a, b):
    n = 0
    while n < len(a) and n < len(b) and a[n] == b[n]:
        n += 1
    return n


def code(head, before, entry):
    """the code of `entry` = (handle, value, doc_freq, count) behind `before` (None at position 0)"""
    h, v, df, count = entry
    hdelta = same = 0
    if not head:
        hdelta = h - before[0]
        same = shared(before[1], v) if before[0] == h else 0
    assert hdelta >= 0
    return varint(hdelta) + varint(same) + varint(len(v) - same) + varint(df) + varint(count) + v[same:]


def term_blocks(entries, B=16):
    """entries: (handle, value bytes, doc_freq, count) per sorted position"""
    assert B in SIZES
    entries = [(int(h), bytes(v), int(df), int(c)) for h, v, df, c in entries]
    out, offsets, handles = bytearray(), [], []
    for k, e in enumerate(entries):
        if k % B == 0:
            offsets.append(len(out))
            handles.append(e[0])
        out += code(k % B == 0, entries[k - 1] if k else None, e)
    offsets.append(len(out))
    totals = [len(handles), len(out), B, sum(len(e[1]) for e in entries)]
    return Blocks(np.frombuffer(bytes(out), np.uint8).copy(), np.array(offsets, np.uint64), np.array(handles, np.uint32).reshape(-1),
                  np.array(totals, np.uint64), len(entries), B)


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
    """[(handle, value, doc_freq, count)] of block j, from its bytes and its handle alone; with the fields as coded:
    [(hdelta, shared, suffix)]"""
    data = bytes(blocks.bytes)
    at, end = int(blocks.block_offsets[j]), int(blocks.block_offsets[j + 1])
    assert 0 <= at < end <= len(data)
    handle, before, out, fields = int(blocks.block_handles[j]), b"", [], []
    while at < end:
        hdelta, at = read_varint(data, at, end)
        same, at = read_varint(data, at, end)
        suffix, at = read_varint(data, at, end)
        df, at = read_varint(data, at, end)
        count, at = read_varint(data, at, end)
        if same > len(before):
            raise Malformed("a shared prefix above the previous value's length")
        if suffix > end - at:
            raise Malformed("a suffix that runs past the block")
        assert out or (hdelta == 0 and same == 0)
        handle += hdelta
        before = before[:same] + data[at:at + suffix]
        at += suffix
        out.append((handle, before, df, count))
        fields.append((hdelta, same, suffix))
    assert len(out) <= blocks.block_entries
    return out, fields


def decode(blocks):
    """all entries in sorted order"""
    return [e for j in range(len(blocks.block_handles)) for e in decode_block(blocks, j)[0]]


def sorted_entries(d, entries, order):
    """(handle, value, doc_freq, count) per sorted position: d the MatchDictionary, entries its (handle, value) pairs, order the
    MatchDictionaryOrder"""
    return [(entries[int(e)][0], entries[int(e)][1], int(d.records[int(e), 4]), int(d.counts[int(e)])) for e in order.order]


def assert_same(got, want):
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (name, a, b)
        assert a.tobytes() == b.tobytes(), name
    assert got.ndict == want.ndict and got.block_entries == want.block_entries


def check_invariants(blocks, want_entries):
    """the invariants of the header"""
    B, n = int(blocks.block_entries), len(want_entries)
    nblocks = (n + B - 1) // B
    assert blocks.ndict == n and len(blocks.block_handles) == nblocks and len(blocks.block_offsets) == nblocks + 1
    offs = blocks.block_offsets.astype(np.int64)
    assert int(offs[0]) == 0 and int(offs[-1]) == len(blocks.bytes) and (np.diff(offs) > 0).all()      # ascending, no block empty
    assert blocks.totals.tolist() == [nblocks, len(blocks.bytes), B, sum(len(e[1]) for e in want_entries)]
    assert decode(blocks) == [(int(h), bytes(v), int(df), int(c)) for h, v, df, c in want_entries]
    for j in range(nblocks):
        assert int(blocks.block_handles[j]) == want_entries[j * B][0]
        assert len(decode_block(blocks, j)[0]) == min(B, n - j * B)
