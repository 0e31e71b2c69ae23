"""The value cases of the dictionary order that its CPU tests (tests/test_dictorder_abi.py) and its GPU tests
(tests/test_dictorder_gpu.py) share: lists of (handle, value bytes) per document, every pair distinct over the batch unless a
case says otherwise.  Needs no device and no library."""

LONG = b"0123456789abcdefghijklmnopqrstuvwxyz"


def _differ_after(n):
    """two values equal in their first n bytes that differ in the next one, and one that ends there"""
    head = (LONG * 2)[:n]
    return [head + b"b" + b"tail", head + b"a" + b"tail", head]


def comparator_values(handle=2, other=5):
    """the comparator edges, in an order that is not the sorted one: (handle, value) pairs"""
    values = [
        b"",                                                    # the empty value: the first of its handle
        b"abc", b"ab", b"abcd", b"abcde",                       # a value that is a prefix of another
        b"a\0\0\0\0", b"a\0\0\0", b"a\0", b"a",                 # zero padding: all tie on the key of four bytes
        b"\x80", b"\x7f", b"\xfe\x01", b"\x01\xfe", b"zz\xc3\xa9", b"zz\x7f",       # bytes >= 0x80 against bytes < 0x80
    ]
    for n in (4, 15, 16, 17):
        values += _differ_after(n)
    pairs = [(handle, v) for v in values]
    pairs += [(other, b"abc"), (other, b""), (1, b"abc")]       # the same bytes under other handles
    assert len(set(pairs)) == len(pairs)
    return pairs


def long_prefix_group(handle=3, n=70, prefix=300):
    """n values that share `prefix` bytes and differ in the last byte: tie paths longer than a wave, compares longer than any
    fast path; descending"""
    head = (LONG * (prefix // len(LONG) + 1))[:prefix]
    return [(handle, head + bytes([33 + n - 1 - k])) for k in range(n)]


def numbered(n, nhandles=7, arrival="shuffle"):
    """n distinct terms b"t%06d" spread over `nhandles` handles, arriving ascending by (handle, value), descending, or in a
    fixed shuffle"""
    pairs = [(1 + k % nhandles, b"t%06d" % k) for k in range(n)]
    if arrival == "ascending":
        return sorted(pairs)
    if arrival == "descending":
        return sorted(pairs, reverse=True)
    assert arrival == "shuffle" and (n < 2 or n % 7919)         # (7919 is prime: k -> 7919 k + 13 mod n is a permutation)
    return [pairs[(k * 7919 + 13) % n] for k in range(n)]


def in_documents(pairs, size=97):
    """the pairs cut into documents of `size` terms"""
    return [pairs[i:i + size] for i in range(0, len(pairs), size)] or [[]]
