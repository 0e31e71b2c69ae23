"""The values of the format strings of a finished batch, restated recursively over numpy arrays and Python integers
(include/strus_pattern_amd.h "result values"; csrc/result_values.hpp is the C++ statement, csrc/l2_values.h the device's).
The rule is the project's own restatement of resultformat.Formatter, unpinned by a reference vector."""
import numpy as np

from tests.span_text_model import item_offsets, span_range

SP_VALUE_RESULTS, SP_VALUE_ITEMS = 1, 2
SP_DOC_ERR_RANGE = 5


class Fail(Exception):
    pass


def parse(fmt):
    """bytes -> list of parts: bytes (literal) or (variable name, separator); ValueError when it does not parse"""
    parts, lit, i, n = [], bytearray(), 0, len(fmt)
    while i < n:
        c = fmt[i:i + 1]
        if c == b"\\" and i + 1 < n:
            lit += fmt[i + 1:i + 2]
            i += 2
        elif c == b"{":
            j = fmt.find(b"}", i + 1)
            if j < 0:
                raise ValueError("missing '}'")
            if lit:
                parts.append(bytes(lit))
                lit = bytearray()
            body = fmt[i + 1:j]
            var, bar, sep = body.partition(b"|")
            var = var.strip(bytes(range(33)))
            if not var:
                raise ValueError("empty variable reference")
            parts.append((var, sep if bar else b" "))
            i = j + 1
        else:
            lit += c
            i += 1
    if lit:
        parts.append(bytes(lit))
    return parts


def batch_values(formats, variable_id, results, items, result_format, item_format, doc_offsets, text, seg_offsets,
                 doc_seg_offsets=None, flags=SP_VALUE_RESULTS | SP_VALUE_ITEMS, max_depth=8):
    """formats: the format strings (bytes) of the handles 1..; variable_id: name (bytes) -> handle or 0.
    -> dict: result_values, result_offsets, item_values, item_offsets (None for a family that `flags` leaves out), status"""
    text = bytes(text)
    parsed = [parse(f) for f in formats]
    results = np.asarray(results, np.int64).reshape(-1, 9)
    items = np.asarray(items, np.int64).reshape(-1, 7)
    ndocs = len(doc_offsets) - 1
    ioffs = item_offsets(results, doc_offsets)
    with_formats = bool(formats) and result_format is not None and item_format is not None
    if with_formats:
        result_format = np.asarray(result_format, np.int64).reshape(-1)
        item_format = np.asarray(item_format, np.int64).reshape(-1, 2)

    def evaluate(d, fmt, b, e, depth):
        if depth > max_depth:
            raise Fail()
        out = []
        for part in parsed[fmt - 1]:
            if isinstance(part, bytes):
                out.append(part)
                continue
            v, vals, i = variable_id(part[0]), [], b
            while i < e:
                f, nsub = int(item_format[i, 0]), int(item_format[i, 1])
                follow = i + 1
                if f:
                    if f > len(formats) or i + 1 + nsub > e:
                        raise Fail()
                    follow = i + 1 + nsub
                if v and int(items[i, 0]) == v:
                    if f:
                        vals.append(evaluate(d, f, i + 1, follow, depth + 1))
                    else:
                        r = span_range(items[i, 3:7], d, seg_offsets, doc_seg_offsets, len(text))
                        if r is None:
                            raise Fail()
                        vals.append(text[r[0]:r[0] + r[1]])
                i = follow
            out.append(part[1].join(vals))
        return b"".join(out)

    def value_of(d, fam, i):
        if fam == "result":
            f, b = int(result_format[i]), int(results[i, 7])
            e = b + int(results[i, 8])
        else:
            f, b = int(item_format[i, 0]), i + 1
            e = b + int(item_format[i, 1])
        if not f:
            return b""
        if f > len(formats) or b < ioffs[d] or e > ioffs[d + 1]:
            raise Fail()
        return evaluate(d, f, b, e, 1)

    families = []
    if flags & SP_VALUE_RESULTS:
        families.append(("result", [int(x) for x in doc_offsets]))
    if flags & SP_VALUE_ITEMS:
        families.append(("item", ioffs))
    status = np.zeros(ndocs, np.int32)
    values = {}
    for name, offs in families:
        for d in range(ndocs):
            n = offs[d + 1] - offs[d]
            try:
                got = [value_of(d, name, i) for i in range(offs[d], offs[d + 1])] if with_formats else [b""] * n
                if sum(len(g) for g in got) >= 2 ** 32:
                    raise Fail()
            except Fail:
                status[d] = SP_DOC_ERR_RANGE
                got = [b""] * n
            values[name, d] = got
    out = {"result_values": None, "result_offsets": None, "item_values": None, "item_offsets": None, "status": status}
    for name, offs in families:
        chunks, value_offsets, at = [], [], 0
        for d in range(ndocs):
            for v in values[name, d]:
                value_offsets.append(at)
                if not status[d]:
                    chunks.append(v)
                    at += len(v)
        out[name + "_values"] = b"".join(chunks)
        out[name + "_offsets"] = np.array(value_offsets + [at], np.uint64)
    return out
