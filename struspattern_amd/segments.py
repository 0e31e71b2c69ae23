"""Host side of segmented documents: cutting a text into paragraph segments and mapping segment-relative positions back
to the file, as the reference's tools print them (tests/utils/testUtils.cpp:125-150: `segmentposmap[ origpos().seg() ] + ofs`).
The stitch itself runs on the device (PatternLexerContext.stitchSegmentsDevice, matchSegmentedDocs)."""
import re

import numpy as np

# the newline that ends a paragraph's last line and the empty (blank) lines behind it
_SEPARATOR = re.compile(rb"\n(?:[ \t\r]*\n)+")


def split_paragraphs(data):
    """The paragraphs of `data` (bytes), split at runs of empty lines: list of (start, end) byte ranges.  The separator
    bytes belong to no segment; a piece without bytes (the file starts or ends with a separator) is no segment."""
    out, at = [], 0
    for m in _SEPARATOR.finditer(data):
        if m.start() > at:
            out.append((at, m.start()))
        at = m.end()
    if at < len(data):
        out.append((at, len(data)))
    return out


def segmented_batch(docs):
    """docs: list of bytes -> (text of all segments back to back, seg_offsets (nseg+1,) u64, doc_seg_offsets (ndocs+1,) u64,
    posmaps: per document the start of each of its segments in the document)"""
    pieces, posmaps, dso = [], [], [0]
    for data in docs:
        ranges = split_paragraphs(data)
        pieces += [data[a:b] for a, b in ranges]
        posmaps.append(np.array([a for a, _ in ranges], np.int64))
        dso.append(len(pieces))
    seg_offsets = np.zeros(len(pieces) + 1, np.uint64)
    seg_offsets[1:] = np.cumsum([len(p) for p in pieces])
    return b"".join(pieces), seg_offsets, np.array(dso, np.uint64), posmaps


def absolute_lexems(lexems, origseg, posmap):
    """lexems (n,4) of one stitched document with origpos relative to the segment -> relative to the document"""
    out = np.array(lexems, np.int64).reshape(-1, 4)
    if len(out):
        out[:, 2] += posmap[np.asarray(origseg, np.int64)]
    return out


def absolute_records(records, posmap):
    """result (n,9) or item (m,7) records: (origseg, origpos) and (origendseg, origend) -> positions in the document
    (the segment columns stay)"""
    out = np.array(records, np.int64)
    if len(out):
        out[:, 4] += posmap[out[:, 3]]
        out[:, 6] += posmap[out[:, 5]]
    return out
