"""bench.py builds its corpus with text_corpus(), an array restatement of synth.text_documents(): the
bytes and the document offsets must be the generator's, so that the benchmark scans what it always
scanned and two runs (or two builds) with the same arguments see identical inputs."""
import numpy as np
import pytest

import bench
from struspattern_amd import synth

CASES = [
    # (vocabulary size, documents, bytes per document, seed, utf8)
    (30000, 120, 16384, 1000, True),     # the head of the pipeline corpus; crosses a stretch of the stream
    (30000, 12, 65536, 1000, False),     # the lexer workload's shape
    (30000, 40, 16384, 1001, True),
    (2000, 60, 3000, 2, True),
    (500, 50, 700, 5, False),
    (100, 300, 64, 9, True),             # documents end after a few tokens
    (30000, 10, 20, 11, True),
]


@pytest.mark.parametrize("nvocab,ndocs,docbytes,seed,utf8", CASES)
def test_text_corpus_equals_the_generator(nvocab, ndocs, docbytes, seed, utf8):
    vocab = synth.vocabulary(nvocab, 1)
    text, offs = synth.text_documents(ndocs, docbytes, vocab, seed, utf8=utf8)
    got, got_offs = bench.text_corpus(ndocs, docbytes, vocab, seed, utf8=utf8)
    assert got.dtype == np.uint8 and got_offs.dtype == np.uint64
    assert np.array_equal(got_offs, offs)
    assert got.tobytes() == text
