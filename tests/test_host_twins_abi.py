"""What the five device-free twins of the products of a finished batch share (csrc/finished_host.hpp): each of spa.batchText,
batchValues, batchPatternFreq, batchTerms and batchDictionary refuses the same three malformed batches -- document offsets that
do not start at 0, that descend, that do not cover the results -- with SP_ERR_INVALID, and the same objects then serve a
well-formed call whose answer is written out by hand.  One document, two results, a text of 4 bytes: the smallest shape that
can express all three conditions.  Needs no device."""
import functools

import numpy as np
import pytest

import struspattern_amd as spa
from tests.test_result_values_abi import matcher_of

V, T = spa.SP_TERM_VALUES, spa.SP_TERM_TEXT
TEXT, SEGMENTS = b"abcd", [0, 4]
BOUND = 3
BAD_OFFSETS = {"not starting at 0": [1, 2], "descending": [2, 1], "not covering the results": [0, 1]}


def _batch():
    """result 0: handle 2, "ab", format 1 over one item "ab" of variable 1; result 1: handle 1, "cd", no format, one item "d" """
    results = [[2, 0, 1, 0, 0, 0, 2, 0, 1], [1, 1, 2, 0, 2, 0, 4, 1, 1]]
    items = [[1, 0, 1, 0, 0, 0, 2], [1, 1, 2, 0, 3, 0, 4]]
    return spa.MatchBatch(np.array(results, np.uint32), np.array(items, np.uint32), np.array([0, 2], np.uint64), np.zeros((1, 4), np.uint64),
                          np.zeros(1, np.int32), np.array([1, 0], np.uint32), np.zeros((2, 2), np.uint32))


@functools.lru_cache(maxsize=None)
def _matcher():
    return matcher_of(["<{a}>"])


# what the terms and the dictionary are built from, written out by hand: the value of result 0, the text of both, their terms
VALUES = spa.MatchValues(b"<ab>", np.array([0, 4, 4], np.uint64), None, None, np.zeros(1, np.int32))
RESULT_TEXT = spa.MatchText(b"abcd", np.array([0, 2, 4], np.uint64), None, None, np.zeros(1, np.int32))
TERM_RECORDS = [[1, 1, 1, 2, 1, 2], [2, 1, 0, 1, 0, 4]]     # (1, "cd") of result 1, (2, "<ab>") of result 0
TERMS = spa.MatchTerms(np.array(TERM_RECORDS, np.uint32), np.array([0, 2], np.uint64), np.array([1, 0], np.uint32), np.zeros(1, np.int32), V | T, BOUND)


def _text(got):
    assert got.result_text == b"abcd" and got.result_offsets.tolist() == [0, 2, 4]
    assert got.item_text == b"abd" and got.item_offsets.tolist() == [0, 2, 3] and got.status.tolist() == [0]


def _values(got):
    assert got.result_values == b"<ab>" and got.result_offsets.tolist() == [0, 4, 4]
    assert got.item_values == b"" and got.item_offsets.tolist() == [0, 0, 0] and got.status.tolist() == [0]


def _pattern_freq(got):
    assert got.records.tolist() == [[1, 1, 1, 2], [2, 1, 0, 1]] and got.doc_offsets.tolist() == [0, 2] and got.status.tolist() == [0]
    assert got.handle_results.tolist() == [0, 1, 1] and got.handle_docs.tolist() == [0, 1, 1]


def _terms(got):
    assert got.records.tolist() == TERM_RECORDS and got.doc_offsets.tolist() == [0, 2]
    assert got.result_term.tolist() == [1, 0] and got.status.tolist() == [0] and got.flags == V | T and got.handle_bound == BOUND


def _dictionary(got):
    assert got.records[:, :6].tolist() == [[1, 2, 0, 0, 1, 1], [2, 4, 0, 1, 1, 1]] and got.counts.tolist() == [1, 1]
    assert got.term_dict.tolist() == [0, 1] and got.doc_offsets.tolist() == [0, 2] and got.handle_terms.tolist() == [0, 1, 1]


# product -> (the call on a batch, the check of its answer for the well-formed batch)
PRODUCTS = {
    "batchText": (lambda mb: spa.batchText(mb, TEXT, SEGMENTS), _text),
    "batchValues": (lambda mb: spa.batchValues(_matcher(), mb, TEXT, SEGMENTS), _values),
    "batchPatternFreq": (lambda mb: spa.batchPatternFreq(mb, BOUND), _pattern_freq),
    "batchTerms": (lambda mb: spa.batchTerms(mb, values=VALUES, text=RESULT_TEXT, handle_bound=BOUND, flags=V | T), _terms),
    "batchDictionary": (lambda mb: spa.batchDictionary(mb, TERMS, values=VALUES, text=RESULT_TEXT), _dictionary),
}


@pytest.mark.parametrize("offsets", sorted(BAD_OFFSETS))
@pytest.mark.parametrize("product", sorted(PRODUCTS))
def test_malformed_document_offsets_are_refused_and_the_same_objects_serve_a_good_call(product, offsets):
    call, check = PRODUCTS[product]
    mb = _batch()
    mb.doc_offsets = np.array(BAD_OFFSETS[offsets], np.uint64)
    with pytest.raises(spa.PatternError, match=r"\(-1\)"):
        call(mb)
    mb.doc_offsets = np.array([0, 2], np.uint64)
    check(call(mb))
