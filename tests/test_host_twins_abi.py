"""What the five device-free twins of the products of a finished batch share (csrc/finished_host.hpp): each of spa.batchText,
batchValues, batchPatternFreq, batchTerms and batchDictionary refuses the same three malformed batches -- document offsets that
do not start at 0, that descend, that do not cover the results -- with SP_ERR_INVALID, and the same objects then serve a
well-formed call whose answer is written out by hand.  One document, two results, a text of 4 bytes: the smallest shape that
can express all three conditions.  Needs no device."""
import functools

import numpy as np
import pytest

import struspattern_amd as spa
from tests.finished_support import (matcher_of, TWIN_BAD_OFFSETS as BAD_OFFSETS, _twin_batch as _batch, TWIN_BOUND as BOUND,
                                    TWIN_RESULT_TEXT as RESULT_TEXT, TWIN_TERM_RECORDS as TERM_RECORDS, TWIN_TERMS as TERMS, TWIN_VALUES as VALUES)

V, T = spa.SP_TERM_VALUES, spa.SP_TERM_TEXT
TEXT, SEGMENTS = b"abcd", [0, 4]


@functools.lru_cache(maxsize=None)
def _matcher():
    return matcher_of(["<{a}>"])


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
