"""The one-language-per-recording rule (tests/lang_pool_restatement.py,
DESIGN.md D13) on its tables: which chunks are pooled (around 480 000 summed
samples and the 0.1-s rule), the length weights, the tie rule, and no chunks at
all."""
import numpy as np
import pytest

import lang_pool_restatement as lp


def test_the_short_chunk_rule_is_ten_mel_frames():
    assert not lp.counts(0) and not lp.counts(-5) and not lp.counts(199)
    assert not lp.counts(1639) and lp.counts(1640) and lp.counts(480000)


@pytest.mark.parametrize("lengths,want", lp.TABLE_CHUNKS)
def test_pooled_chunks(lengths, want):
    assert lp.pooled_chunks(lengths) == want


def test_the_pool_stops_at_480000_exactly():
    for first, n_pooled in ((479999, 2), (480000, 1), (480001, 1)):
        assert len(lp.pooled_chunks([first, 16000, 16000])) == n_pooled
    # split over two chunks: the sum counts, not a single chunk
    for second, n_pooled in ((239999, 3), (240000, 2), (240001, 2)):
        assert len(lp.pooled_chunks([240000, second, 16000, 16000])) == n_pooled


@pytest.mark.parametrize("lengths,probs,want_p,want_id", lp.TABLE_POOL)
def test_pool(lengths, probs, want_p, want_id):
    P, lang = lp.pool(lengths, probs)
    assert P.dtype == np.float32
    assert (P == np.array(want_p, np.float32)).all() and lang == want_id


def test_no_chunks():
    assert lp.pool([], []) == (None, -1)
    assert lp.recording_language([], lambda j: None) == (None, -1)
    assert lp.recording_language([100, 1639], lambda j: None) == (None, -1)


def test_accumulation_is_double_in_chunk_order():
    rng = np.random.default_rng(5)
    lens = [int(v) for v in rng.integers(1640, 480000, 7)]
    probs = rng.random((7, 100)).astype(np.float32)
    probs /= probs.sum(axis=1, keepdims=True)
    P, lang = lp.pool(lens, probs)
    acc = np.zeros(100)
    for n, p in zip(lens, probs):
        acc = acc + n * p.astype(np.float64)
    want = (acc / sum(lens)).astype(np.float32)
    assert (P.view(np.uint32) == want.view(np.uint32)).all()
    assert lang == int(np.argmax(want))
    assert abs(float(P.astype(np.float64).sum()) - 1.0) < 1e-5


def test_the_end_to_end_rule_reads_only_the_pooled_chunks():
    lengths = [1000, 300000, 200000, 16000]
    seen = []

    def probs_of(j):
        seen.append(j)
        return [[0, 0], [0.9, 0.1], [0.2, 0.8], [0, 1]][j]

    P, lang = lp.recording_language(lengths, probs_of)
    assert seen == [1, 2]
    assert lang == 0 and P[0] == np.float32((300000 * np.float64(np.float32(0.9)) +
                                            200000 * np.float64(np.float32(0.2))) / 500000)
