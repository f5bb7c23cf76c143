"""Contextual biasing on the CPU: the matcher tables and the
host transition (csrc/bias.cpp through mwx_test_bias_match: no context, no
device work) against the naive restatement of the rule in tests/bias_ref.py,
which is itself pinned by cases worked by hand."""
import numpy as np
import pytest

import bias_ref
import mwx


def test_hand_cases_pin_the_restatement():
    for name, phrases, hist, want in bias_ref.hand_cases():
        got = bias_ref.bias_set(phrases, hist)
        assert got == {t: np.float32(b) for t, b in want.items()}, name


def test_matcher_equals_the_naive_rule():
    n = 0
    for name, phrases, hist, want in bias_ref.cases():
        rc, got, nbytes = mwx.bias_match(phrases, hist)
        assert rc == len(want), (name, rc, want)
        assert got == want, (name, phrases, hist, got, want)
        total = sum(len(ids) for ids, _ in phrases)
        assert 0 < nbytes <= bias_ref.table_bound(total), (name, nbytes, total)
        n += 1
    assert n >= 300


def test_every_prefix_of_a_history():
    """The state is carried id by id: every prefix of one long history."""
    rng = np.random.default_rng(7)
    phrases, _ = bias_ref.random_case(rng, alphabet=3, max_phrases=30, max_len=16)
    hist = [int(t) for t in rng.integers(0, 3, 64)]
    for n in range(len(hist) + 1):
        rc, got, _ = mwx.bias_match(phrases, hist[:n])
        assert rc >= 0 and got == bias_ref.bias_set(phrases, hist[:n]), n


@pytest.mark.parametrize("shared_prefix", [False, True])
def test_worst_case_table_size(shared_prefix):
    """1024 phrases x 16 tokens: the tables stay inside the bound DESIGN.md D14
    states (32 + 20 bytes per phrase token), which does not grow with
    states x root fan-out."""
    phrases = bias_ref.worst_case()
    if shared_prefix:  # one shared 8-id run after the distinct first ids
        phrases = [([1000 + p] + [9] * 8 + [p % 7, p % 11, p % 13, p % 3, 5, 6, p % 2], b)
                   for p, (_, b) in enumerate(phrases)]
    assert len(phrases) == bias_ref.MAX_PHRASES
    assert all(len(ids) == bias_ref.MAX_TOKENS for ids, _ in phrases)
    total = bias_ref.MAX_PHRASES * bias_ref.MAX_TOKENS
    hist = phrases[5][0][:15]
    rc, got, nbytes = mwx.bias_match(phrases, hist, cap=2048)
    assert rc >= bias_ref.MAX_PHRASES  # every first token, at least
    assert got == bias_ref.bias_set(phrases, hist)
    assert 0 < nbytes <= bias_ref.table_bound(total) == 32 + 20 * 16384
    assert nbytes < 1024 * 1024 * 4  # far from states x fan-out (16385 x 1024 x 4)


def test_refused_inputs():
    ok = [([1, 2], 1.0)]
    assert mwx.bias_match(ok, [1])[0] == 2
    assert mwx.bias_match([([1] * 17, 1.0)], [])[0] == -1
    assert mwx.bias_match([([], 1.0)], [])[0] == -1
    assert mwx.bias_match([([1], float("nan"))], [])[0] == -1
    assert mwx.bias_match([([1], float("inf"))], [])[0] == -1
    assert mwx.bias_match([([1], float("-inf"))], [])[0] == -1
    assert mwx.bias_match([([1, -4], 1.0)], [])[0] == -3
    assert mwx.bias_match([([p], 1.0) for p in range(bias_ref.MAX_PHRASES + 1)], [])[0] == -1
    assert mwx.bias_match([([p], 1.0) for p in range(bias_ref.MAX_PHRASES)], [], cap=0)[0] == 1024


def test_params_layout_and_defaults():
    """FullParams mirrors mwx_full_params to its last field (a wrong layout
    breaks every call): the library's defaults come back with the new fields
    zero and the fields before them intact."""
    p = mwx.Context.default_params(mwx.SAMPLING_BEAM_SEARCH)
    assert not p.bias_phrases and p.n_bias_phrases == 0
    assert p.chunk_language == mwx.CHUNK_LANG_PER_CHUNK and p.beam_search.beam_size == 5
    q = mwx.with_bias(p, [([3, 4, 5], 2.5), ([7], -1.0)])
    assert q.n_bias_phrases == 2 and p.n_bias_phrases == 0
    assert [q.bias_phrases[0].tokens[i] for i in range(3)] == [3, 4, 5]
    assert q.bias_phrases[1].n_tokens == 1 and q.bias_phrases[1].boost == -1.0
    assert q.beam_search.beam_size == 5 and q.language == p.language
