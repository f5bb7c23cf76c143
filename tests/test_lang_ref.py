"""tests/lang_ref.py on the CPU: the f32 emulations of lang_probs_kernel (its
own summation order and pairwise) stay inside the derived bound on every seeded
input, named mutants do not (so the bound is not fitted), and the inputs meet
the margin condition."""
import numpy as np
import pytest

import lang_ref as lr

CASES = [c.name for c in lr.cases()]


def _rows(c):
    # (the 1025-row grid case: every 64th row is enough for the emulation)
    return range(0, c.R, 64 if c.name == "grid" else 1)


def test_depth_and_shapes_are_the_kernels():
    assert lr.MAX_N == 128 and lr.depth(1) == 6 and lr.depth(64) == 6
    assert lr.depth(65) == 7 and lr.depth(128) == 7
    assert lr.N_LANG == 100 and lr.T0_MODEL + lr.MAX_N <= 51865
    want = {(n, V) for n in lr.N_SIZES for V in (n, 51865, 51866)}
    have = {(c.n, c.V) for c in lr.cases() if c.name not in ("grid", "near")}
    assert have == want
    for c in lr.cases():
        assert 0 <= c.t0 and c.t0 + c.n <= c.V and 1 <= c.n <= lr.MAX_N
    t0s = {(c.V > c.n, c.t0 == 0, c.t0 == lr.T0_MODEL, c.t0 == c.V - c.n) for c in lr.cases()}
    assert {(True, True, False, False), (True, False, True, False),
            (True, False, False, True)} <= t0s


@pytest.mark.parametrize("name", CASES)
def test_inputs_meet_the_margin_condition(name):
    c = lr.case(name)
    refs = lr.references(c)
    for k in range(c.R):
        w = c.win[k]
        assert np.isfinite(w).any() and not np.isnan(w).any()
        if name == "near":
            assert 0 < refs[k]["gap"] < refs[k]["need"]  # (exempt: one f32 step apart)
        else:
            lr.margins(refs[k])
        assert abs(refs[k]["p"].sum() - 1.0) < 1e-12


def test_full_rows_hold_the_windows_and_the_leak_values():
    seen = 0
    for name in ("n100_v51866_t50259", "n128_v51865_t0", "n1_v51866_t51865", "grid"):
        c = lr.case(name)
        x = c.x()
        assert x.shape == (c.R, c.V) and x.dtype == np.float32
        assert (x[:, c.t0:c.t0 + c.n].view(np.uint32) == c.win.view(np.uint32)).all()
        for k in c.leak:
            hi = c.win[k][np.isfinite(c.win[k])].max()
            if c.t0 > 0:
                assert x[k, c.t0 - 1] > hi + 40
                seen += 1
            if c.t0 + c.n < c.V:
                assert x[k, c.t0 + c.n] > hi + 40
                seen += 1
    assert seen >= 6


@pytest.mark.parametrize("order", ["kernel", "pairwise"])
@pytest.mark.parametrize("name", CASES)
def test_emulation_inside_the_bound(name, order):
    c = lr.case(name)
    refs = lr.references(c)
    x = c.x()
    worst = {}
    for k in _rows(c):
        for ulp in (0, 2, -2):  # expf off by up to 2.5 ulp one way: inside E
            got = lr.emulate(x[k], c.t0, c.n, order=order, ulp=ulp)
            bad = lr.compare(refs[k], got, worst)
            assert not bad, (name, k, order, ulp, bad)
    print(name, order, {n: round(v, 3) for n, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values())


def test_holes_are_exact_zeros():
    seen = 0
    for c in lr.cases():
        if c.name == "grid":
            continue
        refs = lr.references(c)
        x = c.x()
        for k in range(c.R):
            hole = c.win[k] == -np.inf
            if hole.any():
                got = lr.emulate(x[k], c.t0, c.n)
                assert (got["p"][hole] == 0.0).all() and (refs[k]["p"][hole] == 0.0).all()
                assert (refs[k]["b_p"][hole] == 0.0).all()
                seen += 1
    assert seen >= 100


@pytest.mark.parametrize("mutant", lr.MUTANTS)
def test_mutants_are_caught(mutant):
    """no_max: exp(x) without the maximum subtracted overflows or loses the
    small terms at scale 20 / range 80 / offset 100; t0 / n off by one: another
    window (the leak rows put large values next to it); tie_high: the highest
    index of a bit-equal maximum; best_from_probs: the argmax of the rounded
    probabilities, wrong where two logits one step apart round to one
    probability (the "near" rows)."""
    caught = 0
    for c in lr.cases():
        if c.name == "grid":
            continue
        refs = lr.references(c)
        x = c.x()
        for k in range(c.R):
            got = lr.emulate(x[k], c.t0, c.n, mutant=mutant)
            if got is not None:
                caught += bool(lr.compare(refs[k], got))
    assert caught >= (3 if mutant == "best_from_probs" else 8), (mutant, caught)


def test_tie_and_probability_mutants_flip_only_best():
    c = lr.case("near")
    refs = lr.references(c)
    x = c.x()
    for k in range(c.R):
        assert not lr.compare(refs[k], lr.emulate(x[k], c.t0, c.n))
        bad = lr.compare(refs[k], lr.emulate(x[k], c.t0, c.n, mutant="best_from_probs"))
        assert [b[0] for b in bad] == ["best"], bad
    c = lr.case("n128_v51866_t50259")
    refs = lr.references(c)
    x = c.x()
    ties = [k for k in range(c.R) if (c.win[k] == c.win[k].max()).sum() == 2]
    assert len(ties) == len(lr.tie_pairs(128)) == 5
    for k in ties:
        bad = lr.compare(refs[k], lr.emulate(x[k], c.t0, c.n, mutant="tie_high"))
        assert [b[0] for b in bad] == ["best"], bad
