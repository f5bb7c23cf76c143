"""tests/score_ref.py on the CPU: the f32 emulations of score_rows_kernel (its
own summation order and pairwise) stay inside the derived bound on every seeded
input, named mutants do not (so the bound is not fitted), and the inputs meet
the margin condition the exact fields need."""
import numpy as np
import pytest

import score_ref as sr

CASES = [c.name for c in sr.cases()]


def _case(name):
    return next(c for c in sr.cases() if c.name == name)


def _active_rows(case):
    refs = sr.references(case)
    # (the 257-row grid case: every 16th row is enough for the emulation)
    step = 16 if case.name == "grid" else 1
    return [(k, refs[k]) for k in range(0, case.R, step) if refs[k] is not None]


def test_depth_is_the_kernels():
    assert sr.KERNEL_DEPTH == 62 and sr.MAX_VOCAB == 53248
    assert sr.SC_NPT * sr.SC_T >= max(sr.VOCAB_SIZES)


@pytest.mark.parametrize("name", CASES)
def test_inputs_meet_the_margin_condition(name):
    case = _case(name)
    for k, r in _active_rows(case):
        sr.margins(r)
        x = case.x[k]
        assert np.isfinite(x).any() and not np.isnan(x).any()


@pytest.mark.parametrize("order", ["kernel", "pairwise"])
@pytest.mark.parametrize("name", CASES)
def test_emulation_inside_the_bound(name, order):
    case = _case(name)
    worst = {}
    for k, r in _active_rows(case):
        for ulp in (0, 2, -2):  # expf / logf off by up to 2.5 ulp one way: inside E
            got = sr.emulate(case.x[k], int(case.target[k]), order=order, ulp=ulp)
            bad = sr.compare(r, got, worst)
            assert not bad, (name, k, order, ulp, bad)
    print(name, order, {n: round(v, 3) for n, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values())


def test_hole_at_the_target_is_exact():
    seen = 0
    for case in sr.cases():
        for k, r in _active_rows(case):
            if case.x[k][case.target[k]] == -np.inf:
                got = sr.emulate(case.x[k], int(case.target[k]))
                assert got["plog"] == -np.inf and got["p"] == 0.0
                assert r["plog"] == -np.inf and r["p"] == 0.0
                seen += 1
    assert seen >= 10


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_mutants_are_caught(mutant):
    """no_max: exp(x) without the maximum subtracted overflows or loses the
    small terms at scale 20 / range 80; tie_high: the highest index of a
    bit-equal maximum; target_twice: the target's term summed twice."""
    caught = 0
    for case in sr.cases():
        if case.name == "grid":
            continue
        for k, r in _active_rows(case):
            got = sr.emulate(case.x[k], int(case.target[k]), mutant=mutant)
            caught += bool(sr.compare(r, got))
    assert caught >= 8, (mutant, caught)


def test_tie_mutant_flips_only_the_exact_field():
    case = _case("ties2049")
    refs = sr.references(case)
    for k in range(case.R):
        got = sr.emulate(case.x[k], int(case.target[k]), mutant="tie_high")
        bad = sr.compare(refs[k], got)
        assert [b[0] for b in bad] == ["top_id"], bad
