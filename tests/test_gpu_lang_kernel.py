"""lang_probs_kernel (k_lang.hip) through mwx_test_lang_probs against the
float64 reference of tests/lang_ref.py, which states the contract, derives the
bound (summation depth ceil(n / 64) - 1 + 6) and builds the seeded inputs
(test_lang_ref.py checks them on the CPU): n in {1, 2, 63, 64, 65, 99, 100,
127, 128}, V in {n, 51865, 51866} with the window at 0, at the model's first
language token and at V - n, logits at scale 1 and 20, a range of +-80, rows far
from 0, -inf holes (also every entry but one), bit-equal maxima in one lane's
two entries, across lanes and at indices 0 and n - 1, large values next to the
window, and logits one f32 step apart.

Exact: best, zeros at -inf entries, and a row's bits whether it is launched
alone, as one of the first two rows or in the full launch. Bounded: probs.

Worst |err| / bound observed on MI355X over all cases: probs 0.79
(test_worst_ratios prints it)."""
import ctypes as C

import numpy as np
import pytest

import lang_ref as lr
import mwx

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def ctx(make_model):
    c = mwx.Context.open(make_model("micro"))
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(case, probs, best, rows=None):
    refs = lr.references(case)
    for k in (range(case.R) if rows is None else rows):
        ratios = {}
        bad = lr.compare(refs[k], dict(p=probs[k], best=best[k]), ratios)
        for n, v in ratios.items():
            WORST[n] = max(WORST.get(n, 0.0), v)
        assert not bad, (case.name, k, bad)
        hole = case.win[k] == -np.inf
        assert (bits(probs[k])[hole] == 0).all(), (case.name, k)  # +0.0 exactly


@pytest.mark.parametrize("name", [c.name for c in lr.cases() if c.name != "grid"])
def test_kernel_matches_reference(ctx, name):
    case = lr.case(name)
    x = case.x()
    probs, best = ctx.test_lang_probs(x, case.t0, case.n)
    assert probs.shape == (case.R, case.n) and best.shape == (case.R,)
    check(case, probs, best)
    print(name, {n: round(v, 3) for n, v in WORST.items()})
    # every row alone, and the first two rows: the same bits
    for k in range(case.R):
        p1, b1 = ctx.test_lang_probs(x[k:k + 1], case.t0, case.n)
        assert (bits(p1)[0] == bits(probs)[k]).all() and b1[0] == best[k], (name, k)
    p2, b2 = ctx.test_lang_probs(x[:2], case.t0, case.n)
    assert (bits(p2) == bits(probs)[:2]).all() and (b2 == best[:2]).all(), name


def test_rows_across_the_workgroup_and_grid_edges(ctx):
    """Four rows per workgroup: R = 3, 4, 5 around one workgroup, R = 1023,
    1024, 1025 around the chip's 256 compute units. The 1025-row launch runs
    once; every prefix and sampled single row has the bits it has there."""
    case = lr.case("grid")
    x = case.x()
    assert case.R == 1025
    probs, best = ctx.test_lang_probs(x, case.t0, case.n)
    check(case, probs, best)
    for R in lr.GRID_PREFIXES:
        p, b = ctx.test_lang_probs(x[:R], case.t0, case.n)
        assert (bits(p) == bits(probs)[:R]).all() and (b == best[:R]).all(), R
    for k in (0, 3, 4, 5, 1022, 1023, 1024):
        p, b = ctx.test_lang_probs(x[k:k + 1], case.t0, case.n)
        assert (bits(p)[0] == bits(probs)[k]).all() and b[0] == best[k], k


def test_refusals_launch_nothing(ctx):
    x = np.zeros((2, 200), np.float32)
    for kw in (dict(t0=0, n=0), dict(t0=0, n=129), dict(t0=-1, n=100), dict(t0=101, n=100),
               dict(t0=0, n=100, R=0), dict(t0=0, n=100, R=-3), dict(t0=150, n=100, V=249)):
        rc, probs, best = ctx.test_lang_probs_rc(x, **kw)
        assert rc == -1, kw
        assert np.isnan(probs).all() and (best == -1).all(), kw  # untouched
    # the edge that is allowed: the window ends at V
    rc, probs, best = ctx.test_lang_probs_rc(x, t0=100, n=100)
    assert rc == 0 and not np.isnan(probs).any() and (best == 0).all()
    assert (probs == np.float32(0.01)).all()
    fn = mwx.lib().mwx_test_lang_probs
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    z = np.zeros(8, np.float32)
    zi = np.zeros(8, np.int32)
    assert fn(None, 1, 8, mwx.fptr(z), 0, 8, mwx.fptr(z), zi.ctypes.data_as(ip)) == -1
    assert fn(ctx.ctx, 1, 8, None, 0, 8, mwx.fptr(z), zi.ctypes.data_as(ip)) == -1
    assert fn(ctx.ctx, 1, 8, mwx.fptr(z), 0, 8, None, zi.ctypes.data_as(ip)) == -1
    assert fn(ctx.ctx, 1, 8, mwx.fptr(z), 0, 8, mwx.fptr(z), None) == -1


def test_worst_ratios():
    """Prints the largest kernel error / bound over the cases run before it in
    this session, for the module docstring's figure. It checks nothing of its
    own: check() asserts every ratio row by row."""
    print("lang_probs worst |err| / bound:", {n: round(v, 3) for n, v in sorted(WORST.items())})
