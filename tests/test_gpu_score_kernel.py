"""score_rows_kernel (k_score.hip) through mwx_test_score_rows against the
float64 reference of tests/score_ref.py, which states the contract, derives the
bound (summation depth D = 62) and builds the seeded inputs
(test_score_ref.py checks them on the CPU): vocabulary sizes 1 .. 51866 around
the wave (64), the old chunk width (256) and the workgroup's 1024 entries per
pass, logits at scale 1 and 20, a range of +-80, rows far from 0, -inf holes
(also at the target), bit-equal maxima across lanes, waves and a thread's run,
targets at 0, V - 1, the argmax and a tied maximum.

Exact: top_id, which rows are written, plog = -inf / p = 0 at a -inf target,
and a row's bits whether it is launched alone or among others. Bounded: plog,
top_plog, p.

Worst |err| / bound observed on MI355X over all cases: plog 0.44, top_plog
0.44, p 0.42 (test_worst_ratios prints them)."""
import numpy as np
import pytest

import mwx
import score_ref as sr

pytestmark = pytest.mark.gpu

WORST = {}
FIELDS = ("plog", "p", "top_id", "top_plog")


@pytest.fixture(scope="module")
def ctx(make_model):
    c = mwx.Context.open(make_model("micro"))
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def launch(ctx, x, target, active):
    return dict(zip(FIELDS, ctx.test_score_rows(x, target, active)))


def check(case, got, rows=None):
    refs = sr.references(case)
    for k in (range(case.R) if rows is None else rows):
        if refs[k] is None:
            assert np.isnan(got["plog"][k]) and np.isnan(got["p"][k]) and \
                np.isnan(got["top_plog"][k]) and got["top_id"][k] == -1, (case.name, k)
            continue
        ratios = {}
        bad = sr.compare(refs[k], {n: got[n][k] for n in FIELDS}, ratios)
        print(case.name, k, {n: round(v, 3) for n, v in ratios.items()})
        for n, v in ratios.items():
            WORST[n] = max(WORST.get(n, 0.0), v)
        assert not bad, (case.name, k, bad)


@pytest.mark.parametrize("name", [c.name for c in sr.cases() if c.name != "grid"])
def test_kernel_matches_reference(ctx, name):
    case = next(c for c in sr.cases() if c.name == name)
    got = launch(ctx, case.x, case.target, case.active)
    check(case, got)
    # every row alone, and the first two rows: the same bits
    for k in range(case.R):
        one = launch(ctx, case.x[k:k + 1], case.target[k:k + 1], case.active[k:k + 1])
        for n in FIELDS:
            assert bits(one[n])[0] == bits(got[n])[k], (name, k, n)
    two = launch(ctx, case.x[:2], case.target[:2], case.active[:2])
    for n in FIELDS:
        assert (bits(two[n]) == bits(got[n])[:2]).all(), (name, n)


def test_rows_across_the_grid_edge(ctx):
    """One workgroup per row: R = 255, 256, 257 around the chip's 256 compute
    units, active and inactive rows interleaved; every launch gives each row
    the bits it has alone."""
    case = next(c for c in sr.cases() if c.name == "grid")
    full = launch(ctx, case.x, case.target, case.active)
    check(case, full)
    for R in (1, 2, 255, 256):
        part = launch(ctx, case.x[:R], case.target[:R], case.active[:R])
        for n in FIELDS:
            assert (bits(part[n]) == bits(full[n])[:R]).all(), (R, n)
    for k in (0, 3, 254, 255, 256):
        one = launch(ctx, case.x[k:k + 1], case.target[k:k + 1], case.active[k:k + 1])
        for n in FIELDS:
            assert bits(one[n])[0] == bits(full[n])[k], (k, n)


def test_refusals_launch_nothing(ctx):
    x = np.zeros((2, 8), np.float32)
    ok = np.ones(2, np.int32)
    for tgt in ([0, 8], [-1, 0]):
        rc, *out = ctx.test_score_rows_rc(x, np.array(tgt, np.int32), ok)
        assert rc == -1
        assert np.isnan(out[0]).all() and (out[2] == -1).all()
    import ctypes as C
    fn = mwx.lib().mwx_test_score_rows
    z = np.zeros(4, np.float32)
    zi = np.zeros(4, np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    a = (ctx.ctx, mwx.fptr(z), zi.ctypes.data_as(ip), zi.ctypes.data_as(ip), mwx.fptr(z),
         mwx.fptr(z), zi.ctypes.data_as(ip), mwx.fptr(z))
    assert fn(a[0], 0, 4, *a[1:]) == -1
    assert fn(a[0], 1, 0, *a[1:]) == -1
    assert fn(a[0], 1, sr.MAX_VOCAB + 1, *a[1:]) == -1


def test_worst_ratios():
    """Prints the largest kernel error / bound per quantity over the cases run
    before it in this session, for the module docstring's figures. It checks
    nothing of its own: check() asserts every ratio row by row."""
    print("score_rows worst |err| / bound:", {n: round(v, 3) for n, v in sorted(WORST.items())})
