"""lp_filter_kernel, lp_probs_kernel and lp_pick_row (k_misc.hip) through
mwx_test_logits_process against the float64 reference of tests/logits_ref.py,
which states the stage contract, derives the bounds and builds the seeded
inputs (test_logits_ref.py checks them on the CPU): every vocabulary size at a
chunk edge, beg / eot placements, every rule state, masked chunks, magnitudes,
timestamp-mass ties and argmax ties across lanes, waves, slots and chunks.

Exact: which rows are written, the -inf sets of flt and logprobs (so the
kill_text decision), the surviving flt values, id and tid. Bounded: logprobs,
probs, p, plog, pt, ptsum, nosp.

Worst |err| / bound observed on MI355X over all cases: logprobs 0.70, probs
0.52, p 0.24, plog 0.25, pt 0.03, ptsum 0.25, nosp 0.35 (test_worst_ratios
prints them)."""
import numpy as np
import pytest

import logits_ref as lr
import mwx
import orc

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def ctx(make_model):
    c = mwx.Context.open(make_model("micro"))
    yield c
    c.close()


def lc_struct(lc):
    return mwx.TestLogitsConst(lc.n_vocab, lc.eot, lc.beg, lc.space_id, lc.suppress_blank,
                               lc.max_initial_tid, lc.nosp_id)


def rows_of(flt, probs, lps, out):
    """The hook's outputs as compare() takes them: None for a row left as
    sentinels in every output, probs / logprobs None where they are."""
    got = []
    for k in range(flt.shape[0]):
        rec_untouched = bool((out[k:k + 1].view(np.uint32) == 0xFFFFFFFF).all())
        if rec_untouched and all(np.isnan(a[k]).all() for a in (flt, probs, lps)):
            got.append(None)
            continue
        no_probs = np.isnan(probs[k]).all() and np.isnan(lps[k]).all()
        got.append((flt[k], None if no_probs else probs[k], None if no_probs else lps[k],
                    {n: out[k][n] for n in lr.REC}))
    return got


def run_case(ctx, case, refs=None):
    flt, probs, lps, out = ctx.test_logits_process(case.x, case.smask, case.ctl,
                                                   lc_struct(case.lc))
    refs = lr.references(case) if refs is None else refs
    for k, got in enumerate(rows_of(flt, probs, lps, out)):
        ratios = {}
        bad = lr.compare(refs[k], got, ratios)
        print(case.name, k, {n: round(v, 3) for n, v in ratios.items()})
        for n, v in ratios.items():
            WORST[n] = max(WORST.get(n, 0.0), v)
        assert not bad, (case.name, k, bad)


@pytest.mark.parametrize("name", [c.name for c in lr.cases()])
def test_kernel_matches_reference(ctx, name):
    case = next(c for c in lr.cases() if c.name == name)
    lr.check_margins(case)
    run_case(ctx, case)


def test_all_cases_in_one_launch_shape(ctx):
    """R = 64 rows of one launch (written and unwritten rows interleaved)
    give what the rows give alone: the row index reaches every address."""
    case = next(c for c in lr.cases() if c.name == "beg6656")
    n = -(-64 // case.R)
    x = np.tile(case.x, (n, 1))[:64]
    ctl = np.tile(case.ctl, n)[:64]
    big = lr.Case("beg6656x", case.lc, case.smask, x, ctl)
    refs = (lr.references(case) * n)[:64]
    run_case(ctx, big, refs)


def test_refused_arguments_launch_nothing(ctx):
    V = 300
    lc = lr.LC(V, 100, 200, 50, 1, -1, 101)
    x = np.zeros((2, V), np.float32)
    sm = np.zeros(V, np.float32)
    ctl = np.array([lr.ctl_row()] * 2, lr.CTL)

    def rc_of(x=x, sm=sm, ctl=ctl, **kw):
        rc, flt, probs, lps, out = ctx.test_logits_process_rc(
            x, sm, ctl, lc_struct(lr.LC(**{**lc.__dict__, **kw})))
        assert all(np.isnan(a).all() for a in (flt, probs, lps))
        assert (out.view(np.uint32) == 0xFFFFFFFF).all()
        return rc
    for kw in (dict(eot=-1), dict(eot=V), dict(beg=-1), dict(beg=V + 1), dict(space_id=-1),
               dict(space_id=V), dict(nosp_id=-1), dict(nosp_id=V), dict(n_vocab=V + 1),
               dict(n_vocab=V - 1)):
        assert rc_of(**kw) == -1, kw
    bad = ctl.copy()
    bad["seek_delta"][1] = -2
    assert rc_of(ctl=bad) == -1
    assert rc_of(x=np.zeros((0, V), np.float32), ctl=ctl[:0]) == -1
    assert rc_of(x=np.zeros((257, V), np.float32), ctl=np.array([lr.ctl_row()] * 257, lr.CTL)) == -1
    assert rc_of(x=np.zeros((1, 0), np.float32), sm=sm[:0], ctl=ctl[:1], n_vocab=0) == -1
    V2 = lr.MAX_VOCAB + 1
    rc, *_ = ctx.test_logits_process_rc(np.zeros((1, V2), np.float32), np.zeros(V2, np.float32),
                                        ctl[:1], lc_struct(lr.LC(V2, 100, 200, 50, 1, -1, 101)))
    assert rc == -4
    # beg = V (no timestamp at all) is inside the contract
    assert ctx.test_logits_process_rc(x, sm, ctl, lc_struct(lr.LC(V, 100, V, 50, 1, -1, 101)))[0] == 0


@pytest.mark.parametrize("arch", ["micro", "micro-v3"])
def test_engine_constants_and_mask(make_model, arch):
    """The engine's own LogitsConst and static mask (the functions the decode
    driver calls) against the rule, and rows through the kernel with them."""
    path = make_model(arch)
    o = orc.Oracle(path)
    sp, nst, space = lr.oracle_vocab(o)
    V, beg, eot = o.n_vocab, o.beg, o.eot
    rng = np.random.default_rng(8)
    variants = [dict(), dict(suppress_nst=True), dict(no_timestamps=True), dict(tdrz_enable=True),
                dict(bench_fixed_steps=4), dict(suppress_blank=False, max_initial_ts=0.0),
                dict(suppress_nst=True, max_initial_ts=2.0)]
    with mwx.Context.open(path) as c:
        for kw in variants:
            p = c.default_params(mwx.SAMPLING_GREEDY)
            for k, v in kw.items():
                setattr(p, k, v)
            lcs, sm = c.test_logits_setup(p)
            mi = kw.get("max_initial_ts", p.max_initial_ts)
            want = lr.LC(V, eot, beg, space, int(kw.get("suppress_blank", True)),
                         beg + int(round(mi / 0.02)) if mi > 0 else -1, o.nosp)
            got = lr.LC(*(getattr(lcs, f) for f, _ in lcs._fields_))
            assert got == want, kw
            ref_sm = lr.static_mask(V, sp, nst_ids=nst, suppress_nst=kw.get("suppress_nst", False),
                                    no_timestamps=kw.get("no_timestamps", False),
                                    tdrz=kw.get("tdrz_enable", False),
                                    bench_fixed_steps=kw.get("bench_fixed_steps", 0))
            np.testing.assert_array_equal(lr.bits(sm), lr.bits(ref_sm), err_msg=str(kw))
            no_ts = kw.get("no_timestamps") or kw.get("bench_fixed_steps")
            hists = [[], [17], [17, 900]] if no_ts else \
                [[], [17], [beg + 5], [beg + 5, 17, beg + 40], [beg + 5, 17, beg + 40, beg + 40]]
            rows = []
            for h in hists:
                x = rng.normal(0.0, 3.0, V).astype(np.float32)
                x[int(rng.integers(0, eot))] += 8.0
                x[beg:] += 3.0 * (len(h) % 2)
                rows.append((x, dict(lr.ctl_of_history(h, beg), want_nosp=int(not h),
                                     temperature=0.7 * (len(h) % 2))))
            case = lr._mk(f"{arch}{sorted(kw)}", got, sm, rows)
            lr.check_margins(case)
            run_case(c, case)


def test_worst_ratios():
    """Prints the largest kernel error / bound per quantity over the cases run
    before it in this session, for the module docstring's figures. It checks
    nothing of its own: run_case asserts every ratio row by row."""
    print("worst |err| / bound:", {n: round(v, 3) for n, v in sorted(WORST.items())})
