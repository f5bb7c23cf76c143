"""DTW token timestamps on the GPU (k_dtw.hip, the engine's alignment pass)
against tests/dtw_ref.py: the path kernel exactly, the cost and probability
kernels within their derived bounds, and mwx_full_batch end to end on the
micro geometry (the `micro-rich` weights: timestamps, segments, two windows)."""
import numpy as np
import pytest

import dtw_ref as R
import mwx
import vad_restatement as vr
import vad_segments_restatement as sr

pytestmark = pytest.mark.gpu

HEADS = [(0, 1), (1, 0), (1, 1)]


@pytest.fixture(scope="module")
def ctx(make_model):
    with mwx.Context.open(make_model("micro")) as c:
        yield c


# ---- 1. path: exact --------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int", "f32"])
@pytest.mark.parametrize("group", R.path_shapes(), ids=lambda g: "_".join(f"{n}x{t}" for n, t in g))
def test_path_equals_reference(ctx, kind, group):
    costs = [R.path_cost(kind, 17, n, t) for n, t in group]
    got = ctx.test_dtw_path(costs)                      # one launch, B = 3
    for (n, t), c, (frames, path) in zip(group, costs, got):
        ti, tj = R.dtw(c, np.float32)
        assert path.shape == (len(ti), 2), (n, t, path.shape, len(ti))
        assert np.array_equal(path[:, 0], ti) and np.array_equal(path[:, 1], tj), (n, t)
        assert np.array_equal(frames, R.frames_of_path(ti, tj, n)), (n, t)


def test_every_path_shape_is_covered():
    seen = {s for g in R.path_shapes() for s in g}
    assert seen == {(n, t) for n in R.PATH_NS for t in R.PATH_TS}
    assert all(len(set(g)) == 3 for g in R.path_shapes())


# ---- 2. cost: bounded ------------------------------------------------------------------
COST_CASES = {
    "A1_small": (1, "random", [(2, 1), (3, 3), (63, 4)], 64),
    "A3_edges": (3, "random", [(64, 7), (65, 749), (226, 1500)], 1500),
    "A3_planted": (3, "planted", [(24, 300), (2, 3), (226, 749)], 1500),
    "A1_planted": (1, "planted", [(3, 1), (64, 4), (63, 7)], 300),
}


@pytest.mark.parametrize("name", list(COST_CASES))
def test_cost_within_bound(ctx, name):
    A, kind, shapes, n_keys = COST_CASES[name]
    ncap = max(n for n, _ in shapes)
    w = np.full((len(shapes), A, ncap, n_keys), np.nan, np.float32)   # (unused rows: NaN)
    for b, (n, t) in enumerate(shapes):
        if kind == "random":
            w[b, :, :n] = R.random_probs(31 + b, A, n, n_keys)
        else:
            w[b, :, :n] = R.planted_probs(31 + b, A, n, t, n_keys)[0]
        if t > 2:
            w[b, :, :n, t // 2] = np.float32(2.0 ** -10)              # a constant column: var == 0
    got = ctx.test_dtw_cost(w, [n for n, _ in shapes], [t for _, t in shapes])
    for b, (n, t) in enumerate(shapes):
        wb = w[b, :, :n, :t]
        ref, bound = R.cost_bound(wb)
        err = np.abs(got[b].astype(np.float64) - ref)
        print(f"{name} N={n} T={t}: worst err/bound {np.max(err / bound):.3f}, "
              f"max bound {bound.max():.3g}")
        assert got[b].shape == (n, t) and np.all(np.isfinite(got[b]))
        assert np.all(err <= bound), (n, t, float(np.max(err / bound)))
        if A == 1:
            # the median selects one of its inputs: the cost is (minus) an element of
            # the window of the f32 restatement's z (T <= 3: z itself)
            z32 = R.normalise(wb, np.float32)[0][0]
            win = z32[:, R.reflect_index(t)] if t > 3 else z32[:, :, None]
            assert np.all((win == -got[b][:, :, None]).any(axis=-1)), (n, t)


# ---- 3. probabilities: bounded ---------------------------------------------------------
def _slabs(rng, target, KS):
    g = 0.5 * rng.standard_normal(target.shape + (KS,))
    w = (g - g.mean(axis=-1, keepdims=True) + 1.0 / KS).astype(np.float32)
    return np.ascontiguousarray(np.moveaxis(w * target[..., None], -1, 0), dtype=np.float32)


@pytest.mark.parametrize("cache", ["f16", "mx"])
@pytest.mark.parametrize("KS", [1, 5])
@pytest.mark.parametrize("rows", [1, 8, 9])
def test_align_probs_within_bound(ctx, cache, KS, rows):
    H, A, pos0, n_keys, slots = 2, 3, 3, (1500 if KS == 5 else 77), 3
    heads = [(1, 0), (0, 2)]                       # (head, a); a = 1 is never written
    rng = np.random.default_rng([41, KS, rows, cache == "mx"])
    padded = (rows + 7) // 8 * 8
    clip_slot = [2, 0]                             # two clips reading different slots
    kv, pos, act = [], [], []
    for s in clip_slot:
        for j in range(padded):
            kv.append(s)
            pos.append(pos0 + j if j < rows else 0)
            act.append(1 if j < rows else 0)
        kv += [s, s]                               # sot rows (pos < pos0): active, not aligned
        pos += [0, pos0 - 1]
        act += [1, 1]
    Rn = len(kv)
    qs = np.asarray([(0.05, 3.0, 0.7)[r % 3] for r in range(Rn)], np.float32)
    target = rng.standard_normal((Rn, H * 64)).astype(np.float32) * qs[:, None]
    P = _slabs(rng, target, KS)
    bias = (0.1 * rng.standard_normal(H * 64)).astype(np.float32)
    if cache == "mx":
        codes = rng.integers(0, 256, size=(slots, H, n_keys, 64)).astype(np.uint8)
        codes[(codes & 0x7F) == 0x7F] = 0x30       # no NaN codes
        e8 = rng.integers(115, 119, size=(slots, H, n_keys, 2)).astype(np.uint8)
        K = R.mx_widen(codes, e8)
        kwargs = dict(k=codes, kscale=e8)
    else:
        K = (rng.standard_normal((slots, H, n_keys, 64)) * 64.0 ** -0.25).astype(np.float16)
        kwargs = dict(k=K)
    scale = float(np.float32(64.0) ** np.float32(-0.25))
    out0 = np.full((slots, A, rows, n_keys), np.nan, np.float32)
    out = ctx.test_align_probs(P, bias, heads=heads, A=A, kv_index=kv, pos=pos, active=act,
                               out=out0, pos0=pos0, qscale=1.0, scale=scale, **kwargs)
    acc = P[0].copy()
    for ks in range(1, KS):
        acc = acc + P[ks]
    q = ((acc + bias) * np.float32(1.0)).astype(np.float16).reshape(Rn, H, 64)
    written = np.zeros(out.shape[:3], bool)
    worst = 0.0
    for r in range(Rn):
        n = pos[r] - pos0
        if not act[r] or n < 0:
            continue
        for h, a in heads:
            p, bound = R.probs_ref(q[r, h], K[kv[r], h], scale)
            err = np.abs(out[kv[r], a, n].astype(np.float64) - p)
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), (r, h, float(np.max(err / bound)))
            assert abs(float(out[kv[r], a, n].astype(np.float64).sum()) - 1.0) < 1e-5
            written[kv[r], a, n] = True
    print(f"{cache} KS={KS} rows={rows}: worst err/bound {worst:.3f}")
    assert written.sum() == 2 * rows * len(heads)
    assert np.all(np.isnan(out[~written]))          # padding rows, slot 1, a = 1: untouched


def test_align_probs_refuses_bad_indices(ctx):
    P = np.zeros((1, 8, 128), np.float32)
    K = np.zeros((1, 2, 16, 64), np.float16)
    ok = dict(heads=[(0, 0)], A=1, kv_index=[0] * 8, pos=list(range(8)), active=[1] * 8,
              out=np.zeros((1, 1, 8, 16), np.float32))
    ctx.test_align_probs(P, np.zeros(128, np.float32), K, **ok)
    for bad in (dict(heads=[(2, 0)]), dict(heads=[(0, 1)]), dict(kv_index=[0] * 7 + [1])):
        with pytest.raises(ValueError):
            ctx.test_align_probs(P, np.zeros(128, np.float32), K, **{**ok, **bad})


# ---- 4. context parameters -------------------------------------------------------------
def test_context_parameter_validation(make_model):
    path = make_model("micro")                      # 3 decoder layers x 2 heads

    def opens(**kw):
        try:
            mwx.Context(path, **kw).close()
            return True
        except RuntimeError:
            return False

    assert not lib_default().dtw_token_timestamps
    assert opens(dtw_preset=mwx.AHEADS_CUSTOM, dtw_heads=HEADS)
    assert opens(dtw_preset=mwx.AHEADS_N_TOP_MOST, dtw_n_top=1)
    assert opens(dtw_preset=mwx.AHEADS_N_TOP_MOST, dtw_n_top=3)
    assert opens(dtw_preset=mwx.AHEADS_CUSTOM, dtw_heads=[(2, 1)])
    assert not opens(dtw_preset=mwx.AHEADS_N_TOP_MOST, dtw_n_top=0)
    assert not opens(dtw_preset=mwx.AHEADS_N_TOP_MOST, dtw_n_top=4)
    assert not opens(dtw_preset=mwx.AHEADS_CUSTOM, dtw_heads=[])
    assert not opens(dtw_preset=mwx.AHEADS_CUSTOM, dtw_heads=[(3, 0)])
    assert not opens(dtw_preset=mwx.AHEADS_CUSTOM, dtw_heads=[(0, 2)])
    assert not opens(dtw_preset=mwx.AHEADS_CUSTOM, dtw_heads=[(-1, 0)])
    assert not opens(dtw_preset=mwx.AHEADS_BASE)    # a preset for 6 layers x 8 heads
    assert not opens(dtw_preset=99)


def lib_default():
    return mwx.lib().mwx_context_default_params()


# ---- 5. end to end ---------------------------------------------------------------------
def _params(ctx, mode):
    beam = mode == "beam5"
    p = ctx.default_params(mwx.SAMPLING_BEAM_SEARCH if beam else mwx.SAMPLING_GREEDY)
    p.language = b"en"
    p.token_timestamps = True
    p.suppress_nst = True
    p.no_speech_thold = 0.85
    p.logprob_thold = -0.7
    p.temperature_inc = 0.2 if beam else 0.0       # beam: the temperature fallback is live
    if beam:
        p.beam_search.beam_size = 5
        p.greedy.best_of = 5
    return p


def _records(ctx, state):
    return [(s.t0, s.t1, s.text, s.no_speech_prob,
             [(t.id, t.tid, t.p, t.plog, t.pt, t.ptsum, t.t0, t.t1) for t in s.tokens])
            for s in ctx.segments(state)]


def _dtw_times(ctx, state):
    return [[t.t_dtw for t in s.tokens] for s in ctx.segments(state)]


def _clips():
    return [mwx.pcm16_to_f32(mwx.synth_pcm16(0, 45 * 16000)),      # two windows
            mwx.pcm16_to_f32(mwx.synth_pcm16(1, 12 * 16000)),
            mwx.pcm16_to_f32(mwx.synth_pcm16(2, 16000 + 4000))]     # one short clip


def _check_state(ctx, state, eot, n_audio_ctx=1500):
    """The state's t_dtw against its own dumped passes; returns the number of
    text tokens checked."""
    passes = ctx.dtw_passes(state)
    text = [t for s in ctx.segments(state) for t in s.tokens if t.id < eot]
    others = [t for s in ctx.segments(state) for t in s.tokens if t.id >= eot]
    assert all(t.t_dtw == -1 for t in others)
    k = 0
    for ps in passes:
        N, T = ps["cost"].shape
        assert N >= 3 and 1 <= T <= n_audio_ctx and ps["probs"].shape[1:] == (N, n_audio_ctx)
        np.testing.assert_allclose(ps["probs"].astype(np.float64).sum(axis=-1), 1.0, atol=1e-5)
        want = R.token_times(ps["cost"], ps["seek"])
        got = np.array([t.t_dtw for t in text[k:k + N - 2]])
        assert np.array_equal(got, want), (state, ps["seek"])
        assert np.array_equal(ps["frames"], R.frames(ps["cost"]))
        assert np.all(got >= 0) and np.all(np.diff(got) >= 0)
        assert np.all(got >= ps["seek"]) and np.all(got <= ps["seek"] + 2 * T)
        k += N - 2
    assert k == len(text)
    return k


@pytest.fixture(scope="module")
def pair(make_model):
    path = make_model("micro-rich", mwx.GGML_F16)
    with mwx.Context.open(path) as off, \
            mwx.Context.open(path, dtw_preset=mwx.AHEADS_CUSTOM, dtw_heads=HEADS) as on:
        yield off, on


@pytest.mark.parametrize("mode", ["greedy", "beam5"])
def test_full_batch_with_dtw(pair, mode):
    off, on = pair
    clips = _clips()
    for i in range(len(clips) + 1):
        on.dtw_keep(True, i)
    assert off.full_batch(clips, _params(off, mode)) == 0
    assert on.full_batch(clips, _params(on, mode)) == 0
    eot = on.token("eot")
    n_text = 0
    for i in range(len(clips)):
        # everything but t_dtw is bit-identical with DTW off, where t_dtw is -1
        assert _records(on, i) == _records(off, i), (mode, i)
        assert all(t == -1 for seg in _dtw_times(off, i) for t in seg)
        n_text += _check_state(on, i, eot)
    assert n_text > 0
    assert len(on.dtw_passes(0)) >= 2, "the 45-s clip has two windows with segments"
    # batch equals single
    want = (_records(on, 0), _dtw_times(on, 0))
    assert on.full_batch_states([clips[0]], _params(on, mode), [3]) == 0
    assert (_records(on, 3), _dtw_times(on, 3)) == want


@pytest.mark.parametrize("kind", ["bf16", "mxfp8", "n_top_1"])
def test_other_contexts(make_model, kind):
    """bf16 weights, the MX-fp8 cross cache and the N_TOP_MOST head list: the
    same invariance and the same self-consistency, greedy, one clip."""
    bf = kind in ("bf16", "mxfp8")
    path = make_model("micro-rich", mwx.GGML_BF16 if bf else mwx.GGML_F16)
    compute = mwx.COMPUTE_MXFP8 if kind == "mxfp8" else mwx.COMPUTE_MODEL
    dtw = (dict(dtw_preset=mwx.AHEADS_N_TOP_MOST, dtw_n_top=1) if kind == "n_top_1"
           else dict(dtw_preset=mwx.AHEADS_CUSTOM, dtw_heads=HEADS))
    clip = _clips()[0]
    with mwx.Context.open(path, compute=compute) as off, \
            mwx.Context.open(path, compute=compute, **dtw) as on:
        on.dtw_keep(True)
        assert off.full(clip, _params(off, "greedy")) == 0
        assert on.full(clip, _params(on, "greedy")) == 0
        assert _records(on, 0) == _records(off, 0)
        assert _check_state(on, 0, on.token("eot")) > 0
        assert on.dtw_passes(0)[0]["probs"].shape[0] == (2 if kind == "n_top_1" else 3)


def test_trimmed_call_maps_t_dtw(pair, tmp_path):
    _, on = pair
    vpath = str(tmp_path / "ggml-silero-vad.bin")
    mwx.write_synthetic_vad_model(vpath, 3)
    prm = sr.Params(threshold=0.76)
    cp = mwx.vad_params(threshold=prm.threshold,
                        min_speech_duration_ms=prm.min_speech_duration_ms,
                        min_silence_duration_ms=prm.min_silence_duration_ms,
                        max_speech_duration_s=prm.max_speech_duration_s,
                        speech_pad_ms=prm.speech_pad_ms, samples_overlap=prm.samples_overlap)
    clip = vr.mixed_clip()
    p = _params(on, "greedy")
    with mwx.VadContext(vpath) as v, v.trim_batch([clip], cp) as t:
        assert on.full_batch_trimmed([t], [0], p) == 0
        got = _dtw_times(on, 0)
        pieces = sr.pieces(t.segments(0), prm)[0]
        compact = t.pcm(0)
    assert on.full_batch_states([compact], p, [1]) == 0
    plain = _dtw_times(on, 1)
    want = [[sr.map_time(pieces, x, False) if x >= 0 else -1 for x in seg] for seg in plain]
    assert got == want
    flat_p = [x for seg in plain for x in seg if x >= 0]
    flat_g = [x for seg in got for x in seg if x >= 0]
    assert len(flat_p) > 0 and flat_p != flat_g, "the map must move some time"


# ---- 6. golden: HF eager cross-attention ---------------------------------------------
def test_alignment_pass_matches_hf_golden(make_model):
    """The engine's alignment pass against HF transformers' fp32 eager
    cross-attention of the same seeded weights, tokens and clip
    (tests/golden/make_dtw_golden.py). The device's f16 pipeline is held to
    2e-2 on teacher-forced logits against the oracle (test_gpu_parity.py) and
    the oracle to 2e-3 against HF (test_oracle_golden.py): the cross-attention
    scores come out of the same pipeline, and a score error of d moves a
    softmax probability by at most p (e^(2 d) - 1) (its own score and the
    normaliser), d = 2.2e-2."""
    import os

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "dtw_golden.npz"))
    heads = [tuple(int(x) for x in h) for h in g["heads"]]
    assert heads == HEADS
    pcm = mwx.pcm16_to_f32(mwx.synth_pcm16(0))
    with mwx.Context.open(make_model("micro", mwx.GGML_F16), dtw_preset=mwx.AHEADS_CUSTOM,
                          dtw_heads=heads) as c:
        c.test_encode(pcm)
        ps = c.test_dtw_align(g["tokens"], int(g["pos0"]), 1500)
    got = ps["probs"][:, :, g["frames"]].astype(np.float64)
    want = g["probs"].astype(np.float64)
    assert got.shape == want.shape
    d = 2.2e-2
    bound = want * (np.exp(2 * d) - 1) + 1e-9
    err = np.abs(got - want)
    print(f"golden: worst |p - p_hf| {err.max():.3e} (p up to {want.max():.3e}), "
          f"worst err/bound {np.max(err / bound):.3f}, worst relative {np.max(err / want):.3e}")
    assert np.all(err <= bound), float(np.max(err / bound))
    assert np.array_equal(ps["frames"], R.frames(ps["cost"]))
