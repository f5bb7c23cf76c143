"""Audio context on the GPU (mwx_full_params.audio_ctx / audio_ctx_fit,
DESIGN.md D9) against the CPU oracle run on the model rewritten to the short
context (tests/audio_ctx_ref.py), and against itself: a clip's result does not
depend on its batch mates.

The stage bounds are those tests/test_gpu_parity.py applies to the same stages
at full context: its test bodies are run here as they stand, with the device's
encode redirected to mwx_test_encode_ctx at K frames and the oracle to the
model rewritten to K frames. LOGITS_BOUND restates the one of them the margin
rule of the pipeline tests needs as a number (test_decoder_logits_parity's
2e-2 on f16 teacher-forced logits)."""
import numpy as np
import pytest

import mwx
import orc
import test_gpu_parity as TP
import vad_restatement as vr
from audio_ctx_ref import CtxOracles, audio_ctx_rule, rewrite_model
from test_gpu_dtw import HEADS, _check_state

pytestmark = pytest.mark.gpu

LOGITS_BOUND = 2e-2
N_CTX = 1500


def clip(k, seconds):
    return mwx.pcm16_to_f32(mwx.synth_pcm16(k, int(seconds * 16000)))


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("audio_ctx"))


@pytest.fixture(scope="module")
def micro(make_model, workdir):
    path = make_model("micro")
    with mwx.Context.open(path) as ctx:
        yield ctx, CtxOracles(path, workdir), path


@pytest.fixture(scope="module")
def rich(make_model, workdir):
    path = make_model("micro-rich")
    with mwx.Context.open(path) as ctx:
        yield ctx, CtxOracles(path, workdir), path


@pytest.fixture(scope="module")
def rich_mx(make_model):
    path = make_model("micro-rich", mwx.GGML_BF16)
    with mwx.Context.open(path, compute=mwx.COMPUTE_MXFP8) as ctx:
        yield ctx


def encode_at(monkeypatch, K, seek=0):
    """Context.test_encode -> mwx_test_encode_ctx at K frames (window at `seek`)."""
    monkeypatch.setattr(mwx.Context, "test_encode",
                        lambda self, pcm, **kw: self.test_encode_ctx(pcm, K, seek=seek))


class AtSeek:
    """An oracle whose encode() takes its window at `seek`."""

    def __init__(self, o, seek):
        self._o, self._seek = o, seek

    def __getattr__(self, name):
        return getattr(self._o, name)

    def encode(self, mel):
        return self._o.encode(mel, self._seek)


def oracle_at(monkeypatch, workdir, K):
    """orc.Oracle(path, ...) -> the oracle of the model rewritten to K frames."""
    real = orc.Oracle
    made = {}

    def make(path, **kw):
        if path not in made:
            made[path] = rewrite_model(path, f"{workdir}/mx-{len(made)}-ctx{K}.bin", K)
        return real(made[path], **kw)

    monkeypatch.setattr(orc, "Oracle", make)


def records(ctx, state=0):
    return [(s.t0, s.t1, s.text, s.no_speech_prob,
             [(t.id, t.tid, t.p, t.plog, t.pt, t.ptsum, t.t0, t.t1, t.t_dtw) for t in s.tokens])
            for s in ctx.segments(state)]


def run_fresh(ctx, pcm, p):
    """The records of a run on a state never used before (decoder 0's RNG
    lives in the state, and beam search draws from it)."""
    idx = len(ctx.states)
    assert ctx.full(pcm, p, state_index=idx) == 0
    return records(ctx, idx)


def params(ctx, beam=1, audio_ctx=0, fit=False):
    p = TP.service_params(ctx, beam=beam, temperature_inc=0.0, language=b"en")
    p.audio_ctx = audio_ctx
    p.audio_ctx_fit = fit
    return p


def options(beam=1):
    opt = orc.FullOptions.service_defaults(beam_size=beam)
    opt.temperature_inc = 0.0
    opt.language = "en"
    return opt


# ---- 1. stage parity ------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 96, 100, 200])
def test_stage_parity(micro, monkeypatch, K):
    """K = 64: one key tile, less than a query block; 96: a masked tail tile;
    100: K % 8 != 0 (padded V^T rows); 200: two query blocks and a tail."""
    ctx, refs, path = micro
    oK = refs.at(K)
    encode_at(monkeypatch, K)
    TP.test_encoder_and_cross_kv_parity((ctx, oK, path))
    TP.test_decoder_logits_parity((ctx, oK, path))
    # 16 teacher-forced tokens over the device's own cross K/V of K rows
    pcm = clip(4, 4.0)
    enc, k, v = ctx.test_encode_ctx(pcm, K)
    assert enc.shape == (K, ctx.d) and k.shape == v.shape == (ctx.n_text_layer, K, ctx.d)
    toks = [oK.sot, 300, 1234, oK.beg, 777, 40000, 220, oK.beg + 37,
            11, 2050, 31000, oK.beg + 40, oK.beg + 40, 907, 15, 4242]
    dev = ctx.test_decode(toks)
    ref = oK.decode_seq(k, v, toks)
    err = float(np.abs(dev - ref).max())
    print(f"K={K}: 16-token teacher-forced logits err {err:.4g}")
    assert err < LOGITS_BOUND, err


@pytest.mark.parametrize("K,seek", [(96, 137), (200, 1001), (64, 2950)])
def test_stage_parity_at_a_seek(micro, monkeypatch, K, seek):
    """A window that does not start at 0 or 3000 (the seek a timestamp leaves):
    the stem reads frames seek .. seek + 2 K of the 30-s clip, real frames past
    them count as zero, and at 2950 the clip's mel ends inside the window."""
    ctx, refs, path = micro
    encode_at(monkeypatch, K, seek)
    TP.test_encoder_and_cross_kv_parity((ctx, AtSeek(refs.at(K), seek), path))
    TP.test_decoder_logits_parity((ctx, AtSeek(refs.at(K), seek), path))


@pytest.mark.parametrize("K", [96, 100])
def test_stage_parity_mxfp8(make_model, workdir, monkeypatch, K):
    """MWX_COMPUTE_MXFP8 against the oracle's MX mode on the rewritten model,
    with the micro-scale MX bounds of test_gpu_parity.py (its test bodies)."""
    encode_at(monkeypatch, K)
    oracle_at(monkeypatch, workdir, K)
    TP.test_mxfp8_encoder_matches_mx_oracle(make_model)
    TP.test_mxfp8_decoder_logits_match_mx_oracle(make_model)


# ---- 2. K = n_audio_ctx is the default ------------------------------------------------
@pytest.mark.parametrize("beam", [1, 5])
def test_full_context_value_is_the_default(rich, beam):
    ctx, _, _ = rich
    pcm = clip(7, 33.0)
    want = run_fresh(ctx, pcm, params(ctx, beam))
    assert run_fresh(ctx, pcm, params(ctx, beam, audio_ctx=N_CTX)) == want and len(want) > 2


# ---- 3. whole pipeline ----------------------------------------------------------------
# (seconds, audio_ctx, fit) and, per beam size, (clip seed, bench_fixed_steps):
# picked on the CPU reference so that every traced decision's margin is at
# least 4 x LOGITS_BOUND. The 41-s clip runs under bench_fixed_steps (a fixed
# number of steps per window, then a whole-window seek: exactly two windows,
# 1500 and 640 frames); with the free-running token rules the micro-rich weights
# decode it in four windows of some hundred tokens each, whose reference
# (every row answered through the callbacks) takes minutes on the CPU and
# whose hundreds of beam decisions leave no seed with the required margin.
PIPELINE = {
    "short_ctx192": (2.5, 192, False, {1: (0, 0), 5: (0, 0)}),
    "two_windows_fit": (41.0, 0, True, {1: (0, 16), 5: (0, 6)}),
}
MARGIN_KINDS = ("argmax", "assign", "ts_mass", "best", "fallback", "no_speech")


def reference(refs, pcm, beam, audio_ctx, fit, steps):
    opt = options(beam)
    opt.bench_fixed_steps = steps
    (out, windows), trace = refs.base.traced(refs.full, pcm, opt, audio_ctx=audio_ctx, fit=fit)
    margins = [e.margin for e in trace if e.kind in MARGIN_KINDS]
    return out, windows, (min(margins) if margins else float("inf"))


@pytest.mark.parametrize("beam", [1, 5])
@pytest.mark.parametrize("case", list(PIPELINE))
def test_pipeline_matches_reference(rich, case, beam):
    ctx, refs, _ = rich
    seconds, audio_ctx, fit, picks = PIPELINE[case]
    seed, steps = picks[beam]
    pcm = clip(seed, seconds)
    (rc, osegs, _, _), windows, margin = reference(refs, pcm, beam, audio_ctx, fit, steps)
    print(f"{case} beam {beam}: windows {windows}, smallest reference margin {margin:.4f}")
    assert rc == 0 and margin >= 4 * LOGITS_BOUND, margin
    want_k = [audio_ctx_rule(N_CTX, len(pcm), s, audio_ctx, fit) for s, _ in windows]
    assert [k for _, k in windows] == want_k
    if fit:
        assert windows == [(0, N_CTX), (3000, 640)]
    p = params(ctx, beam, audio_ctx, fit)
    p.bench_fixed_steps = steps
    idx = len(ctx.states)
    assert ctx.full(pcm, p, state_index=idx) == 0
    segs = ctx.segments(idx)
    assert len(segs) > 0
    TP.assert_same(segs, osegs)


# ---- 4. batch invariance --------------------------------------------------------------
BATCH_SECONDS = (1.0, 3.2, 7.0, 30.0)


def check_batch_invariance(ctx, beam):
    """One call with fit on over four clips against each clip alone with fit
    on (the free-running token rules: the longer clips take several windows,
    each with its own context), and against each clip alone with audio_ctx =
    mwx_audio_ctx_for(...) under bench_fixed_steps, where every clip is one
    window, so that one value is the whole clip's context."""
    pcms = [clip(20 + i, s) for i, s in enumerate(BATCH_SECONDS)]
    n = len(pcms)
    ks = [ctx.audio_ctx_for(len(x), 0, 0, True) for x in pcms]
    assert ks == [audio_ctx_rule(N_CTX, len(x), 0, 0, True) for x in pcms] == [128, 192, 384, 1500]
    for steps in (0, 8):
        def prm(**kw):
            p = params(ctx, beam, **kw)
            p.bench_fixed_steps = steps
            return p
        base = len(ctx.states)
        assert ctx.full_batch_states(pcms, prm(fit=True), range(base, base + n)) == 0
        batched = [records(ctx, base + i) for i in range(n)]
        assert all(len(r) > 0 for r in batched[1:])
        for i, x in enumerate(pcms):
            assert run_fresh(ctx, x, prm(fit=True)) == batched[i], ("alone, fit on", steps, i)
            if steps:
                assert run_fresh(ctx, x, prm(audio_ctx=ks[i])) == batched[i], (
                    "alone, audio_ctx", i, ks[i])
        # the context shows in the result: a short clip does not decode as at 1500 frames
        assert run_fresh(ctx, pcms[1], prm()) != batched[1]


@pytest.mark.parametrize("beam", [1, 5])
def test_batch_invariance_f16(rich, beam):
    check_batch_invariance(rich[0], beam)


@pytest.mark.parametrize("beam", [1, 5])
def test_batch_invariance_mxfp8(rich_mx, beam):
    check_batch_invariance(rich_mx, beam)


@pytest.mark.parametrize("kind", ["f16", "mxfp8"])
def test_batch_invariance_trimmed(rich, rich_mx, tmp_path, kind):
    """mwx_full_batch_trimmed passes the params through: the trimmed clips of a
    batch with fit on equal each trimmed clip alone, and the compacted audio
    alone with its own audio_ctx (times apart: those are mapped back)."""
    ctx = rich[0] if kind == "f16" else rich_mx
    vpath = str(tmp_path / "ggml-silero-vad.bin")
    mwx.write_synthetic_vad_model(vpath, 3)
    clips = [vr.mixed_clip(), clip(31, 3.2), clip(32, 9.0)]
    n = len(clips)
    p = params(ctx, 1, fit=True)
    with mwx.VadContext(vpath) as v, v.trim_batch(clips, mwx.vad_params(threshold=0.76)) as t:
        base = len(ctx.states)
        assert ctx.full_batch_trimmed([t] * n, list(range(n)), p, state0=base) == 0
        batched = [records(ctx, base + i) for i in range(n)]
        compact = [t.pcm(i) for i in range(n)]
        for i in range(n):
            idx = len(ctx.states)
            assert ctx.full_batch_trimmed([t], [i], p, state0=idx) == 0
            assert records(ctx, idx) == batched[i], i
    ids = lambda rec: [(tok[0], tok[2], tok[3]) for s in rec for tok in s[4]]
    shorter = 0
    for i in range(n):
        if len(compact[i]) == 0:
            continue
        k = ctx.audio_ctx_for(len(compact[i]), 0, 0, True)
        shorter += k < ctx.audio_ctx_for(len(clips[i]), 0, 0, True)
        assert ids(run_fresh(ctx, compact[i], params(ctx, 1, audio_ctx=k))) == ids(batched[i]), (i, k)
    assert shorter > 0, "trimming must shorten some clip's context"


# ---- 5. cross readers -----------------------------------------------------------------
TOKS = lambda o: [o.sot, 300, 1234, o.beg, 777, 40000, 220, o.beg + 37, 11, 2050]


def test_cross_readers_f16(micro):
    """K = 96 through dec_attn_kernel's cross path (one row per step: item 1
    holds its logits to the oracle) and through the grouped kernel at 2, 5 and
    8 rows per slot (the prompt prefill's groups): bit-identical logits."""
    ctx, refs, _ = micro
    K = 96
    oK = refs.at(K)
    _, k, v = ctx.test_encode_ctx(clip(4, 3.0), K)
    toks = TOKS(oK)
    step = ctx.test_decode(toks)
    assert float(np.abs(step - oK.decode_seq(k, v, toks)).max()) < LOGITS_BOUND
    for n in (3, 6, 9):                      # prefill rows n - 1 = the cross group size
        assert np.array_equal(ctx.test_decode_last_prefill(toks[:n]), step[n - 1]), n


@pytest.mark.parametrize("mfs", [1, 0])
def test_cross_readers_mxfp8(make_model, workdir, monkeypatch, mfs):
    """The MX-fp8 cache at K = 96 with the scores on MFMA and on v_dot2: the
    MX decoder bound of test_gpu_parity.py, and the grouped sizes 2 and 5
    bit-identical to one row per step."""
    K = 96
    prev = mwx.lib().mwx_test_set_xattn_mfs(mfs)
    try:
        encode_at(monkeypatch, K)
        oracle_at(monkeypatch, workdir, K)
        TP.test_mxfp8_decoder_logits_match_mx_oracle(make_model)
        monkeypatch.undo()
        path = make_model("micro-rich", mwx.GGML_BF16)
        with mwx.Context.open(path, compute=mwx.COMPUTE_MXFP8) as ctx:
            ctx.test_encode_ctx(clip(4, 3.0), K)
            toks = [ctx.token("sot"), 300, 1234, ctx.token("beg"), 777, 40000, 220]
            step = ctx.test_decode(toks)
            for n in (3, 6):
                assert np.array_equal(ctx.test_decode_last_prefill(toks[:n]), step[n - 1]), n
    finally:
        mwx.lib().mwx_test_set_xattn_mfs(prev)


def test_readers_in_the_pipeline(rich):
    """Beam 5 and best-of 2 (sampling at t = 0.4) with fit on (128 frames): the
    grouped kernel at 5 and 2 rows per slot inside mwx_full, in a batch with a
    30-s neighbour and alone."""
    ctx, _, _ = rich
    short, long_ = clip(41, 1.9), clip(42, 30.0)
    for mode in ("beam5", "bestof2"):
        p = params(ctx, 5 if mode == "beam5" else 1, fit=True)
        if mode == "bestof2":
            p.temperature = 0.4
            p.greedy.best_of = 2
        assert ctx.audio_ctx_for(len(short), 0, 0, True) == 128
        base = len(ctx.states)
        assert ctx.full_batch_states([short, long_], p, [base, base + 1]) == 0
        both = [records(ctx, base), records(ctx, base + 1)]
        assert run_fresh(ctx, short, p) == both[0], mode
        assert run_fresh(ctx, long_, p) == both[1], mode


# ---- 6. DTW ---------------------------------------------------------------------------
def test_dtw_at_192(make_model):
    K = 192
    path = make_model("micro-rich")
    pcm = clip(0, 3.0)
    with mwx.Context.open(path) as off, \
            mwx.Context.open(path, dtw_preset=mwx.AHEADS_CUSTOM, dtw_heads=HEADS) as on:
        on.dtw_keep(True)
        assert off.full(pcm, params(off, audio_ctx=K)) == 0
        assert on.full(pcm, params(on, audio_ctx=K)) == 0
        strip = lambda rec: [(a, b, c, d, [t[:-1] for t in toks]) for a, b, c, d, toks in rec]
        assert strip(records(on)) == strip(records(off))
        eot = on.token("eot")
        assert _check_state(on, 0, eot, n_audio_ctx=K) > 0
        passes = on.dtw_passes(0)
        assert len(passes) == 1 and passes[0]["probs"].shape[2] == K
        t = [tok.t_dtw for s in on.segments() for tok in s.tokens if tok.id < eot]
        assert all(0 <= x < 2 * K for x in t) and t == sorted(t)
        # at full context the dump's key dim is unchanged
        assert on.full(pcm, params(on)) == 0
        assert on.dtw_passes(0)[0]["probs"].shape[2] == N_CTX


# ---- 7. errors ------------------------------------------------------------------------
def test_errors(rich):
    ctx, _, _ = rich
    pcm = clip(3, 2.0)
    assert ctx.full(pcm, params(ctx, audio_ctx=N_CTX + 1)) == -5
    assert ctx.full(pcm, params(ctx, audio_ctx=N_CTX + 1, fit=True)) == -5
    assert ctx.full(pcm, params(ctx), state_index=0) == 0
    assert ctx.full(pcm, params(ctx, audio_ctx=-3), state_index=1) == 0
    assert records(ctx, 0) == records(ctx, 1)
    assert ctx.full(pcm, params(ctx, audio_ctx=1), state_index=1) == 0       # the smallest context
    assert ctx.audio_ctx_for(len(pcm), 0, N_CTX + 1, False) == -1
    with pytest.raises(RuntimeError):
        ctx.test_encode_ctx(pcm, N_CTX + 1)
