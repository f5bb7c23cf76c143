"""Transcript alignment on the GPU (mwx_align_batch / mwx_align_row, rule D12 of
DESIGN.md; Driver::align_pass, k_score.hip) on the micro geometry.

The references are pre-existing code: the engine's own decode steps
(mwx_test_encode + mwx_test_decode on the D12 sequence give the raw step
logits), the CPU oracle's teacher-forced decoder, the DTW pass of
mwx_full_batch and of mwx_test_dtw_align, and mwx_full_batch's language
detection. Scores are held to the bound of tests/score_ref.py (b_lp at the
target and at the top, b_p) around the float64 log-softmax of the reference
logits; top_id, t_dtw, the batch / block-size invariance and the untouched
decode state are exact.

Worst |err| / bound observed on MI355X (the tests print it): against the decode
steps 0.435 (f16), 0.441 (bf16), 0.429 (MX-fp8); against the CPU oracle 0.285
of 2 eps_row + b_lp, eps_row up to 1.9e-2."""
import ctypes as C

import numpy as np
import pytest

import mwx
import orc
import score_ref as sr

pytestmark = pytest.mark.gpu

HEADS = [(0, 1), (1, 0), (1, 1)]
NS = (0, 1, 7, 8, 9, 224)


def clip(k, seconds):
    return mwx.pcm16_to_f32(mwx.synth_pcm16(k, int(seconds * 16000)))


def text_tokens(seed, n, eot):
    return [int(t) for t in np.random.default_rng([17, seed, n]).integers(0, eot, n)]


def d12_seq(ctx, toks, lang_id=None, translate=False):
    """(sequence, pos0): sot sequence, NOT, the text, EOT."""
    s = [ctx.token("sot")]
    if lang_id is not None:
        s += [ctx.token("sot") + 1 + lang_id,
              ctx.token("translate") if translate else ctx.token("transcribe")]
    pos0 = len(s)
    return s + [ctx.token("not")] + list(toks) + [ctx.token("eot")], pos0


def params(ctx, language=b"en", **kw):
    p = ctx.default_params(mwx.SAMPLING_GREEDY)
    p.language = language
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def result(ctx, state=0):
    """The state's alignment result: segments as plain tuples (floats as bits)
    and the score rows as bits."""
    b = lambda v: int(np.array([v], np.float32).view(np.uint32)[0])
    segs = [(s.t0, s.t1, s.text, [(t.id, t.tid, b(t.p), b(t.plog), t.pt, t.ptsum, t.t0, t.t1,
                                   t.t_dtw) for t in s.tokens]) for s in ctx.segments(state)]
    rows = ctx.align_rows(state)
    return segs, [tuple(np.array(list(r), np.float64).view(np.uint64).tolist()) for r in rows]


def check_rows(ctx, state, toks, logits, extra=None, label=""):
    """The state's rows against raw reference logits [n + 1][V] (float32):
    top_id exact, plog / top_plog / p within the bound (+ extra[i] per row).
    Returns the worst |err| / allowance."""
    eot = ctx.token("eot")
    segs = ctx.segments(state)
    rows = ctx.align_rows(state)
    n = len(toks)
    assert len(segs) == 1 and len(segs[0].tokens) == n and len(rows) == n + 1
    worst = 0.0
    for i in range(n + 1):
        t = toks[i] if i < n else eot
        r = sr.reference(logits[i], t)
        ex = 0.0 if extra is None else float(extra[i])
        if extra is None:
            assert int(rows["top_id"][i]) == r["top_id"], (label, i)
        got = [(float(rows["plog"][i]), r["plog"], r["b_plog"]),
               (float(rows["top_plog"][i]), r["top_plog"], r["b_top_plog"])]
        if i < n:
            td = segs[0].tokens[i]
            assert td.id == t and np.float32(td.plog) == rows["plog"][i]
            if extra is None:
                got.append((float(td.p), r["p"], r["b_p"]))
        for g, want, b in got:
            allow = b + ex
            assert abs(g - want) <= allow, (label, i, g, want, abs(g - want) / allow)
            worst = max(worst, abs(g - want) / allow)
    return worst


@pytest.fixture(scope="module")
def pcm30():
    return clip(0, 30)


# ---- 1. against the engine's own decode steps ---------------------------------------
@pytest.mark.parametrize("kind", ["f16", "bf16", "mxfp8"])
def test_against_decode_steps(make_model, pcm30, kind):
    path = make_model("micro-rich", mwx.GGML_F16 if kind == "f16" else mwx.GGML_BF16)
    compute = mwx.COMPUTE_MXFP8 if kind == "mxfp8" else mwx.COMPUTE_MODEL
    with mwx.Context.open(path, compute=compute) as ctx:
        eot = ctx.token("eot")
        worst = 0.0
        for n in NS:
            toks = text_tokens(1, n, eot)
            seq, pos0 = d12_seq(ctx, toks)
            ctx.test_encode(pcm30, cross=False)
            steps = ctx.test_decode(seq)[pos0:pos0 + n + 1]
            assert ctx.align_batch([pcm30], [toks], params(ctx)) == 0
            worst = max(worst, check_rows(ctx, 0, toks, steps, label=(kind, n)))
            seg = ctx.segments(0)[0]
            assert (seg.t0, seg.t1) == (0, 2999)
            assert all(t.t_dtw == -1 and t.tid == t.id and t.pt == 0 and t.ptsum == 0 and
                       t.t0 == -1 and t.t1 == -1 for t in seg.tokens)
        print(f"{kind}: worst |err| / bound against the decode steps {worst:.3f}")


# ---- 2. against the CPU oracle ---------------------------------------------------------
def test_against_cpu_oracle(make_model, pcm30):
    path = make_model("micro-rich", mwx.GGML_F16)
    o = orc.Oracle(path)
    with mwx.Context.open(path) as ctx:
        toks = text_tokens(2, 9, ctx.token("eot"))
        seq, pos0 = d12_seq(ctx, toks)
        mel, _ = o.mel(pcm30)
        k, v = o.cross(o.encode(mel, 0))
        ref = o.decode_seq(k, v, seq)[pos0:pos0 + len(toks) + 1]
        ctx.test_encode(pcm30, cross=False)
        dev = ctx.test_decode(seq)[pos0:pos0 + len(toks) + 1]
        eps = np.abs(dev.astype(np.float64) - ref.astype(np.float64)).max(axis=1)
        assert ctx.align_batch([pcm30], [toks], params(ctx)) == 0
        # log-softmax moves by at most 2 eps under a sup-norm perturbation eps
        worst = check_rows(ctx, 0, toks, ref, extra=2.0 * eps, label="oracle")
        print(f"oracle: eps_row up to {eps.max():.3e}, worst |err| / (2 eps_row + b_lp) {worst:.3f}")


# ---- 3. times ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(make_model):
    path = make_model("micro-rich", mwx.GGML_F16)
    with mwx.Context.open(path) as off, \
            mwx.Context.open(path, dtw_preset=mwx.AHEADS_CUSTOM, dtw_heads=HEADS) as on:
        yield off, on


def test_times_equal_the_dtw_hook(pair):
    off, on = pair
    pcm = clip(1, 12)
    n_cols = min(1500, (1 + (len(pcm) - 200) // 160 + 1) // 2)
    for n in (1, 9, 224):
        toks = text_tokens(3, n, on.token("eot"))
        seq, pos0 = d12_seq(on, toks)
        on.test_encode(pcm, cross=False)
        frames = on.test_dtw_align(seq, pos0, n_cols)["frames"]
        assert on.align_batch([pcm], [toks], params(on)) == 0
        got = [t.t_dtw for t in on.segments(0)[0].tokens]
        assert got == [2 * int(f) for f in frames[1:n + 1]], n
        # without DTW: every time -1, the scores the same bits
        assert off.align_batch([pcm], [toks], params(off)) == 0
        s_on, r_on = result(on)
        s_off, r_off = result(off)
        assert r_on == r_off
        assert [t[:8] for t in s_on[0][3]] == [t[:8] for t in s_off[0][3]]
        assert all(t[8] == -1 for t in s_off[0][3])
    assert on.align_batch([pcm], [[]], params(on)) == 0
    assert on.segments(0)[0].tokens == [] and len(on.align_rows(0)) == 1


def test_times_equal_full_batch(pair):
    _, on = pair
    clips = [clip(0, 30), clip(1, 12), clip(2, 1.25)]
    p = params(on, no_timestamps=True, temperature_inc=0.0)
    for i in range(len(clips)):
        on.dtw_keep(True, i)
    assert on.full_batch(clips, p) == 0
    eot = on.token("eot")
    n_checked = 0
    for i, pcm in enumerate(clips):
        toks = [(t.id, t.t_dtw) for s in on.segments(i) for t in s.tokens if t.id < eot]
        if not toks:
            continue
        assert len(on.dtw_passes(i)) == 1
        ids = [t[0] for t in toks]
        assert on.align_batch([pcm], [ids], params(on), [4]) == 0
        assert [t.t_dtw for t in on.segments(4)[0].tokens] == [t[1] for t in toks], i
        n_checked += len(ids)
    for i in range(len(clips)):
        on.dtw_keep(False, i)
    assert n_checked > 0


# ---- 4. batch, block size, decode state --------------------------------------------------
def test_batch_invariance_and_decode_state(pair):
    _, on = pair
    eot = on.token("eot")
    clips = [clip(0, 30), clip(1, 12), clip(2, 1.25)]
    toks = [text_tokens(4, n, eot) for n in (224, 0, 1)]
    p = params(on, audio_ctx_fit=True)
    pf = params(on, temperature_inc=0.0, token_timestamps=True)
    rec = lambda i: [(s.t0, s.t1, s.text, [(t.id, t.tid, t.p, t.plog, t.pt, t.ptsum, t.t0, t.t1,
                                            t.t_dtw) for t in s.tokens]) for s in on.segments(i)]
    assert on.full_batch(clips, pf) == 0
    before = [rec(i) for i in range(3)]
    assert on.align_batch(clips, toks, p) == 0
    batch = [result(on, i) for i in range(3)]
    assert [len(b[1]) for b in batch] == [225, 1, 2]
    assert on.audio_ctx_for(len(clips[2]), 0, 0, True) < 1500
    for i in range(3):
        assert on.align_batch([clips[i]], [toks[i]], p, [5]) == 0
        assert result(on, 5) == batch[i], i
    try:
        assert mwx.set_score_rows_cap(8) == 256
        assert on.align_batch(clips, toks, p) == 0
        assert [result(on, i) for i in range(3)] == batch
    finally:
        assert mwx.set_score_rows_cap(0) == 8
    assert on.align_batch(clips, toks, p) == 0
    assert on.full_batch(clips, pf) == 0
    assert [rec(i) for i in range(3)] == before


# ---- 5. language ---------------------------------------------------------------------------
def test_language(make_model):
    path = make_model("micro-ml-rich", mwx.GGML_F16)
    pcm = clip(3, 12)
    L = mwx.lib()
    L.mwx_lang_id.argtypes = [C.c_char_p]
    with mwx.Context.open(path) as ctx:
        toks = text_tokens(5, 7, ctx.token("eot"))
        assert ctx.full(pcm, params(ctx, language=b"auto", temperature_inc=0.0)) == 0
        detected = ctx.lang_id(0)
        assert ctx.align_batch([pcm], [toks], params(ctx, language=b"auto"), [1]) == 0
        assert ctx.lang_id(1) == detected
        auto = result(ctx, 1)
        de = L.mwx_lang_id(b"de")
        assert de >= 0
        seen = [auto]
        for lang, lid, tr in ((b"de", de, False), (b"de", de, True)):
            seq, pos0 = d12_seq(ctx, toks, lid, tr)
            ctx.test_encode(pcm, cross=False)
            steps = ctx.test_decode(seq)[pos0:pos0 + len(toks) + 1]
            assert ctx.align_batch([pcm], [toks], params(ctx, language=lang, translate=tr)) == 0
            assert ctx.lang_id(0) == lid
            check_rows(ctx, 0, toks, steps, label=(lang, tr))
            seen.append(result(ctx, 0))
        if detected != de:
            assert seen[0] != seen[1]
        assert seen[1] != seen[2], "translate changes the sot sequence"
        assert ctx.align_batch([pcm], [toks], params(ctx, language=b"xx")) == -3


# ---- 6. errors and limits --------------------------------------------------------------------
def test_errors_leave_the_state_intact(make_model):
    with mwx.Context.open(make_model("micro-rich", mwx.GGML_F16)) as ctx:
        eot = ctx.token("eot")
        pcm = clip(1, 3)
        toks = text_tokens(6, 5, eot)
        assert ctx.align_batch([pcm], [toks], params(ctx)) == 0
        good = result(ctx)
        assert len(good[1]) == 6
        bad = [
            (-3, [pcm], [toks[:2] + [eot]], params(ctx)),
            (-3, [pcm], [[-1]], params(ctx)),
            (-1, [pcm], [text_tokens(6, 225, eot)], params(ctx)),
            (-1, [np.zeros(480001, np.float32)], [toks], params(ctx)),
            (-1, [], [], params(ctx)),
            (-1, [pcm], [toks], params(ctx, offset_ms=10)),
            (-1, [pcm], [toks], params(ctx, duration_ms=10)),
            (-5, [pcm], [toks], params(ctx, audio_ctx=1501)),
        ]
        for rc, clips, tk, p in bad:
            assert ctx.align_batch(clips, tk, p) == rc, rc
            assert result(ctx) == good
        # the limits themselves pass
        assert ctx.align_batch([np.zeros(480000, np.float32) + clip(2, 30)],
                               [text_tokens(6, 224, eot)], params(ctx)) == 0
        assert len(ctx.align_rows(0)) == 225
        # the abort callback: before the encode, then before the pass
        for after, rc in ((0, -6), (1, -9)):
            calls = [0]

            def cb(_):
                calls[0] += 1
                return calls[0] > after
            keep = mwx.ABORT_CB(cb)
            assert ctx.align_batch([pcm], [toks], params(ctx, abort_callback=keep)) == rc
        # a clip too short to decode: no segment, no rows
        assert ctx.align_batch([pcm[:1000]], [toks], params(ctx)) == 0
        assert ctx.segments(0) == [] and len(ctx.align_rows(0)) == 0


# ---- 7. host ---------------------------------------------------------------------------------
def test_host_align_pcm16(make_model, tmp_path):
    import os
    import shutil
    path = make_model("micro-rich", mwx.GGML_F16)
    shutil.copy(path, tmp_path / "ggml-micro.bin")
    pcm8k = mwx.synth_pcm16(4, 5 * 8000, 8000)
    text = "  hello world \n"
    L = mwx.stt_lib()
    eng = L.mwx_stt_new(str(tmp_path).encode(), b"ggml-micro.bin", 1, 20000, 1, b"en", 500, 0)
    assert eng
    try:
        got = mwx.stt_align_pcm16(L, eng, pcm8k, 8000, text, "en")
    finally:
        L.mwx_stt_free(eng)
    with mwx.Context.open(path) as ctx:
        pcm16k = ctx.resample(mwx.pcm16_to_f32(pcm8k), 8000, 16000)
        buf = (C.c_int32 * 224)()
        n = mwx.lib().mwx_tokenize(ctx.ctx, b" hello world", buf, 224)
        assert n > 0
        toks = list(buf[:n])
        assert ctx.align_batch([pcm16k], [toks], params(ctx)) == 0
        seg = ctx.segments(0)[0]
        rows = ctx.align_rows(0)
    assert got["ok"] and got["language"] == "en" and got["text"] == seg.text
    assert [t["id"] for t in got["tokens"]] == toks
    f32 = lambda v: np.float32(v)
    for i, t in enumerate(got["tokens"]):
        assert f32(t["plog"]) == rows["plog"][i] and f32(t["p"]) == f32(seg.tokens[i].p)
        assert t["top_id"] == rows["top_id"][i] and f32(t["top_plog"]) == rows["top_plog"][i]
        assert t["t"] == -1
    assert f32(got["eot_logprob"]) == rows["plog"][n]
    assert got["n_agree"] == sum(int(rows["top_id"][i]) == toks[i] for i in range(n))
    assert abs(got["avg_logprob"] - float(np.mean(rows["plog"][:n].astype(np.float64)))) < 1e-5
