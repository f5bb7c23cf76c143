"""One language per recording in chunked long-form transcription
(mwx_full_params.chunk_language = MWX_CHUNK_LANG_RECORDING)
against the plain-Python restatement of the rule
(tests/lang_pool_restatement.py), with the VAD fixtures of
test_gpu_vad_chunks.py (VAD model seed 3, threshold 0.76, chunk_s = 1.0) and
the micro-ml-rich model.

Every expected value is an integer or a bit pattern: the pooled probabilities
are the restatement's double accumulation, rounded to float, of the
probabilities each pooled chunk gives when run alone with detect_language; the
segments are those of each chunk run alone with the pooled language.

A recording whose per-chunk languages differ from the pooled one was looked
for among burst_clip(seed), seed in SEEDS_LOOKED_AT, and found: seed 33 has
three chunks whose own languages are 73, 82 and 39 and pools to 82
(DIFFERING); the test asserts that this still holds.
"""
import numpy as np
import pytest

import lang_pool_restatement as lp
import mwx
import vad_chunks_restatement as cr
import vad_restatement as vr
import vad_segments_restatement as sr
from test_gpu_vad_segments import SEED, _c_params, _records, two_clip

pytestmark = pytest.mark.gpu

THR = 0.76
SEEDS_LOOKED_AT = (31, 32, 33, 34, 35, 36)
# The seed of SEEDS_LOOKED_AT whose recording has a chunk whose own language
# (chunk_language = 0) differs from the recording's pooled one, or None if the
# list has none (then the first seed is used and that power condition is not
# asserted).
DIFFERING = 33


def burst_clip(seed):
    """7 s of zeros with three bursts of Gaussian noise of seeded lengths,
    levels and spectral tilt (a one-pole low-pass of seeded strength)."""
    rng = np.random.default_rng(seed)
    x = np.zeros(7 * 16000 + 31, np.float32)
    at = 4000
    for _ in range(3):
        n = int(rng.integers(14000, 26000))
        b = rng.standard_normal(n)
        a = float(rng.uniform(0.0, 0.9))
        for i in range(1, n):
            b[i] += a * b[i - 1]
        b *= float(rng.uniform(0.2, 0.4)) / np.abs(b).max() * 3.0
        x[at:at + n] = np.clip(b, -1.0, 1.0).astype(np.float32)
        at += n + int(rng.integers(6000, 12000))
    return x


@pytest.fixture(scope="module")
def vad(tmp_path_factory):
    d = tmp_path_factory.mktemp("vadlang")
    path = str(d / "ggml-silero-vad.bin")
    mwx.write_synthetic_vad_model(path, SEED)
    seed = SEEDS_LOOKED_AT[0] if DIFFERING is None else DIFFERING
    clips = [vr.mixed_clip(), np.zeros(20000, np.float32), two_clip(), burst_clip(seed)]
    with mwx.VadContext(path) as v:
        yield {"ctx": v, "clips": clips}


def _params(ctx, language=b"auto", chunk_language=mwx.CHUNK_LANG_RECORDING):
    p = ctx.default_params(mwx.SAMPLING_GREEDY)
    p.language = language
    p.temperature = 0.0
    p.temperature_inc = 0.0
    p.token_timestamps = True
    p.chunk_language = chunk_language
    return p


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()


def _chunk_records(ctx, pcs, ch, pcm, p, state=8):
    """The chunk's slice of the compacted clip run alone with p: its records on
    the caller's timeline, and the state's language."""
    assert ctx.full_batch_states([pcm[ch[2]:ch[2] + ch[3]]], p, [state]) == 0
    recs = []
    for t0, t1, text, toks in _records(ctx, state):
        recs.append((cr.chunk_map_time(pcs, ch, t0, False), cr.chunk_map_time(pcs, ch, t1, True),
                     text, [(tid, pr, pl, cr.chunk_map_time(pcs, ch, a, False),
                             cr.chunk_map_time(pcs, ch, b, True)) for tid, pr, pl, a, b in toks]))
    return recs, ctx.lang_id(state)


def test_one_language_per_recording(vad, make_model):
    v = vad["ctx"]
    clips = vad["clips"]
    n = len(clips)
    prm = sr.Params(threshold=THR)
    with mwx.Context.open(make_model("micro-ml-rich", mwx.GGML_F16)) as ctx, \
            v.trim_batch(clips, _c_params(prm), chunk_s=1.0) as t:
        p = _params(ctx)
        assert ctx.full_batch_chunked([t] * n, list(range(n)), p) == 0
        got = [(_records(ctx, i), ctx.lang_id(i), bits(ctx.lang_probs(i))) for i in range(n)]
        # the result does not depend on max_batch
        for mb in (1, 2, 32):
            assert ctx.full_batch_chunked([t] * n, list(range(n)), p, max_batch=mb) == 0
            again = [(_records(ctx, i), ctx.lang_id(i), bits(ctx.lang_probs(i))) for i in range(n)]
            assert again == got, mb
        # the restatement over each pooled chunk's own detection
        pd = _params(ctx)
        pd.detect_language = True
        want, per_chunk, pooled_lang, n_multi = [], [], [], 0
        for i in range(n):
            pcs, _ = sr.pieces(t.segments(i), prm)
            chs = t.chunks(i)
            assert chs == cr.chunks(pcs, 16000)
            pcm = t.pcm(i)
            lens = [ch[3] for ch in chs]
            idx = lp.pooled_chunks(lens)
            if not idx:
                want.append(([], None, []))
                per_chunk.append([])
                pooled_lang.append(-1)
                continue
            probs = []
            for j in idx:
                ch = chs[j]
                assert ctx.full_batch_states([pcm[ch[2]:ch[2] + ch[3]]], pd, [8]) == 0
                assert ctx.segments(8) == []
                probs.append(ctx.lang_probs(8))
                assert probs[-1].shape == (100,)
            P, lang = lp.pool([lens[j] for j in idx], probs)
            n_multi += len(idx) >= 2
            fixed = _params(ctx, mwx.lang_str(lang).encode())
            recs, langs = [], []
            for ch in chs:
                r, used = _chunk_records(ctx, pcs, ch, pcm, fixed)
                assert used == lang
                recs += r
                langs.append(_chunk_records(ctx, pcs, ch, pcm, _params(ctx))[1])
            want.append((recs, lang, bits(P)))
            per_chunk.append(langs)
            pooled_lang.append(lang)
        print("chunks pooled per recording >= 2:", n_multi, "per-chunk languages:", per_chunk,
              "pooled:", pooled_lang)
        assert n_multi >= 2  # two recordings with several chunks each, at least
        for i in range(n):
            if want[i][1] is None:  # no chunk of at least 0.1 s: no segments, nothing detected
                assert got[i][0] == [] and got[i][2] == []
                continue
            assert got[i] == want[i], i
            assert got[i][1] == int(np.argmax(np.array(got[i][2], np.uint32).view(np.float32)))
        assert sum(len(g[0]) for g in got) > 0
        if DIFFERING is not None:
            assert any(l != pooled_lang[n - 1] for l in per_chunk[n - 1])
        # lang_ids wins over the pooling: entry 0 fixed, the others pooled
        tr = mwx.lang_id("tr")
        assert ctx.full_batch_chunked([t] * n, list(range(n)), p, lang_ids=[tr] + [-1] * (n - 1)) == 0
        assert ctx.lang_id(0) == tr and ctx.lang_probs(0).size == 0
        assert [(_records(ctx, i), ctx.lang_id(i), bits(ctx.lang_probs(i)))
                for i in range(1, n)] == got[1:]
        pcs, _ = sr.pieces(t.segments(0), prm)
        recs = []
        for ch in t.chunks(0):
            recs += _chunk_records(ctx, pcs, ch, t.pcm(0), _params(ctx, b"tr"))[0]
        assert _records(ctx, 0) == recs
        assert ctx.full_batch_chunked([t] * n, list(range(n)), p, lang_ids=[100] * n) == -3
        assert [_records(ctx, i) for i in range(n)] == [[]] * n


def test_per_chunk_mode_is_unchanged(vad, make_model):
    """chunk_language = 0: every chunk detects its own language, as before; the
    state reports chunk 0's language and now also its probabilities."""
    v = vad["ctx"]
    clips = vad["clips"]
    n = len(clips)
    prm = sr.Params(threshold=THR)
    with mwx.Context.open(make_model("micro-ml-rich", mwx.GGML_F16)) as ctx, \
            v.trim_batch(clips, _c_params(prm), chunk_s=1.0) as t:
        p = _params(ctx, chunk_language=mwx.CHUNK_LANG_PER_CHUNK)
        assert ctx.full_batch_chunked([t] * n, list(range(n)), p) == 0
        got = [_records(ctx, i) for i in range(n)]
        langs = [ctx.lang_id(i) for i in range(n)]
        probs = [bits(ctx.lang_probs(i)) for i in range(n)]
        for i in range(n):
            pcs, _ = sr.pieces(t.segments(i), prm)
            chs = t.chunks(i)
            recs = []
            for j, ch in enumerate(chs):
                r, used = _chunk_records(ctx, pcs, ch, t.pcm(i), p)
                recs += r
                if j == 0:
                    assert langs[i] == used and probs[i] == bits(ctx.lang_probs(8))
            assert got[i] == recs, i
            if not chs:
                assert probs[i] == []
        assert sum(len(g) for g in got) > 0
        # a fixed language ignores chunk_language
        pf = _params(ctx, b"en")
        assert ctx.full_batch_chunked([t] * n, list(range(n)), pf) == 0
        fixed = [_records(ctx, i) for i in range(n)]
        pf.chunk_language = mwx.CHUNK_LANG_PER_CHUNK
        assert ctx.full_batch_chunked([t] * n, list(range(n)), pf) == 0
        assert [_records(ctx, i) for i in range(n)] == fixed
        assert all(ctx.lang_probs(i).size == 0 for i in range(n))
