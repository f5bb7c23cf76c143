"""Chunked long-form transcription on the GPU (csrc/k_vad.hip vad_chunks_kernel,
mwx_vad_trim_batch_chunked, mwx_full_batch_chunked, SttEngine's vad_chunk_s)
against the plain-Python restatement of the rule (tests/vad_chunks_restatement.py,
DESIGN.md D10).

Every expected value is an integer or a bit pattern. Where probabilities come
from the network, the restatement is applied to the segments the device
reports, which test_gpu_vad_segments.py pins to the segment rule.
"""
import ctypes as C
import os

import numpy as np
import pytest

import mwx
import vad_chunks_restatement as cr
import vad_restatement as vr
import vad_segments_restatement as sr
from test_gpu_vad_segments import (SEED, _c_params, _expected_json, _is_empty_result, _one,
                                   _records, _stt, two_clip)

pytestmark = pytest.mark.gpu

THR = 0.76


@pytest.fixture(scope="module")
def vad(tmp_path_factory):
    d = tmp_path_factory.mktemp("vadchunk")
    path = str(d / "ggml-silero-vad.bin")
    mwx.write_synthetic_vad_model(path, SEED)
    clips = {"mixed": vr.mixed_clip(), "zeros": np.zeros(20000, np.float32), "two": two_clip()}
    with mwx.VadContext(path) as v:
        yield {"dir": str(d), "ctx": v, "clips": clips}


def _want(p, N, prm, L):
    pcs, _ = sr.pieces(sr.segments(p, N, prm), prm)
    return pcs, cr.chunks(pcs, L)


# ---- 1. the kernel against the restatement --------------------------------------------
def test_kernel_equals_restatement(vad):
    v = vad["ctx"]
    cases = []  # (probs, N, Params, L)
    for name, L in sorted(cr.TABLE):
        rn, N, prm, _, _, _ = sr.TABLE[name]
        cases.append((sr.runs(*rn), N, prm, L))
    n_table = len(cases)
    for n in cr.ALT_N:
        for L in (511, 8959, 8960, 10 ** 9):
            cases.append(cr.alternating(n) + (L,))
    n_fixed = len(cases)
    rng = np.random.default_rng(2025)
    drawn = [sr.random_case(rng) for _ in range(300)]
    cases += [c + (int(rng.choice([512, 8000, 16000, 24000, 48000, 480000])),) for c in drawn]
    want = [_want(*c) for c in cases]
    # the table and the alternating cases are what the rule's text says
    for (name, L), (_, ch) in zip(sorted(cr.TABLE), want[:n_table]):
        assert ch == cr.TABLE[(name, L)], (name, L)
    k = n_table
    for i, n in enumerate(cr.ALT_N):
        for L in (511, 8959, 8960, 10 ** 9):
            pcs, ch = want[k]
            k += 1
            assert len(pcs) == cr.ALT_PIECES[i]
            if L in cr.ALT_CHUNKS:
                assert len(ch) == cr.ALT_CHUNKS[L][i], (n, L)
            if L == 8960:
                assert ch[:2] == cr.ALT_8960_FIRST_TWO
    # conditions on the random inputs
    n_pieces = [len(pcs) for pcs, _ in want[n_fixed:]]
    print("random cases: >= 2 pieces", sum(m >= 2 for m in n_pieces), "none",
          sum(m == 0 for m in n_pieces), "largest", max(n_pieces))
    assert sum(m >= 2 for m in n_pieces) >= 100
    assert sum(m == 0 for m in n_pieces) >= 30
    assert max(n_pieces) == 64
    assert sum(len(ch) >= 2 for _, ch in want[n_fixed:]) >= 30
    # all clips in one call
    got = v.test_chunks([c[0] for c in cases], [c[1] for c in cases],
                        [_c_params(c[2]) for c in cases], [c[3] for c in cases])
    for c, g, (_, ch) in zip(cases, got, want):
        assert g == ch, (c[2], c[1], c[3], c[0].tolist())
    # a sample alone: the fixed cases and every tenth random one
    for i in list(range(n_fixed)) + list(range(n_fixed, len(cases), 10)):
        p, N, prm, L = cases[i]
        assert v.test_chunks([p], [N], [_c_params(prm)], [L])[0] == want[i][1], i
    with pytest.raises(RuntimeError):  # the hook takes any cap >= 1
        v.test_chunks([cases[0][0]], [cases[0][1]], [_c_params(cases[0][2])], [0])


# ---- 2. the plan through the real pipeline --------------------------------------------
def test_plan_through_the_pipeline(vad):
    v = vad["ctx"]
    names = ["mixed", "zeros", "two"]
    clips = [vad["clips"][n] for n in names]
    prm = sr.Params(threshold=THR)
    cp = _c_params(prm)
    with v.trim_batch(clips, cp) as plain, v.trim_batch(clips, cp, chunk_s=1.0) as t:
        n_chunks = []
        for i, n in enumerate(names):
            segs = t.segments(i)
            pcs, total = sr.pieces(segs, prm)
            assert segs == plain.segments(i), n
            assert t.n_samples(i) == plain.n_samples(i) == total, n
            assert t.pcm(i).tobytes() == plain.pcm(i).tobytes(), n
            want = cr.chunks(pcs, 16000)
            assert t.chunks(i) == want, n
            # an object of the plain call: the whole compacted clip as one chunk
            assert plain.chunks(i) == ([(0, len(pcs), 0, total)] if pcs else []), n
            n_chunks.append(len(want))
            for j, ch in enumerate(want):
                for tc in list(range(-1, ch[3] // 160 + 3)):
                    for is_end in (False, True):
                        assert t.chunk_map_time(i, j, tc, is_end) == \
                            cr.chunk_map_time(pcs, ch, tc, is_end), (n, j, tc, is_end)
            for tc in range(-1, total // 160 + 3):
                for is_end in (False, True):
                    if pcs:
                        assert plain.chunk_map_time(i, 0, tc, is_end) == \
                            sr.map_time(pcs, tc, is_end)
        print("chunks per clip at chunk_s = 1.0:", dict(zip(names, n_chunks)))
        assert n_chunks[1] == 0
        assert max(n_chunks) >= 2
        L = mwx.lib()
        assert L.mwx_vad_trimmed_n_chunks(t.t, 3) == -1
        assert L.mwx_vad_trimmed_chunk(t.t, 0, n_chunks[0], None, None, None, None) != 0
    ptrs = (C.c_void_p * 1)(clips[0].ctypes.data)
    lens = (C.c_int * 1)(len(clips[0]))
    for bad in (0.5, 31.0, float("nan")):
        assert not mwx.lib().mwx_vad_trim_batch_chunked(v.vctx, cp, bad, ptrs, lens, 1), bad


# ---- 3. chunked transcription ---------------------------------------------------------
def _params(ctx):
    p = ctx.default_params(mwx.SAMPLING_GREEDY)
    p.language = b"en"
    p.temperature = 0.0
    p.temperature_inc = 0.0
    p.token_timestamps = True
    return p


def test_chunked_transcription(vad, make_model):
    """mixed / zeros / two at threshold 0.76, chunk_s = 1.0, micro-rich f16, VAD
    model seed 3: the clips of the issue satisfy every power condition."""
    v = vad["ctx"]
    names = ["mixed", "zeros", "two"]
    clips = [vad["clips"][n] for n in names]
    prm = sr.Params(threshold=THR)
    cp = _c_params(prm)
    with mwx.Context.open(make_model("micro-rich", mwx.GGML_F16)) as ctx:
        p = _params(ctx)
        with v.trim_batch(clips, cp, chunk_s=1.0) as t:
            assert ctx.full_batch_chunked([t] * 3, [0, 1, 2], p) == 0
            got = [_records(ctx, i) for i in range(3)]
            for mb in (1, 2):  # scratch-state reuse, the per-state mel cache with other audio
                assert ctx.full_batch_chunked([t] * 3, [0, 1, 2], p, max_batch=mb) == 0
                assert [_records(ctx, i) for i in range(3)] == got, mb
            assert ctx.full_batch_chunked([t] * 3, [0, 1, 2], p) == 0
            assert [_records(ctx, i) for i in range(3)] == got
            # errors leave 0 segments
            assert ctx.full_batch_chunked([t] * 2, [0, 3], p) != 0  # no such clip
            assert [_records(ctx, i) for i in range(2)] == [[], []]
            assert ctx.full_batch_chunked([t] * 3, [0, 1, 2], p) == 0
            assert [_records(ctx, i) for i in range(3)] == got
            p_off = _params(ctx)
            p_off.offset_ms = 10
            assert ctx.full_batch_chunked([t] * 3, [0, 1, 2], p_off) != 0
            assert [_records(ctx, i) for i in range(3)] == [[], [], []]
            assert ctx.full_batch_chunked([t] * 3, [0, 1, 2], p, max_batch=0) != 0
            # the reference: every chunk's slice of the compacted clip, run alone
            want = []
            n_moved = n_from_chunks = 0
            for i in range(3):
                pcs, _ = sr.pieces(t.segments(i), prm)
                chs = cr.chunks(pcs, 16000)
                assert t.chunks(i) == chs
                pcm = t.pcm(i)
                recs, sources = [], set()
                for j, ch in enumerate(chs):
                    assert ctx.full_batch_states([pcm[ch[2]:ch[2] + ch[3]]], p, [8]) == 0
                    for t0, t1, text, toks in _records(ctx, 8):
                        m0 = cr.chunk_map_time(pcs, ch, t0, False)
                        m1 = cr.chunk_map_time(pcs, ch, t1, True)
                        mt = [(tid, pr, pl, cr.chunk_map_time(pcs, ch, a, False),
                               cr.chunk_map_time(pcs, ch, b, True)) for tid, pr, pl, a, b in toks]
                        n_moved += (m0 != t0) + (m1 != t1) + sum(
                            (x[3] != y[3]) + (x[4] != y[4]) for x, y in zip(mt, toks))
                        recs.append((m0, m1, text, mt))
                        sources.add(j)
                n_from_chunks = max(n_from_chunks, len(sources))
                want.append(recs)
            n_segments = sum(len(w) for w in want)
            print(f"segments: {n_segments}, times moved by the map: {n_moved}, most chunks "
                  f"contributing to one clip: {n_from_chunks}")
            assert n_segments > 0 and n_moved > 0 and n_from_chunks >= 2
            assert got == want
            assert got[1] == []
        # chunk_s = 30, and an object of plain trim_batch: mwx_full_batch_trimmed's records
        with v.trim_batch(clips, cp) as plain, v.trim_batch(clips, cp, chunk_s=30.0) as t30:
            assert ctx.full_batch_trimmed([plain] * 3, [0, 1, 2], p) == 0
            trimmed = [_records(ctx, i) for i in range(3)]
            assert sum(len(r) for r in trimmed) > 0
            for obj in (t30, plain):
                assert [len(obj.chunks(i)) for i in range(3)] == [1, 0, 1]
                assert ctx.full_batch_chunked([obj] * 3, [0, 1, 2], p) == 0
                assert [_records(ctx, i) for i in range(3)] == trimmed


# ---- 4. the host engine ---------------------------------------------------------------
def _speaker_ids(L, results, x):
    """The speakers of `results` (segments of clip x on its own timeline),
    clustered in order as the engine does it."""
    lens = []
    for r in results:
        s0 = max(0, min(int(r["t0"] / 100.0 * 16000.0), len(x)))
        s1 = max(s0, min(int(r["t1"] / 100.0 * 16000.0), len(x)))
        lens.append(s1 - s0)
    long = [i for i, ln in enumerate(lens) if ln >= 160]
    buf = C.create_string_buffer(1 << 16)
    if long:
        lv = np.ascontiguousarray([results[i]["speaker_vec"] for i in long], np.float32)
        assert L.mwx_stt_cluster_ids(mwx.fptr(lv), len(long), 0.88, buf, 1 << 16) >= 0
        for i, sid in zip(long, buf.value.decode().split("\n")):
            results[i]["speaker"] = sid
    for i, ln in enumerate(lens):
        if ln < 160:
            results[i]["speaker"] = "?"


def test_host_vad_chunk(vad):
    d = vad["dir"]
    mwx.write_synthetic_model(os.path.join(d, "ggml-micro.bin"), "micro-rich", mwx.GGML_F16, 0)
    v = vad["ctx"]
    mixed, two, zeros = (vad["clips"][n] for n in ("mixed", "two", "zeros"))
    L = _stt()
    L.mwx_stt_set_vad_chunk.argtypes = [C.c_void_p, C.c_float, C.c_int]

    def new(ctor, enable, *more, max_batch=1, vad_ms_min=500):
        eng = ctor(d.encode(), b"ggml-micro.bin", 2, 5000, 1, b"en", vad_ms_min, 0, max_batch, 2000,
                   8000, int(enable), b"ggml-silero-vad.bin", THR, *more)
        assert eng
        engines.append(eng)
        return eng

    engines = []
    try:
        # (no minimum duration: a chunk may be shorter than a request may be)
        off = new(L.mwx_stt_new_vad, False, vad_ms_min=0)
        trim = new(L.mwx_stt_new_vad_trim, True, 1)
        chunk = new(L.mwx_stt_new_vad_trim, True, 1)
        chunk_q = new(L.mwx_stt_new_vad_trim, True, 1, max_batch=2)
        gate = new(L.mwx_stt_new_vad, True)
        for eng in (chunk, chunk_q):
            assert L.mwx_stt_set_vad_chunk(eng, 0.5, 32) == -1
            assert L.mwx_stt_set_vad_chunk(eng, 1.0, 32) == 1
        assert L.mwx_stt_set_vad_chunk(gate, 1.0, 32) == 0  # no vad_trim: set, inactive
        # the host's parameters: its threshold, max_speech_duration_s = min(FLT_MAX, chunk_s)
        prm = sr.Params(threshold=THR, max_speech_duration_s=1.0)
        want = {}
        with v.trim_batch([mixed, two], _c_params(prm), chunk_s=1.0) as t, \
                mwx.Context.open(os.path.join(d, "ggml-micro.bin")) as ctx:
            for i, (n, x) in enumerate((("mixed", mixed), ("two", two))):
                pcs, _ = sr.pieces(t.segments(i), prm)
                chs = t.chunks(i)
                assert chs == cr.chunks(pcs, 16000) and len(chs) >= 2
                pcm = t.pcm(i)
                res = []
                for ch in chs:
                    res += _expected_json(L, ctx, _one(L, off, pcm[ch[2]:ch[2] + ch[3]]),
                                          cr.chunk_pieces(pcs, ch), x)
                _speaker_ids(L, res, x)
                want[n] = res
        assert all(len(w) > 0 for w in want.values())
        before = {n: _one(L, trim, vad["clips"][n]) for n in ("mixed", "two")}
        assert any(want[n] != before[n] for n in want)  # chunking shows in the result
        for eng in (chunk, chunk_q):  # transcribe(): direct, and through the request batcher
            assert _one(L, eng, mixed) == want["mixed"]
            assert _one(L, eng, two) == want["two"]
            _is_empty_result(_one(L, eng, zeros), len(zeros))
        # chunking off again: today's vad_trim output
        for eng in (chunk, chunk_q):
            assert L.mwx_stt_set_vad_chunk(eng, 0.0, 32) == 0
            for n in ("mixed", "two"):
                assert _one(L, eng, vad["clips"][n]) == before[n]
        assert _one(L, gate, mixed) == _one(L, off, mixed)
    finally:
        for e in engines:
            L.mwx_stt_free(e)
