"""VAD speech segments and silence-trimmed transcription on the GPU
(csrc/k_vad.hip vad_segments_kernel / vad_compact_kernel, mwx_vad_segments_*,
mwx_vad_trim_batch, mwx_full_batch_trimmed, SttEngine's vad_trim) against the
plain-Python restatement of the rule (tests/vad_segments_restatement.py).

Every expected value is an integer or a bit pattern. Where probabilities come
from the network, the restatement is applied to the device's own f32
probabilities, so the same numbers meet the same f32 thresholds.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mwx
import vad_restatement as vr
import vad_segments_restatement as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STT_LIB = os.path.join(ROOT, "sentiric-stt-whisper-service_amd", "libmwx_stt.so")
SEED = 3  # the VAD model of test_gpu_vad.py


def _c_params(prm: sr.Params) -> mwx.VadParams:
    return mwx.vad_params(threshold=prm.threshold,
                          min_speech_duration_ms=prm.min_speech_duration_ms,
                          min_silence_duration_ms=prm.min_silence_duration_ms,
                          max_speech_duration_s=prm.max_speech_duration_s,
                          speech_pad_ms=prm.speech_pad_ms, samples_overlap=prm.samples_overlap)


def two_clip():
    """5 s + 77 samples of zeros with two noise bursts."""
    rng = np.random.default_rng(11)
    x = np.zeros(5 * 16000 + 77, np.float32)
    x[8000:30000] = (0.3 * rng.standard_normal(22000)).astype(np.float32)
    x[52000:72000] = (0.3 * rng.standard_normal(20000)).astype(np.float32)
    return x


@pytest.fixture(scope="module")
def vad(tmp_path_factory):
    d = tmp_path_factory.mktemp("vadseg")
    path = str(d / "ggml-silero-vad.bin")
    mwx.write_synthetic_vad_model(path, SEED)
    clips = {"mixed": vr.mixed_clip(), "two": two_clip(), "zeros": np.zeros(20000, np.float32),
             "noise": vr.noise_clip(3 * 16000 + 5, seed=21)}
    with mwx.VadContext(path) as v:
        probs = {k: v.detect(x) for k, x in clips.items()}
        yield {"dir": str(d), "ctx": v, "clips": clips, "probs": probs}


def _expect(p, N, prm):
    segs = sr.segments(p, N, prm)
    pcs, total = sr.pieces(segs, prm)
    return segs, pcs, total


# ---- 1. the table ---------------------------------------------------------------------
def test_table(vad):
    v = vad["ctx"]
    names = sorted(sr.TABLE)
    probs = [sr.runs(*sr.TABLE[n][0]) for n in names]
    ns = [sr.TABLE[n][1] for n in names]
    prms = [_c_params(sr.TABLE[n][2]) for n in names]
    together = v.test_segments(probs, ns, prms)
    for i, n in enumerate(names):
        _, N, prm, want_segs, want_len, want_pieces = sr.TABLE[n]
        segs, pcs, total = together[i]
        assert segs == want_segs, n
        assert total == want_len, n
        assert pcs == sr.pieces(want_segs, prm)[0], n
        if want_pieces is not None:
            assert pcs == want_pieces, n
        assert v.test_segments([probs[i]], [N], [prms[i]])[0] == together[i], n


# ---- 2. random inputs -----------------------------------------------------------------
def test_random_inputs_equal_restatement(vad):
    v = vad["ctx"]
    rng = np.random.default_rng(2024)
    cases = [sr.random_case(rng) for _ in range(300)]
    assert sum(1 for _, N, _ in cases if N % 512) in range(100, 201)
    assert sum(1 for _, _, prm in cases if prm.max_speech_duration_s < 100) >= 50
    n_segments = 0
    i = 0
    while i < len(cases):
        batch = cases[i:i + int(rng.integers(1, 33))]
        i += len(batch)
        got = v.test_segments([c[0] for c in batch], [c[1] for c in batch],
                              [_c_params(c[2]) for c in batch])
        for (p, N, prm), g in zip(batch, got):
            want = _expect(p, N, prm)
            assert g == want, (prm, N, p.tolist())
            n_segments += len(want[0])
    assert n_segments >= 300  # the inputs do produce segments
    # a 10-minute clip: 18 750 chunks, 293 steps of 64
    p, N, _ = sr.random_case(rng, n_chunks=18750)
    for prm in (sr.Params(), sr.Params(threshold=0.6, max_speech_duration_s=2.5, speech_pad_ms=200)):
        want = _expect(p, N, prm)
        assert len(want[0]) > 50
        assert v.test_segments([p], [N], [_c_params(prm)])[0] == want


def test_invalid_parameters_are_refused(vad):
    v = vad["ctx"]
    v.detect(vad["clips"]["zeros"])
    L = mwx.lib()
    for bad in (dict(threshold=0.0), dict(threshold=1.0), dict(threshold=float("nan")),
                dict(min_speech_duration_ms=-1), dict(min_silence_duration_ms=-1),
                dict(speech_pad_ms=-1), dict(max_speech_duration_s=0.0),
                dict(max_speech_duration_s=float("nan")), dict(samples_overlap=-0.1),
                dict(samples_overlap=float("nan"))):
        prm = mwx.vad_params(**bad)
        assert not L.mwx_vad_segments_from_probs(v.vctx, prm), bad
        ptrs = (C.c_void_p * 1)(vad["clips"]["zeros"].ctypes.data)
        lens = (C.c_int * 1)(20000)
        assert not L.mwx_vad_trim_batch(v.vctx, prm, ptrs, lens, 1), bad
        with pytest.raises(RuntimeError):
            v.test_segments([np.zeros(2, np.float32)], [1024], [prm])


# ---- 3. from_samples / from_probs -----------------------------------------------------
@pytest.mark.parametrize("name,thr,n_seg,cover", [("mixed", 0.76, 2, 0.61), ("two", 0.80, 2, 0.33),
                                                   ("two", 0.74, 3, 0.42)])
def test_segments_from_samples_and_probs(vad, name, thr, n_seg, cover):
    v = vad["ctx"]
    x, p = vad["clips"][name], vad["probs"][name]
    prm = sr.Params(threshold=thr)
    t32, n32 = np.float32(thr), sr.derived(prm)[1]
    # power: no probability is near either threshold, and the clip is cut as stated
    assert np.min(np.abs(p - t32)) > 1e-3 and np.min(np.abs(p - n32)) > 1e-3
    want = sr.segments(p, len(x), prm)
    print(name, thr, want)
    assert len(want) == n_seg
    assert round(sum(e - s for s, e in want) / len(x), 2) == cover
    want_cs = [(np.float32(s) / np.float32(160.0), np.float32(e) / np.float32(160.0))
               for s, e in want]
    assert v.segments_from_samples(x, _c_params(prm)) == want_cs
    assert v.detect(x).tobytes() == p.tobytes()
    assert v.segments_from_probs(_c_params(prm)) == want_cs
    # other parameters over the same probabilities, without another VAD pass
    prm2 = sr.Params(threshold=thr, speech_pad_ms=100, min_silence_duration_ms=300)
    want2 = sr.segments(p, len(x), prm2)
    assert [(int(round(a * 160)), int(round(b * 160)))
            for a, b in v.segments_from_probs(_c_params(prm2))] == want2


# ---- 4. compaction --------------------------------------------------------------------
TRIM_PARAMS = [sr.Params(threshold=0.76), sr.Params(threshold=0.76, max_speech_duration_s=1.0),
               sr.Params(threshold=0.80, samples_overlap=0.0, speech_pad_ms=0)]


@pytest.mark.parametrize("prm", TRIM_PARAMS, ids=["default", "max1s", "nopad"])
def test_compaction_bitwise(vad, make_model, prm):
    v = vad["ctx"]
    names = ["mixed", "two", "empty", "zeros", "noise", "mixed"]
    clips = dict(vad["clips"], empty=np.empty(0, np.float32))
    probs = dict(vad["probs"], empty=np.empty(0, np.float32))
    want = {}
    for n in set(names):
        segs, pcs, total = _expect(probs[n], len(clips[n]), prm)
        want[n] = (segs, total, sr.compact(clips[n], pcs, total), pcs)
    assert want["zeros"][0] == [] and want["empty"][1] == 0
    assert any(len(want[n][0]) > 1 for n in names)
    if prm.max_speech_duration_s == 1.0:  # adjacent pieces: no zeros between them
        assert any(a[0] + a[1] == b[0] and a[2] + a[1] == b[2]
                   for n in names for a, b in zip(want[n][3], want[n][3][1:]))
    else:                                 # a gap of zeros inside a compacted clip
        assert any(a[2] + a[1] + sr.GAP == b[2] for n in names
                   for a, b in zip(want[n][3], want[n][3][1:]))

    def check(t, order):
        assert len(t) == len(order)
        for i, n in enumerate(order):
            assert t.segments(i) == want[n][0], n
            assert t.n_samples(i) == want[n][1], n
            assert t.pcm(i).tobytes() == want[n][2].tobytes(), n

    cp = _c_params(prm)
    with v.trim_batch([clips[n] for n in names], cp) as t:  # host clips
        check(t, names)
    for n in ("mixed", "empty", "zeros"):                   # single calls
        with v.trim_batch([clips[n]], cp) as t:
            check(t, [n])
    with mwx.Context.open(make_model("micro", mwx.GGML_F16)) as ctx:
        dev = {n: ctx.upload(clips[n]) for n in ("mixed", "two", "noise")}
        try:
            with v.trim_batch([dev["mixed"], dev["two"], dev["noise"]], cp) as t:  # device clips
                check(t, ["mixed", "two", "noise"])
            with v.trim_batch([clips["two"], dev["mixed"], clips["zeros"], dev["noise"],
                               clips["empty"]], cp) as t:                          # a mix
                check(t, ["two", "mixed", "zeros", "noise", "empty"])
                pcs = want["mixed"][3]
                for tc in range(0, want["mixed"][1] // 160 + 2):
                    for is_end in (False, True):
                        assert t.map_time(1, tc, is_end) == sr.map_time(pcs, tc, is_end)
                assert t.map_time(1, -1, False) == -1
        finally:
            for b in dev.values():
                b.free()


# ---- 5. trimmed transcription ---------------------------------------------------------
def _records(ctx, state):
    return [(s.t0, s.t1, s.text, [(t.id, t.p, t.plog, t.t0, t.t1) for t in s.tokens])
            for s in ctx.segments(state)]


def test_trimmed_transcription(vad, make_model):
    v = vad["ctx"]
    prm = sr.Params(threshold=0.76)
    names = ["mixed", "zeros", "two"]
    clips = [vad["clips"][n] for n in names]
    with mwx.Context.open(make_model("micro-rich", mwx.GGML_F16)) as ctx:
        p = ctx.default_params(mwx.SAMPLING_GREEDY)
        p.language = b"en"
        p.temperature = 0.0
        p.temperature_inc = 0.0
        p.token_timestamps = True
        with v.trim_batch(clips, _c_params(prm)) as t:
            assert ctx.full_batch_trimmed([t] * 3, [0, 1, 2], p) == 0
            got = [_records(ctx, i) for i in range(3)]
            pieces = [sr.pieces(t.segments(i), prm)[0] for i in range(3)]
            compacted = [t.pcm(i) for i in range(3)]
            # one single-clip object per entry, as the request batcher passes them
            with v.trim_batch([clips[2]], _c_params(prm)) as t2:
                assert ctx.full_batch_trimmed([t2, t], [0, 0], p, state0=3) == 0
                assert _records(ctx, 3) == got[2] and _records(ctx, 4) == got[0]
            assert ctx.full_batch_trimmed([t], [3], p) != 0  # no such clip
        assert got[1] == [] and pieces[1] == []
        run = [0, 2]
        assert ctx.full_batch_states([compacted[i] for i in run], p, [5, 6]) == 0
        n_moved = n_token_times = 0
        for i, st in zip(run, (5, 6)):
            plain = _records(ctx, st)
            assert len(plain) > 0
            want = []
            for t0, t1, text, toks in plain:
                m0, m1 = sr.map_time(pieces[i], t0, False), sr.map_time(pieces[i], t1, True)
                mt = [(tid, pr, pl, sr.map_time(pieces[i], a, False),
                       sr.map_time(pieces[i], b, True)) for tid, pr, pl, a, b in toks]
                n_moved += (m0 != t0) + (m1 != t1) + sum(
                    (x[3] != y[3]) + (x[4] != y[4]) for x, y in zip(mt, toks))
                n_token_times += sum(x[3] >= 0 for x in toks)
                want.append((m0, m1, text, mt))
            assert got[i] == want, names[i]
        print(f"times moved by the map: {n_moved}, tokens with t0 >= 0: {n_token_times}")
        assert n_moved > 0 and n_token_times > 0


# ---- 6. the host engine ---------------------------------------------------------------
def _stt():
    L = C.CDLL(STT_LIB)
    ctor = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int,
            C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_float]
    L.mwx_stt_new_vad.restype = C.c_void_p
    L.mwx_stt_new_vad.argtypes = ctor
    L.mwx_stt_new_vad_trim.restype = C.c_void_p
    L.mwx_stt_new_vad_trim.argtypes = ctor + [C.c_int]
    L.mwx_stt_free.argtypes = [C.c_void_p]
    fp = C.POINTER(C.c_float)
    L.mwx_stt_transcribe_f32_ex.argtypes = [C.c_void_p, fp, C.c_int, C.c_int, C.c_char_p, C.c_int,
                                            C.c_float, C.c_char_p, C.c_int, C.POINTER(C.c_double),
                                            C.c_int, C.POINTER(C.c_int)]
    L.mwx_stt_transcribe_batch_f32.argtypes = [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int),
                                               C.c_int, C.c_char_p, C.c_int, C.c_float, C.c_char_p,
                                               C.c_int]
    L.mwx_stt_cluster_ids.argtypes = [fp, C.c_int, C.c_float, C.c_char_p, C.c_int]
    return L


def _one(L, eng, x):
    cap = 1 << 20
    buf = C.create_string_buffer(cap)
    r = L.mwx_stt_transcribe_f32_ex(eng, mwx.fptr(x), len(x), 16000, b"en", 1, -1.0, buf, cap,
                                    None, -1, None)
    assert r >= 0, r
    return json.loads(buf.value.decode())


def _batch(L, eng, xs):
    cap = 1 << 20
    buf = C.create_string_buffer(cap)
    ptrs = (C.POINTER(C.c_float) * len(xs))(*[mwx.fptr(x) for x in xs])
    lens = (C.c_int * len(xs))(*[len(x) for x in xs])
    r = L.mwx_stt_transcribe_batch_f32(eng, ptrs, lens, len(xs), b"en", 1, -1.0, buf, cap)
    assert r >= 0, r
    return json.loads(buf.value.decode())


def _f32(x):
    """A float as it comes back from the engine's JSON (printed with %.9g)."""
    return float("%.9g" % float(np.float32(x)))


def _expected_json(L, ctx, plain, pieces, x):
    """The engine's result for clip x decoded from its compacted audio: `plain`
    (an untrimmed engine's result for that audio) with every time mapped, and
    prosody / speakers recomputed over the original PCM at the mapped times."""
    out = []
    starts, lens = [], []
    for r in plain:
        r = json.loads(json.dumps(r))
        r["t0"], r["t1"] = sr.map_time(pieces, r["t0"], False), sr.map_time(pieces, r["t1"], True)
        for tk in r["tokens"]:
            tk["t0"] = sr.map_time(pieces, tk["t0"], False)
            tk["t1"] = sr.map_time(pieces, tk["t1"], True)
        s0 = max(0, min(int(r["t0"] / 100.0 * 16000.0), len(x)))
        s1 = max(s0, min(int(r["t1"] / 100.0 * 16000.0), len(x)))
        starts.append(s0)
        lens.append(s1 - s0)
        out.append(r)
    if not out:
        return out
    pros = ctx.prosody_batch(x, starts, lens)
    vecs = np.array([list(p.speaker_vec) for p in pros], np.float32)
    buf = C.create_string_buffer(1 << 16)
    for r, p in zip(out, pros):
        r["gender"], r["emotion"] = p.gender_proxy, p.emotion_proxy
        for k in ("arousal", "valence", "pitch_mean", "pitch_std", "energy_mean", "energy_std",
                  "spectral_centroid", "zero_crossing_rate"):
            r[k] = _f32(getattr(p, k))
        r["speaker_vec"] = [_f32(a) for a in p.speaker_vec]
    # speakers: clustered in order over the segments of at least 160 samples
    long = [i for i, ln in enumerate(lens) if ln >= 160]
    if long:
        lv = np.ascontiguousarray(vecs[long])
        assert L.mwx_stt_cluster_ids(mwx.fptr(lv), len(long), 0.88, buf, 1 << 16) >= 0
        ids = buf.value.decode().split("\n")
        for i, sid in zip(long, ids):
            out[i]["speaker"] = sid
    for i, ln in enumerate(lens):
        if ln < 160:
            out[i]["speaker"] = "?"
    return out


def _is_empty_result(res, n):
    assert len(res) == 1
    r = res[0]
    assert r["text"] == "" and bytes.fromhex(r["language"]) == b"unknown"
    assert r["prob"] == 0 and r["t0"] == 0 and r["t1"] == n // 16
    assert r["tokens"] == [] and r["n"] == 0 and r["speaker"] == "unknown"


def test_host_vad_trim(vad):
    d = vad["dir"]
    model = os.path.join(d, "ggml-micro.bin")
    mwx.write_synthetic_model(model, "micro-rich", mwx.GGML_F16, 0)
    thr = 0.76
    prm = sr.Params(threshold=thr)
    mixed, two, zeros = (vad["clips"][n] for n in ("mixed", "two", "zeros"))
    exp = {}
    for n in ("mixed", "two"):
        _, pcs, total = _expect(vad["probs"][n], len(vad["clips"][n]), prm)
        exp[n] = (pcs, sr.compact(vad["clips"][n], pcs, total))
    L = _stt()

    def new(ctor, enable, vad_file, *more, max_batch=1):
        eng = ctor(d.encode(), b"ggml-micro.bin", 2, 5000, 1, b"en", 500, 0, max_batch, 2000, 8000,
                   int(enable), vad_file, thr, *more)
        assert eng
        engines.append(eng)
        return eng

    engines = []
    try:
        off = new(L.mwx_stt_new_vad, False, b"ggml-silero-vad.bin")
        gate = new(L.mwx_stt_new_vad, True, b"ggml-silero-vad.bin")
        trim = new(L.mwx_stt_new_vad_trim, True, b"ggml-silero-vad.bin", 1)
        trim_q = new(L.mwx_stt_new_vad_trim, True, b"ggml-silero-vad.bin", 1, max_batch=2)
        no_trim = new(L.mwx_stt_new_vad_trim, True, b"ggml-silero-vad.bin", 0)
        missing = new(L.mwx_stt_new_vad_trim, True, b"no-such-vad.bin", 1)
        no_vad = new(L.mwx_stt_new_vad_trim, False, b"ggml-silero-vad.bin", 1)
        with mwx.Context.open(model) as ctx:
            want = {n: _expected_json(L, ctx, _one(L, off, exp[n][1]), exp[n][0], vad["clips"][n])
                    for n in ("mixed", "two")}
        assert all(len(w) > 0 for w in want.values())
        untrimmed = {n: _one(L, off, vad["clips"][n]) for n in ("mixed", "two", "zeros")}
        assert any(want[n] != untrimmed[n] for n in want)
        # transcribe(): direct, and through the request batcher
        for eng in (trim, trim_q):
            assert _one(L, eng, mixed) == want["mixed"]
            assert _one(L, eng, two) == want["two"]
            _is_empty_result(_one(L, eng, zeros), len(zeros))
        # transcribe_batch(): the zero-segment clip is held back, a short clip has no result
        short = vr.noise_clip(4000, seed=4)
        got = _batch(L, trim, [mixed, zeros, short, two])
        assert got[0] == want["mixed"] and got[3] == want["two"] and got[2] == []
        _is_empty_result(got[1], len(zeros))
        # vad_trim off: the gate of the parent
        for n in ("mixed", "two"):
            assert _one(L, no_trim, vad["clips"][n]) == _one(L, gate, vad["clips"][n]) \
                == untrimmed[n]
        _is_empty_result(_one(L, no_trim, zeros), len(zeros))
        assert _batch(L, no_trim, [mixed, zeros, two]) == _batch(L, gate, [mixed, zeros, two])
        # no VAD model, or VAD off: everything untrimmed
        for eng in (missing, no_vad):
            for n in ("mixed", "zeros"):
                assert _one(L, eng, vad["clips"][n]) == untrimmed[n]
    finally:
        for e in engines:
            L.mwx_stt_free(e)
