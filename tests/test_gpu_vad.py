"""GPU voice-activity detection (csrc/k_vad.hip, mwx_vad_*) against the numpy
restatement of the network (tests/vad_restatement.py), and the host SttEngine's
VAD gate over the real engine.

Parity bound: max |p_dev - p_f64| <= 16 * e32, where e32 is the distance of the
f32 restatement from the f64 one on the same clip (the largest e32 of the clips
where a clip's own is zero), and < 1e-4 in any case. The device differs from
the f32 restatement only in summation order and in its expf / tanhf, f32
rounding sequences of the same length; an indexing, padding or gate-order
mistake moves the probabilities of this net (span >= 0.3,
test_vad_format.py) by >= 1e-2.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mwx
import vad_restatement as vr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STT_LIB = os.path.join(ROOT, "sentiric-stt-whisper-service_amd", "libmwx_stt.so")
SEED = 3  # as test_vad_format.py: power condition and gate gap hold
EDGE = [0, 1, 511, 512, 513, 7 * 512 + 137]
FACTOR = 16.0


def _clips():
    c = {f"n{n}": vr.noise_clip(n, seed=100 + n) for n in EDGE}
    c["mixed"] = vr.mixed_clip()
    c["window"] = vr.window_clip()
    return c


@pytest.fixture(scope="module")
def vad(tmp_path_factory):
    """(path, VadContext, clips, f64 probabilities, e32 per clip, largest e32)"""
    d = tmp_path_factory.mktemp("vadgpu")
    path = str(d / "ggml-silero-vad.bin")
    mwx.write_synthetic_vad_model(path, SEED)
    model = vr.load(path)
    clips = _clips()
    p64 = {k: vr.forward(model, x, np.float64) for k, x in clips.items()}
    e32 = {}
    for k, x in clips.items():
        p32 = vr.forward(model, x, np.float32).astype(np.float64)
        e32[k] = float(np.max(np.abs(p32 - p64[k]))) if len(p32) else 0.0
    with mwx.VadContext(path) as v:
        yield {"path": path, "dir": str(d), "ctx": v, "clips": clips, "p64": p64, "e32": e32,
               "e32_max": max(e32.values()), "model": model}


def _check_parity(vad, name):
    x = vad["clips"][name]
    got = vad["ctx"].detect(x)
    want = vad["p64"][name]
    assert got.dtype == np.float32 and len(got) == len(want) == vr.n_chunks(len(x))
    if len(x) == 0:
        return
    e32 = vad["e32"][name] if vad["e32"][name] > 0.0 else vad["e32_max"]
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"{name}: chunks {len(got)}, err {err:.3e}, e32 {e32:.3e}, err / e32 = {err / e32:.2f}")
    assert np.all(np.isfinite(got)) and got.min() >= 0.0 and got.max() <= 1.0
    assert err < 1e-4
    assert err <= FACTOR * e32


@pytest.mark.parametrize("name", [f"n{n}" for n in EDGE] + ["mixed"])
def test_parity_edge_shapes(vad, name):
    _check_parity(vad, name)


def test_parity_full_window(vad):
    assert len(vad["clips"]["window"]) == 480000 and len(vad["p64"]["window"]) == 938
    _check_parity(vad, "window")


def test_batch_equals_single_bitwise(vad):
    v = vad["ctx"]
    clips = [np.empty(0, np.float32), vr.noise_clip(1, seed=5), vr.noise_clip(513, seed=6),
             vr.noise_clip(33 * 512, seed=7), vad["clips"]["mixed"]]
    batch = v.detect_batch(clips)
    assert [len(b) for b in batch] == [0, 1, 2, 33, 188]
    for b, x in zip(batch, clips):
        assert b.tobytes() == v.detect(x).tobytes()
    for b, r in zip(batch, reversed(v.detect_batch(clips[::-1]))):
        assert b.tobytes() == r.tobytes()
    for b, r in zip(batch, v.detect_batch(clips)):
        assert b.tobytes() == r.tobytes()
    assert v.detect_batch([]) == []


def test_state_resets_between_calls(vad):
    v = vad["ctx"]
    a, b = vad["clips"]["mixed"], vr.noise_clip(20 * 512 + 3, seed=9)
    first = v.detect(a)
    v.detect(b)
    assert v.detect(a).tobytes() == first.tobytes()


def test_device_resident_input(vad, make_model):
    v = vad["ctx"]
    x = vad["clips"]["mixed"]
    host = v.detect(x)
    with mwx.Context.open(make_model("micro", mwx.GGML_F16)) as ctx:
        buf = ctx.upload(x)
        try:
            assert v.detect(buf).tobytes() == host.tobytes()
            mixed = v.detect_batch([buf, x[:5000], buf])
            assert mixed[0].tobytes() == host.tobytes() == mixed[2].tobytes()
            assert mixed[1].tobytes() == v.detect(x[:5000]).tobytes()
        finally:
            buf.free()


# ---- the host gate over the real engine ---------------------------------------------
def _stt():
    L = C.CDLL(STT_LIB)
    L.mwx_stt_new_vad.restype = C.c_void_p
    L.mwx_stt_new_vad.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_char_p, C.c_float]
    L.mwx_stt_free.argtypes = [C.c_void_p]
    fp = C.POINTER(C.c_float)
    L.mwx_stt_transcribe_f32_ex.argtypes = [C.c_void_p, fp, C.c_int, C.c_int, C.c_char_p, C.c_int,
                                            C.c_float, C.c_char_p, C.c_int, C.POINTER(C.c_double),
                                            C.c_int, C.POINTER(C.c_int)]
    L.mwx_stt_transcribe_batch_f32.argtypes = [C.c_void_p, C.POINTER(fp), C.POINTER(C.c_int),
                                               C.c_int, C.c_char_p, C.c_int, C.c_float, C.c_char_p,
                                               C.c_int]
    return L


def _new(L, d, enable, vad_file, thr):
    eng = L.mwx_stt_new_vad(d.encode(), b"ggml-micro.bin", 2, 5000, 1, b"en", 500, 0, 1, 2000,
                            8000, int(enable), vad_file, thr)
    assert eng
    return eng


def _one(L, eng, x):
    cap = 1 << 20
    buf = C.create_string_buffer(cap)
    m = (C.c_double * 3)()
    r = L.mwx_stt_transcribe_f32_ex(eng, mwx.fptr(x), len(x), 16000, b"en", 1, -1.0, buf, cap, m,
                                    -1, None)
    assert r >= 0, r
    return json.loads(buf.value.decode()), list(m)


def _batch(L, eng, xs):
    cap = 1 << 20
    buf = C.create_string_buffer(cap)
    ptrs = (C.POINTER(C.c_float) * len(xs))(*[mwx.fptr(x) for x in xs])
    lens = (C.c_int * len(xs))(*[len(x) for x in xs])
    r = L.mwx_stt_transcribe_batch_f32(eng, ptrs, lens, len(xs), b"en", 1, -1.0, buf, cap)
    assert r >= 0, r
    return json.loads(buf.value.decode())


def _is_empty_result(res, n):
    assert len(res) == 1
    r = res[0]
    assert r["text"] == "" and bytes.fromhex(r["language"]) == b"unknown"
    assert r["prob"] == 0 and r["t0"] == 0 and r["t1"] == n // 16
    assert r["tokens"] == [] and r["n"] == 0
    assert r["speaker"] == "unknown" and r["speaker_vec"] == [0.0] * 8


def test_host_gate(vad):
    d = vad["dir"]
    mwx.write_synthetic_model(os.path.join(d, "ggml-micro.bin"), "micro-rich", mwx.GGML_F16, 0)
    silent = np.zeros(32000, np.float32)
    noise = vr.noise_clip(32000)
    p_sil = float(vr.forward(vad["model"], silent).max())
    p_noi = float(vr.forward(vad["model"], noise).max())
    print(f"max p: silence {p_sil:.4f}, noise {p_noi:.4f}")
    assert p_noi - p_sil >= 0.05
    thr = 0.5 * (p_sil + p_noi)
    L = _stt()
    engines = []
    try:
        off = _new(L, d, False, b"ggml-silero-vad.bin", thr)
        on = _new(L, d, True, b"ggml-silero-vad.bin", thr)
        missing = _new(L, d, True, b"no-such-vad.bin", thr)
        engines = [off, on, missing]
        # each engine has two states, used in turn: every clip below meets a fresh one
        ref_silent, _ = _one(L, off, silent)
        ref_noise, _ = _one(L, off, noise)
        got, metrics = _one(L, on, silent)
        _is_empty_result(got, len(silent))
        assert metrics[0] == 0.0 and metrics[1] > 0.0 and metrics[2] == 0.0
        assert _one(L, on, noise)[0] == ref_noise
        assert len(ref_noise) > 0
        # batch: the silent clip is held back, the others are as without VAD
        ref_batch = _batch(L, off, [noise, silent, noise])
        got_batch = _batch(L, on, [noise, silent, noise])
        assert len(got_batch) == 3
        _is_empty_result(got_batch[1], len(silent))
        assert got_batch[0] == ref_batch[0] and got_batch[2] == ref_batch[2]
        # a VAD model that does not load: the engine constructs, the gate is open
        assert _one(L, missing, silent)[0] == ref_silent
        assert _one(L, missing, noise)[0] == ref_noise
    finally:
        for e in engines:
            L.mwx_stt_free(e)
