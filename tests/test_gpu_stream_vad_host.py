"""Streaming VAD in the host's stream sessions on the GPU (Settings::stream_vad,
Settings::stream_endpoint_silence_ms; host/stt_stream.h).

(a) With stream_vad the session's gate decisions come from its VAD stream:
    every event equals that of an identically configured engine that runs the
    whole-buffer gate, and the whole-buffer gate no longer runs.
(b) With endpointing the events equal a Python restatement of the rule, driven
    by a second engine (the transcriptions), VadContext.detect (the
    probabilities of the buffer) and the online scan of
    tests/vad_stream_restatement.py (the cuts).
"""
import ctypes as C

import numpy as np
import pytest

import mwx
import vad_segments_restatement as sr
import vad_stream_restatement as st
from test_stt_engine import _transcribe
from test_stt_stream import MAX, STEP, check, feed, lib as stream_lib

pytestmark = pytest.mark.gpu

SEED = 3     # the VAD model of test_gpu_vad.py
# The seeded net answers digital silence with about 0.68 and noise with values
# between 0.4 and 0.95: at this threshold silence is below threshold - 0.15 and
# noise crosses the threshold now and then.
THR = 0.84
S_MS = 300   # the endpoint's silence


def lib():
    L = stream_lib()
    L.mwx_stt_new_stream_vad.restype = C.c_void_p
    L.mwx_stt_new_stream_vad.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int,
                                         C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_char_p, C.c_float, C.c_int, C.c_int, C.c_int]
    L.mwx_stt_vad_gate_runs.restype = C.c_long
    L.mwx_stt_vad_gate_runs.argtypes = [C.c_void_p]
    L.mwx_stt_stream_vad_active.restype = C.c_int
    L.mwx_stt_stream_vad_active.argtypes = [C.c_void_p]
    return L


def bursts(seed, n, spans):
    """int16 digital silence with 0.3-amplitude Gaussian noise in `spans`."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, np.int16)
    for a, b in spans:
        x[a:b] = np.clip(0.3 * 32768 * rng.standard_normal(b - a), -32768, 32767).astype(np.int16)
    return x


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("streamvad")
    mwx.write_synthetic_model(str(d / "ggml-micro.bin"), "micro-rich", mwx.GGML_F16, 0)
    mwx.write_synthetic_vad_model(str(d / "ggml-silero-vad.bin"), SEED)
    return str(d)


def engine(L, d, stream_vad, endpoint_ms):
    e = L.mwx_stt_new_stream_vad(d.encode(), b"ggml-micro.bin", 1, 20000, 1, b"en", 500, 0, 1, 2000,
                                 STEP, 1, b"ggml-silero-vad.bin", THR, 0, int(stream_vad),
                                 endpoint_ms)
    assert e
    return e


def session(L, eng, chunks):
    s = L.mwx_stt_stream_new(eng)
    try:
        return [feed(L, s, ch) for ch in chunks]
    finally:
        L.mwx_stt_stream_free(s)


def cadence(x, step=STEP):
    raw = x.tobytes()
    return [raw[i:i + 2 * step] for i in range(0, len(raw), 2 * step)]


def test_stream_vad_gate_equals_whole_buffer_gate(models):
    L = lib()
    # 1.5 s of zeros, then noise bursts
    x = bursts(41, 7 * 16000, [(24000, 56000), (80000, 100000)])
    chunks = cadence(x) + [b""] + cadence(x[:2 * 16000]) + [b""]  # then a silent buffer
    old, new = engine(L, models, False, 0), engine(L, models, True, 0)
    try:
        assert L.mwx_stt_stream_vad_active(old) == 0 and L.mwx_stt_stream_vad_active(new) == 1
        want = session(L, old, chunks)
        got = session(L, new, chunks)
        runs_old, runs_new = L.mwx_stt_vad_gate_runs(old), L.mwx_stt_vad_gate_runs(new)
    finally:
        L.mwx_stt_free(old)
        L.mwx_stt_free(new)
    assert got == want
    assert runs_new == 0 and runs_old > 0
    # power: the gate was closed on a partial and open on one. The zeros of the
    # first three partials and of the second buffer stay below the threshold
    # (no event: the gate's empty result has no text); later partials have text.
    with mwx.VadContext(models + "/ggml-silero-vad.bin") as v:
        f = x.astype(np.float32) / np.float32(32768.0)
        assert v.detect(f[:3 * STEP]).max() < np.float32(THR) <= v.detect(f[:9 * STEP]).max()
        assert v.detect(f[:2 * 16000]).max() < np.float32(THR)
    n = len(cadence(x))
    assert want[0] == want[1] == want[2] == [] and all(e == [] for e in want[n + 1:])
    assert any(e and not e[0]["final"] for e in want[3:n])
    assert want[n] and all(e["final"] for e in want[n])


def expected_endpoint_events(L, eng, vad, chunks, prm):
    """The session of stt_stream.h with stream_endpoint_silence_ms restated:
    `eng` transcribes (its whole-buffer gate is rule D6, which the session's
    stream reproduces), `vad` gives the probabilities of the buffer, the online
    scan the raw segments. Returns (events per chunk, cuts [(cut, remainder)])."""
    buf = np.zeros(0, np.int16)
    last = 0
    per_chunk, cuts = [], []

    def finals(pcm):
        _, res, _ = _transcribe(L, eng, pcm, lang=b"", beam=-1, temp=-1.0)
        return [("final", bytes.fromhex(r["text"]), r,
                 [(bytes.fromhex(w["text"]), np.float32(w["t0"]) / np.float32(100),
                   np.float32(w["t1"]) / np.float32(100), w["p"]) for w in r["tokens"]])
                for r in res if bytes.fromhex(r["text"])]

    for ch in chunks:
        evs = []
        if len(ch) == 0:
            if len(buf):
                evs += finals(buf)
                buf = np.zeros(0, np.int16)
                last = 0
            per_chunk.append(evs)
            continue
        buf = np.concatenate([buf, np.frombuffer(ch, np.int16)])
        while True:
            p = vad.detect(buf.astype(np.float32) / np.float32(32768.0))
            scan = st.OnlineScan(prm)
            scan.feed(p[:len(buf) // 512])  # the scan does not see a partial chunk
            if not scan.closed:
                break
            cut = scan.closed[-1][2]
            evs += finals(buf[:cut])
            buf = buf[cut:]
            last = 0
            cuts.append((cut, len(buf)))
        if len(buf) - last >= STEP:
            _, res, _ = _transcribe(L, eng, buf, lang=b"", beam=-1, temp=-1.0)
            last = len(buf)
            texts = [r for r in res if bytes.fromhex(r["text"])]
            if texts:
                evs.append(("partial", b"".join(bytes.fromhex(r["text"]) + b" " for r in texts),
                            texts[-1], None))
            if len(buf) > MAX:
                evs += [("forced", bytes.fromhex(r["text"]), r, None) for r in texts]
                buf = np.zeros(0, np.int16)
                last = 0
        per_chunk.append(evs)
    return per_chunk, cuts


@pytest.mark.parametrize("stream_vad", [True, False], ids=["stream-gate", "buffer-gate"])
def test_endpointing_equals_restatement(models, stream_vad):
    L = lib()
    # two bursts 1.5 s apart (S + 1.2 s), then 1 s of silence, then the empty chunk
    x = bursts(43, 6 * 16000 + 500, [(8000, 36000), (60000, 80000)])
    chunks = cadence(x) + [b""]
    prm = sr.Params(threshold=THR, min_silence_duration_ms=S_MS)
    ref, eng = engine(L, models, False, 0), engine(L, models, stream_vad, S_MS)
    try:
        assert L.mwx_stt_stream_vad_active(eng) == (3 if stream_vad else 2)
        with mwx.VadContext(models + "/ggml-silero-vad.bin") as v:
            want, cuts = expected_endpoint_events(L, ref, v, chunks, prm)
        got = session(L, eng, chunks)
        runs = L.mwx_stt_vad_gate_runs(eng)
    finally:
        L.mwx_stt_free(ref)
        L.mwx_stt_free(eng)
    print("cuts (cut, remainder):", cuts)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        check(g, w)
    assert (runs == 0) == stream_vad
    # power: an endpoint final before the empty chunk, and a cut with a remainder
    assert any(kind == "final" for evs in want[:-1] for (kind, *_r) in evs)
    assert cuts and any(rem > 0 for _, rem in cuts)
