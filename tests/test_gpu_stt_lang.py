"""Language identification through the host SttEngine's C glue (stt_lib()):
mwx_stt_detect_language_pcm16 against Context.lang_probs on the same audio,
TranscriptionResult::language_probability after "auto" and after a fixed
language, and Settings::chunk_language_recording on the chunked path. Model
micro-ml-rich, the VAD fixtures of test_gpu_vad_chunks.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mwx
import vad_segments_restatement as sr
from test_gpu_vad_segments import SEED, _c_params, two_clip

pytestmark = pytest.mark.gpu

THR = 0.76
MODEL = "ggml-ml.bin"


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sttlang"))
    mwx.write_synthetic_model(os.path.join(d, MODEL), "micro-ml-rich", mwx.GGML_F16, 0)
    mwx.write_synthetic_vad_model(os.path.join(d, "ggml-silero-vad.bin"), SEED)
    L = mwx.stt_lib()
    ctor = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int,
            C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_float, C.c_int]
    L.mwx_stt_new_vad_trim.restype = C.c_void_p
    L.mwx_stt_new_vad_trim.argtypes = ctor
    L.mwx_stt_set_vad_chunk.argtypes = [C.c_void_p, C.c_float, C.c_int]
    L.mwx_stt_transcribe_pcm16_ex.argtypes = [C.c_void_p, C.POINTER(C.c_int16), C.c_int, C.c_int,
                                              C.c_char_p, C.c_int, C.c_float, C.c_char_p, C.c_int,
                                              C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    engines = []

    def plain(language=b"auto"):
        e = L.mwx_stt_new(d.encode(), MODEL.encode(), 1, 5000, 1, language, 500, 0)
        assert e
        engines.append(e)
        return e

    def chunked():
        e = L.mwx_stt_new_vad_trim(d.encode(), MODEL.encode(), 1, 5000, 1, b"auto", 500, 0, 1, 2000,
                                   8000, 1, b"ggml-silero-vad.bin", THR, 1)
        assert e
        engines.append(e)
        assert L.mwx_stt_set_vad_chunk(e, 1.0, 32) == 1
        return e

    yield {"dir": d, "L": L, "plain": plain, "chunked": chunked}
    for e in engines:
        L.mwx_stt_free(e)


def transcribe(L, eng, pcm16, language=b""):
    pcm16 = np.ascontiguousarray(pcm16, np.int16)
    cap = 1 << 20
    buf = C.create_string_buffer(cap)
    r = L.mwx_stt_transcribe_pcm16_ex(eng, pcm16.ctypes.data_as(C.POINTER(C.c_int16)), len(pcm16),
                                      16000, language, 1, -1.0, buf, cap, None, -1, None)
    assert r >= 0, r
    return json.loads(buf.value.decode())


def f32(x):
    """A float as it comes back from the engine's JSON (printed with %.9g)."""
    return float("%.9g" % float(np.float32(x)))


def test_detect_language_and_language_probability(env):
    L = env["L"]
    eng = env["plain"]()
    pcm16 = mwx.synth_pcm16(20, 3 * 16000)
    with mwx.Context.open(os.path.join(env["dir"], MODEL)) as ctx:
        p = ctx.default_params(mwx.SAMPLING_GREEDY)
        p.language = b"auto"
        p.detect_language = True
        assert ctx.full(mwx.pcm16_to_f32(pcm16), p) == 0
        probs = ctx.lang_probs()
        lang = ctx.lang_id()
    assert probs.shape == (100,)
    order = sorted(range(100), key=lambda i: (-float(probs[i]), i))
    for k in (3, 1, 0, 100, 250):
        got = mwx.stt_detect_language_pcm16(L, eng, pcm16, 16000, k)
        n = k if 1 <= k <= 100 else 100
        assert [c for c, _ in got] == [mwx.lang_str(i) for i in order[:n]], k
        assert [np.float32(v).view(np.uint32) for _, v in got] == \
            [probs[i].view(np.uint32) for i in order[:n]], k
    assert mwx.stt_detect_language_pcm16(L, eng, pcm16, 16000, 3)[0][0] == mwx.lang_str(lang)
    # under the engine's minimum duration (500 ms): nothing
    assert mwx.stt_detect_language_pcm16(L, eng, pcm16[:7999], 16000, 3) == []
    # language_probability: the used language's probability after "auto" ...
    res = transcribe(L, eng, pcm16)
    assert len(res) > 0
    for r in res:
        assert r["language_probability"] == f32(probs[lang])
        assert bytes.fromhex(r["language"]) == b"auto"
    # ... and -1 after a fixed language
    res = transcribe(L, eng, pcm16, b"tr")
    assert len(res) > 0
    for r in res:
        assert r["language_probability"] == -1
        assert bytes.fromhex(r["language"]) == b"tr"


def test_chunk_language_recording(env):
    L = env["L"]
    eng = env["chunked"]()
    x = two_clip()
    pcm16 = np.round(x * 32767.0).astype(np.int16)
    xf = pcm16.astype(np.float32) / np.float32(32768.0)  # what the engine decodes
    # the host's VAD parameters: its threshold, max_speech_duration_s = min(FLT_MAX, chunk_s)
    prm = sr.Params(threshold=THR, max_speech_duration_s=1.0)
    want = {}
    with mwx.VadContext(os.path.join(env["dir"], "ggml-silero-vad.bin")) as v, \
            mwx.Context.open(os.path.join(env["dir"], MODEL)) as ctx, \
            v.trim_batch([xf], _c_params(prm), chunk_s=1.0) as t:
        assert len(t.chunks(0)) >= 2
        for mode in (mwx.CHUNK_LANG_PER_CHUNK, mwx.CHUNK_LANG_RECORDING):
            p = ctx.default_params(mwx.SAMPLING_GREEDY)
            p.language = b"auto"
            p.chunk_language = mode
            assert ctx.full_batch_chunked([t], [0], p) == 0
            want[mode] = f32(ctx.lang_probs(0)[ctx.lang_id(0)])
    print("language_probability per chunk / per recording:", want)
    for mode in (mwx.CHUNK_LANG_PER_CHUNK, mwx.CHUNK_LANG_RECORDING, mwx.CHUNK_LANG_PER_CHUNK):
        assert L.mwx_stt_set_chunk_language_recording(eng, mode) == 0
        res = transcribe(L, eng, pcm16)
        assert len(res) > 0
        # one language, and one probability, for the whole recording
        assert {r["language_probability"] for r in res} == {want[mode]}, mode
    assert L.mwx_stt_set_chunk_language_recording(None, 1) == -1
