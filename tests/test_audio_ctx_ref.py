"""Audio context (mwx_full_params.audio_ctx / audio_ctx_fit) on
the CPU: the reference construction of tests/audio_ctx_ref.py is sound, the
exported context rule equals its restatement, and the host SttEngine carries
the two settings into the params of every request path."""
import os
import subprocess

import numpy as np

import mwx
import orc
from audio_ctx_ref import CtxOracles, audio_ctx_rule, rewrite_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "audio_ctx")


def _pcm(k, seconds):
    return mwx.pcm16_to_f32(mwx.synth_pcm16(k, int(seconds * 16000)))


def _records(segs):
    return [(s.t0, s.t1, s.raw, [(t.id, t.tid, t.p, t.plog, t.pt, t.ptsum, t.t0, t.t1)
                                 for t in s.tokens]) for s in segs]


def test_full_external_with_the_model_itself_is_full(make_model, tmp_path):
    """M' = M (K = n_audio_ctx): the pipeline reference wired as for a short
    context (every encode and every logits row answered through the
    callbacks) returns exactly Oracle(M).full: greedy over two windows, beam
    search over one."""
    path = make_model("micro-rich")
    refs = CtxOracles(path, str(tmp_path))
    for beam, seconds, n_win in ((1, 31.0, 2), (5, 2.5, 1)):
        pcm = _pcm(3, seconds)
        opt = orc.FullOptions.service_defaults(beam_size=beam)
        opt.language = "en"
        opt.temperature_inc = 0.0
        want = refs.base.full(pcm, opt)
        got, windows = refs.full(pcm, opt, audio_ctx=refs.N if beam == 1 else 0)
        assert got[0] == want[0] == 0
        assert _records(got[1]) == _records(want[1])
        assert got[2:] == want[2:]
        assert len(want[3]) == n_win and [k for _, k in windows] == [refs.N] * n_win


def test_rewritten_model_is_the_model_with_a_short_context(make_model, tmp_path):
    """M' differs from M in n_audio_ctx and the positional embedding's rows
    only; its oracle's stem reads the first 2 K frames (zeros past them)."""
    path = make_model("micro")
    o = orc.Oracle(path)
    K = 100
    ok = orc.Oracle(rewrite_model(path, str(tmp_path / "m100.bin"), K))
    assert ok.hp[1] == K and ok.hp[:1] + ok.hp[2:] == o.hp[:1] + o.hp[2:]
    pe, pek = o.tensor("encoder.positional_embedding"), ok.tensor("encoder.positional_embedding")
    assert np.array_equal(pek, pe[:K * o.d])
    for name in ("encoder.conv1.weight", "decoder.token_embedding.weight", "decoder.ln.bias"):
        assert np.array_equal(o.tensor(name), ok.tensor(name))
    mel, _ = o.mel(_pcm(1, 4.0))
    cut = mel.copy()
    cut[:, 2 * K:] = 0.0
    x, xc = ok.encode_stem(mel), ok.encode_stem(cut)
    assert x.shape == (K, o.d) and np.array_equal(x, xc)
    # the stem's rows away from the cut are the full model's rows (same frames,
    # same positional rows): the conv padding only reaches the last row
    assert np.array_equal(x[:K - 1], o.encode_stem(mel)[:K - 1])


def test_audio_ctx_for_equals_the_rule():
    """mwx_audio_ctx_for over the grid of clip lengths, seeks, floors and both
    modes (a host function: no context needed, N = 1500)."""
    L = mwx.lib()
    N = 1500
    lens = [0, 1, 159, 160] + [int(16000 * s) for s in (0.5, 3, 10.23, 29, 30, 31, 65)]
    seen = set()
    for n in lens:
        for seek in (0, 1500, 3000):
            for floor in (0, 64, 100, 1500):
                for fit in (False, True):
                    got = L.mwx_audio_ctx_for(None, n, seek, floor, fit)
                    want = audio_ctx_rule(N, n, seek, floor, fit)
                    assert got == want, (n, seek, floor, fit, got, want)
                    assert 1 <= got <= N and (not fit or got % 64 == 0 or got in (N, floor))
                    if fit and floor == 0:
                        seen.add(got)
    assert {64, 128, 192, 576, 1500} <= seen, sorted(seen)
    # fit, no floor: 0.64 s of trailing context, rounded up to the key tile
    assert L.mwx_audio_ctx_for(None, 3 * 16000, 0, 0, True) == 192     # 150 + 32 -> 192
    assert L.mwx_audio_ctx_for(None, 16000, 0, 0, True) == 128         # 50 + 32 -> 128
    assert L.mwx_audio_ctx_for(None, 41 * 16000, 3000, 0, True) == 640  # 1100 frames left
    assert L.mwx_audio_ctx_for(None, 16000, 0, 1501, False) == -1
    assert L.mwx_audio_ctx_for(None, 16000, 0, -7, False) == N         # negative: as 0


def test_host_settings_reach_every_request_path(tmp_path):
    """tests/audio_ctx/host_ctx_check.cpp: a stand-alone program over the CPU
    stand-ins (built with AddressSanitizer + UBSan, run as a child process)."""
    subprocess.check_call(["make", "-s", "-C", DIR, "_build/host_ctx_check"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([os.path.join(DIR, "_build", "host_ctx_check"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "host_ctx_check: 0 failure(s)" in r.stdout
