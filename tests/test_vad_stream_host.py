"""The host side of streaming VAD on the CPU (Settings::stream_vad and
stream_endpoint_silence_ms, StreamSession): tests/vad_stream/
host_stream_check.cpp drives the engine and its sessions over CPU stand-ins
(Whisper, VAD, the stream calls), also from several threads, built with
AddressSanitizer + UBSan as stand-alone programs and run as child processes;
once with the stream calls present and once linked without them (both settings
are then inert and the events are today's)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "vad_stream")


@pytest.mark.parametrize("prog", ["host_stream_check", "host_stream_fallback"])
def test_host_vad_stream_under_asan_ubsan(tmp_path, prog):
    subprocess.check_call(["make", "-s", "-C", DIR, f"_build/{prog}"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([os.path.join(DIR, "_build", prog), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "host_stream_check: 0 failure(s)" in r.stdout


def test_stream_calls_are_bound_weakly():
    subprocess.check_call(["make", "-s", "-C", DIR, "_build/host_stream_fallback"])
    out = subprocess.check_output(["nm", os.path.join(DIR, "_build", "host_stream_fallback")],
                                  text=True)
    names = ("mwx_vad_stream_init", "mwx_vad_stream_free", "mwx_vad_stream_reset",
             "mwx_vad_stream_feed_batch", "mwx_vad_stream_n_probs", "mwx_vad_stream_probs",
             "mwx_vad_stream_max_prob", "mwx_vad_stream_n_segments", "mwx_vad_stream_segment")
    for n in names:
        lines = [l for l in out.splitlines() if l.split()[-1] == n]
        assert lines and all(l.split()[-2] == "w" for l in lines), (n, lines)
