"""The host SttEngine's chunked-transcription plumbing on the CPU: tests/vad_chunk/
host_chunk_check.cpp drives the engine over CPU stand-ins (Whisper, VAD, the
trimming and the chunked calls) from several threads, with the request batcher
on and off, built with AddressSanitizer + UBSan as stand-alone programs and run
as child processes; once with the chunked calls present and once linked without
them (the path is then vad_trim's)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "vad_chunk")


@pytest.mark.parametrize("prog", ["host_chunk_check", "host_chunk_fallback"])
def test_host_vad_chunk_under_asan_ubsan(tmp_path, prog):
    subprocess.check_call(["make", "-s", "-C", DIR, f"_build/{prog}"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([os.path.join(DIR, "_build", prog), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "host_chunk_check: 0 failure(s)" in r.stdout


def test_chunked_calls_are_bound_weakly():
    subprocess.check_call(["make", "-s", "-C", DIR, "_build/host_chunk_fallback"])
    out = subprocess.check_output(["nm", os.path.join(DIR, "_build", "host_chunk_fallback")],
                                  text=True)
    names = ("mwx_vad_trim_batch_chunked", "mwx_vad_trimmed_n_chunks", "mwx_full_batch_chunked")
    for n in names:
        lines = [l for l in out.splitlines() if l.split()[-1] == n]
        assert lines and all(l.split()[-2] == "w" for l in lines), (n, lines)
