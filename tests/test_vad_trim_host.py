"""The host SttEngine's vad_trim plumbing on the CPU: tests/vad_trim/
host_trim_check.cpp drives the engine over CPU stand-ins (Whisper, VAD and the
trimming calls) from several threads, built with AddressSanitizer + UBSan as
stand-alone programs and run as child processes; once with the trimming calls
present and once linked without them (vad_trim then falls back to the gate)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "vad_trim")


@pytest.mark.parametrize("prog", ["host_trim_check", "host_trim_fallback"])
def test_host_vad_trim_under_asan_ubsan(tmp_path, prog):
    subprocess.check_call(["make", "-s", "-C", DIR, f"_build/{prog}"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([os.path.join(DIR, "_build", prog), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "host_trim_check: 0 failure(s)" in r.stdout


def test_trimming_calls_are_bound_weakly():
    subprocess.check_call(["make", "-s", "-C", DIR, "_build/host_trim_fallback"])
    out = subprocess.check_output(["nm", os.path.join(DIR, "_build", "host_trim_fallback")],
                                  text=True)
    names = ("mwx_vad_default_params", "mwx_vad_trim_batch", "mwx_vad_trimmed_n_segments",
             "mwx_vad_trimmed_free", "mwx_full_batch_trimmed")
    for n in names:
        lines = [l for l in out.splitlines() if l.split()[-1] == n]
        assert lines and all(l.split()[-2] == "w" for l in lines), (n, lines)
