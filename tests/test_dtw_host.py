"""The host SttEngine's DTW token times on the CPU: tests/dtw/host_dtw_check.cpp
drives the engine over a CPU stand-in that reports t_dtw, built with
AddressSanitizer + UBSan as a stand-alone program and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "dtw")


def test_host_dtw_token_times_under_asan_ubsan(tmp_path):
    subprocess.check_call(["make", "-s", "-C", DIR, "_build/host_dtw_check"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    for k in [k for k in env if k.startswith("STT_WHISPER_SERVICE_DTW_")]:
        del env[k]
    r = subprocess.run([os.path.join(DIR, "_build", "host_dtw_check"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "host_dtw_check: 0 failure(s)" in r.stdout
