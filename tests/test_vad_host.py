"""The host SttEngine's VAD gate on the CPU: tests/vad/host_vad_check.cpp drives
the engine over the CPU stand-ins tests/san/mwx_stub.cpp and
tests/vad/vad_stub.cpp (canned probabilities) from several threads, built with
AddressSanitizer + UBSan as a stand-alone program and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAD = os.path.join(ROOT, "tests", "vad")


def test_host_vad_gate_under_asan_ubsan(tmp_path):
    subprocess.check_call(["make", "-s", "-C", VAD])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([os.path.join(VAD, "_build", "host_vad_check"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "host_vad_check: 0 failure(s)" in r.stdout


def test_san_build_links_without_vad_symbols():
    """tests/san links the host against a libmwx stand-in that has no mwx_vad_*
    symbols: the host binds them weakly."""
    san = os.path.join(ROOT, "tests", "san")
    subprocess.check_call(["make", "-s", "-C", san, "_build/host_asan"])
    out = subprocess.check_output(["nm", os.path.join(san, "_build", "host_asan")], text=True)
    weak = [l for l in out.splitlines() if "mwx_vad_" in l]
    assert weak and all(l.split()[-2] == "w" for l in weak), weak
