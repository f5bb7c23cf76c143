"""Constrained decoding on the CPU, as a stand-alone program built with
AddressSanitizer + UBSan and run as a child process (tests/constraint/Makefile):
host_constraint_check links the constraint source (csrc/constraint.cpp)
directly (choices with every flag, the refusals, the 4095-state limit, a DFA)
and drives the host SttEngine over a CPU stand-in that records
mwx_full_params.constraint and walks it during the call (the key rule: no
choices means the old key; the penalty's default and resolution order; dropped
choices; the per-key constraint cache; choice_match; the batch entry point, the
batcher and a streaming session)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "constraint")


def test_host_constraint_under_asan_ubsan(tmp_path):
    prog = "host_constraint_check"
    subprocess.check_call(["make", "-s", "-C", DIR, f"_build/{prog}"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    for k in [k for k in env if k.startswith("STT_WHISPER_SERVICE_")]:
        del env[k]
    r = subprocess.run([os.path.join(DIR, "_build", prog), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert f"{prog}: 0 failure(s)" in r.stdout
