"""Contextual biasing on the CPU, as stand-alone programs built with
AddressSanitizer + UBSan and run as child processes (tests/bias/Makefile):
matcher_check links the matcher source (csrc/bias.cpp) directly and repeats the
random comparison against the naive rule, the carried state, the table bound
and the refused inputs; host_bias_check drives the host SttEngine over a CPU
stand-in that records mwx_full_params.bias_phrases (two phrases per hotword,
the boost's resolution order, dropped hotwords, the batching key, nothing
passed when the boost resolves to 0, the batcher and a streaming session)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "bias")


@pytest.mark.parametrize("prog", ["matcher_check", "host_bias_check"])
def test_host_bias_under_asan_ubsan(tmp_path, prog):
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
