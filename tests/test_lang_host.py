"""The host SttEngine's language identification on the CPU:
tests/lang/host_lang_check.cpp drives detect_language / detect_language_pcm16
and TranscriptionResult::language_probability over a CPU stand-in with the
language-probability calls, and once more linked against the plain stand-in
without them (detect_language() must answer nothing, language_probability stay
-1). Both are built with AddressSanitizer + UBSan as stand-alone programs and
run as child processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "lang")


@pytest.mark.parametrize("prog", ["host_lang_check", "host_lang_unbound"])
def test_host_lang_under_asan_ubsan(tmp_path, prog):
    subprocess.check_call(["make", "-s", "-C", DIR, f"_build/{prog}"])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    for k in [k for k in env if k.startswith("STT_WHISPER_SERVICE_DTW_")]:
        del env[k]
    r = subprocess.run([os.path.join(DIR, "_build", prog), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert f"{prog}: 0 failure(s)" in r.stdout
