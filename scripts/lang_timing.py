"""Times language identification (DESIGN.md "Language identification").

large-v3-l2 bf16, 30-s clips:

(a) wall time of a detection-only call (detect_language: log-mel, encoder, one
    decode step, lang_probs_kernel, the copies back) for 1 clip and for 32
    clips, the median of --runs after --warmup;
(b) device time of lang_probs_kernel alone at R = 32 rows of the model's
    vocabulary: the perf class "lang" of the 32-clip detection call (a HIP
    event pair around the launch), one call per sample.

Every step runs in a child process of its own under a time limit (the parent
never opens the GPU) and the script stops at the first step that fails. With
MWX_LIB pointing at an older libmwx.so the same steps of (a) time that library
(step (b) is skipped when the library has no lang_probs kernel): the
detection-only call of this change must not be slower than its parent's by
more than the run-to-run spread.

Prints one JSON line per step (the lines for DESIGN.md).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "sentiric-stt-whisper-service_amd"))

STEPS = ("detect1", "detect32", "kernel32")
STEP_LIMIT_S = 240


def step(args):
    import mwx

    L = mwx.lib()
    n_clips = 1 if args.step == "detect1" else 32
    has_kernel = hasattr(L, "mwx_test_lang_probs")
    if args.step == "kernel32" and not has_kernel:
        print(json.dumps({"step": args.step, "skipped": "the library has no lang_probs kernel"}),
              flush=True)
        return
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{args.arch}.bin")
        mwx.write_synthetic_model(path, args.arch, mwx.GGML_BF16, 0)
        clips = [mwx.pcm16_to_f32(mwx.synth_pcm16(k, 30 * 16000)) for k in range(n_clips)]
        with mwx.Context.open(path) as ctx:
            p = ctx.default_params(mwx.SAMPLING_GREEDY)
            p.language = b"auto"
            p.detect_language = True

            def detect():
                t0 = time.perf_counter()
                rc = ctx.full_batch(clips, p)
                assert rc == 0, rc
                return (time.perf_counter() - t0) * 1e3

            for _ in range(args.warmup):
                detect()
            if args.step != "kernel32":
                w = [detect() for _ in range(args.runs)]
                print(json.dumps({"step": args.step, "arch": args.arch, "clips": n_clips,
                                  "lib": os.environ.get("MWX_LIB", "in-tree"),
                                  "wall_ms_detect": round(statistics.median(w), 3),
                                  "wall_ms_min_max": [round(min(w), 3), round(max(w), 3)],
                                  "wall_ms_all": [round(x, 2) for x in w]}), flush=True)
                return
            st0 = ctx.state(0)
            dev = []
            for _ in range(args.runs):
                L.mwx_perf_read(st0, None, None)
                L.mwx_perf_enable(st0, b"lang")
                detect()
                ms, n = ctypes.c_double(), ctypes.c_int()
                L.mwx_perf_read_class(st0, b"lang", ctypes.byref(ms), ctypes.byref(n))
                assert n.value == 1, n.value
                dev.append(ms.value * 1e3)
                L.mwx_perf_enable(st0, None)
            print(json.dumps({"step": args.step, "arch": args.arch, "rows": n_clips,
                              "vocab": ctx.hparam("n_vocab"),
                              "device_us_lang_probs": round(statistics.median(dev), 2),
                              "device_us_all": [round(x, 2) for x in dev]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="large-v3-l2")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--steps", default=",".join(STEPS))
    args = ap.parse_args()
    if args.step:
        step(args)
        return 0
    for s in args.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__),
               "--arch", args.arch, "--warmup", str(args.warmup), "--runs", str(args.runs),
               "--step", s]
        rc = subprocess.run(cmd).returncode
        if rc != 0:  # (a fault, an abort or the time limit: nothing more on the GPU)
            print(json.dumps({"step": s, "failed": rc}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
