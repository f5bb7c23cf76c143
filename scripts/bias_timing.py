"""Times contextual biasing (DESIGN.md "Contextual biasing").

Per model (micro f16 and the large-v3-shaped large-v3-l2 bf16), 8 clips of
30 s, greedy, a fixed number of decode steps per window (bench_fixed_steps):

(a) the decode step's wall time with 0, 16 and 1024 phrases: the difference
    between a 72-step and an 8-step call divided by 64 (the log-mel and the
    encoder cancel), the median of --runs after --warmup;
(b) device time of logits_bias_kernel per launch with 16 and 1024 phrases: the
    perf class "logits_bias" (a HIP event pair around the launch on every 8th
    step of the graph).

The phrases are seeded random text ids, 1 to 16 per phrase, at a boost of 0.5
(they change the output: what is timed is the launch, not the text).

Every step runs in a child process of its own under a time limit (the parent
never opens the GPU) and the script stops at the first step that fails. With
MWX_LIB pointing at the parent commit's libmwx.so only the 0-phrase column of
(a) runs: that column of this change must not be slower than the parent's by
more than the run-to-run spread.

Prints one JSON line per step (the lines for profiles/bias_timing.md).
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

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "sentiric-stt-whisper-service_amd"))

STEPS = ("micro:0", "micro:16", "micro:1024", "large-v3-l2:0", "large-v3-l2:16",
         "large-v3-l2:1024")
STEP_LIMIT_S = 240
N_CLIPS = 8
SHORT, LONG = 8, 72


def step(args):
    import mwx

    L = mwx.lib()
    arch, n_phr = args.step.split(":")
    n_phr = int(n_phr)
    has_bias = hasattr(L, "mwx_test_bias_match")
    if n_phr and not has_bias:
        print(json.dumps({"step": args.step, "skipped": "the library has no contextual biasing"}),
              flush=True)
        return
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{arch}.bin")
        wtype = mwx.GGML_F16 if arch == "micro" else mwx.GGML_BF16
        mwx.write_synthetic_model(path, arch, wtype, 0)
        clips = [mwx.pcm16_to_f32(mwx.synth_pcm16(k, 30 * 16000)) for k in range(N_CLIPS)]
        with mwx.Context.open(path) as ctx:
            rng = np.random.default_rng(n_phr)
            eot = ctx.token("eot")
            phrases = [([int(t) for t in rng.integers(0, eot, int(rng.integers(1, 17)))], 0.5)
                       for _ in range(n_phr)]

            def params(steps):
                p = ctx.default_params(mwx.SAMPLING_GREEDY)
                p.language = b"en"
                p.temperature_inc = 0.0
                p.greedy.best_of = 1
                p.bench_fixed_steps = steps
                return mwx.with_bias(p, phrases) if n_phr else p

            ps, pl = params(SHORT), params(LONG)

            def call(p):
                t0 = time.perf_counter()
                rc = ctx.full_batch(clips, p)
                assert rc == 0, rc
                return (time.perf_counter() - t0) * 1e3

            for _ in range(args.warmup):
                call(ps)
                call(pl)
            per_step = []
            for _ in range(args.runs):
                a, b = call(ps), call(pl)
                per_step.append((b - a) / (LONG - SHORT) * 1e3)
            out = {"step": args.step, "arch": arch, "phrases": n_phr, "rows": N_CLIPS,
                   "lib": os.environ.get("MWX_LIB", "in-tree"),
                   "step_us": round(statistics.median(per_step), 2),
                   "step_us_min_max": [round(min(per_step), 2), round(max(per_step), 2)]}
            if n_phr:
                st0 = ctx.state(0)
                dev = []
                for _ in range(args.runs):
                    L.mwx_perf_read(st0, None, None)
                    L.mwx_perf_enable(st0, b"logits_bias")
                    call(pl)
                    ms, n = ctypes.c_double(), ctypes.c_int()
                    L.mwx_perf_read_class(st0, b"logits_bias", ctypes.byref(ms), ctypes.byref(n))
                    L.mwx_perf_enable(st0, None)
                    assert n.value > 0, n.value
                    dev.append(ms.value / n.value * 1e3)
                out["device_us_logits_bias"] = round(statistics.median(dev), 2)
                out["device_us_min_max"] = [round(min(dev), 2), round(max(dev), 2)]
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--steps", default=",".join(STEPS))
    args = ap.parse_args()
    if args.step:
        step(args)
        return 0
    for s in args.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__),
               "--warmup", str(args.warmup), "--runs", str(args.runs), "--step", s]
        rc = subprocess.run(cmd).returncode
        if rc != 0:  # (a fault, an abort or the time limit: nothing more on the GPU)
            print(json.dumps({"step": s, "failed": rc}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
