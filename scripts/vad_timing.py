"""Times the VAD gate: one detect_batch of 32 x 30-s clips and one single clip,
both from HBM-resident input (3 warm-up runs, the median of --runs timed runs,
wall clock around the synchronous call), with the per-kernel split of the
median run (front end / recurrence, and microseconds per LSTM step).

The yardstick is the batch the gate guards: --bench-json names a file holding
the result line of `python bench.py --gpus 1 --lanes 1 ...` from the same box
and visit; one batch takes clips * clip_seconds / audio_sec_per_s_per_gpu, and
gating it should cost no more than 2 % of that.

Writes profiles/vad_timing.json (--out) and prints the two lines for DESIGN.md.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "sentiric-stt-whisper-service_amd"))
import numpy as np  # noqa: E402

import mwx  # noqa: E402


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    rows = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        rows.append((time.perf_counter() - t0) * 1e3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--clip-seconds", type=float, default=30.0)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bench-json", default=None,
                    help="file with the JSON line of bench.py --lanes 1 (same box, same visit)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_timing.json"))
    args = ap.parse_args()
    assert args.runs >= 10 and args.warmup >= 3
    n = int(args.clip_seconds * 16000)
    with tempfile.TemporaryDirectory() as d:
        wpath, vpath = os.path.join(d, "micro.bin"), os.path.join(d, "vad.bin")
        mwx.write_synthetic_model(wpath, "micro", mwx.GGML_F16, 0)  # owns the device buffers
        mwx.write_synthetic_vad_model(vpath, 3)
        with mwx.Context.open(wpath) as ctx, mwx.VadContext(vpath) as vad:
            bufs = [ctx.upload(mwx.pcm16_to_f32(mwx.synth_pcm16(k, n))) for k in range(args.clips)]
            res = {}
            for name, clips in (("batch", bufs), ("single", bufs[:1])):
                kernel = []

                def run():
                    vad.detect_batch(clips)
                    kernel.append(vad.last_kernel_ms())

                wall = timed(run, args.warmup, args.runs)
                kernel = kernel[args.warmup:]
                mid = sorted(range(len(wall)), key=wall.__getitem__)[len(wall) // 2]
                steps = mwx.lib().mwx_vad_n_chunks(n)
                res[name] = {
                    "clips": len(clips), "chunks_per_clip": steps,
                    "wall_ms_median": round(statistics.median(wall), 4),
                    "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4),
                    "frontend_ms": round(kernel[mid][0], 4), "lstm_ms": round(kernel[mid][1], 4),
                    "lstm_us_per_step": round(kernel[mid][1] * 1e3 / steps, 4),
                }
            for b in bufs:
                b.free()
    out = {"clip_seconds": args.clip_seconds, "runs": args.runs, "warmup": args.warmup,
           "input": "HBM-resident f32 PCM (synthetic speech-like clips)", **res}
    if args.bench_json:
        line = [l for l in open(args.bench_json).read().splitlines() if l.startswith("{")][-1]
        rate = json.loads(line)["audio_sec_per_s_per_gpu"]
        batch_ms = args.clips * args.clip_seconds / rate * 1e3
        share = res["batch"]["wall_ms_median"] / batch_ms
        out["yardstick"] = {"bench_lanes1_audio_sec_per_s": rate,
                            "batch_ms": round(batch_ms, 2),
                            "gate_share_of_batch": round(share, 5), "target_share": 0.02,
                            "met": bool(share <= 0.02)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for name in ("batch", "single"):
        r = res[name]
        print(f"VAD {name}: {r['clips']} x {args.clip_seconds:g} s, median {r['wall_ms_median']:.3f} ms "
              f"(front end {r['frontend_ms']:.3f} ms, recurrence {r['lstm_ms']:.3f} ms = "
              f"{r['lstm_us_per_step']:.2f} us/step)")
    if "yardstick" in out:
        y = out["yardstick"]
        print(f"yardstick: one --lanes 1 batch = {y['batch_ms']:.1f} ms; the gate is "
              f"{100 * y['gate_share_of_batch']:.2f} % of it (target <= 2 %)")


if __name__ == "__main__":
    main()
