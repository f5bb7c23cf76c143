"""Times VAD silence trimming (mwx_vad_trim_batch, mwx_full_batch_trimmed).

(a) Kernel time: one trim_batch of 32 HBM-resident 30-s clips (3 warm-up runs,
    the median of --runs timed runs): device time of vad_segments_kernel and
    vad_compact_kernel next to the front end + recurrence of the same call.
(b) End to end: 32 clips of 60 s (bursts of the synthetic speech-like signal
    between silence), bench_fixed_steps so that every 30-s window costs the
    same, and the threshold (scanned over the device's own probabilities) at
    which the rule keeps closest to half of the audio. Windows decoded and
    wall time of the untrimmed mwx_full_batch and of trim_batch +
    mwx_full_batch_trimmed, same build, same states. The seeded VAD net is not
    a speech detector: the figure shows only that removed audio is removed
    work.

Writes profiles/vad_trim_timing.json (--out) and prints the lines for DESIGN.md.
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


def median_run(fn, warmup, runs):
    """(wall ms of every timed run, index of the median run)"""
    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall, sorted(range(runs), key=wall.__getitem__)[runs // 2]


def kernel_leg(ctx, vad, args):
    n = 30 * 16000
    bufs = [ctx.upload(mwx.pcm16_to_f32(mwx.synth_pcm16(k, n))) for k in range(args.clips)]
    # the copy is largest when everything is kept: the candidate threshold at
    # which this net keeps the most audio

    def kept_at(thr):
        with vad.trim_batch(bufs, mwx.vad_params(threshold=thr)) as t:
            return sum(t.n_samples(i) for i in range(len(t)))

    thr = max((0.5, 0.35, 0.2, 0.1, 0.03), key=kept_at)
    prm = mwx.vad_params(threshold=thr)
    rows = []

    def run():
        with vad.trim_batch(bufs, prm) as t:
            kept = sum(t.n_samples(i) for i in range(len(t)))
            segs = sum(len(t.segments(i)) for i in range(len(t)))
        rows.append(vad.last_kernel_ms() + vad.last_trim_kernel_ms() + (kept, segs))

    wall, mid = median_run(run, args.warmup, args.runs)
    fe, lstm, seg, cp, kept, segs = rows[args.warmup + mid]
    for b in bufs:
        b.free()
    return {"clips": args.clips, "clip_seconds": 30, "threshold": thr,
            "chunks_per_clip": mwx.lib().mwx_vad_n_chunks(n), "segments": segs,
            "compacted_mb": round(kept * 4 / 1e6, 2),
            "wall_ms_median": round(statistics.median(wall), 4),
            "frontend_ms": round(fe, 4), "lstm_ms": round(lstm, 4),
            "segments_ms": round(seg, 4), "compact_ms": round(cp, 4),
            "new_kernels_share_of_vad_pass": round((seg + cp) / (fe + lstm), 4)}


def e2e_leg(ctx, vad, args):
    n = 60 * 16000
    clips = []
    for k in range(args.clips):
        x = mwx.pcm16_to_f32(mwx.synth_pcm16(100 + k, n))
        keep = np.zeros(n, bool)
        for a, b in ((2, 14), (31, 44)):  # two bursts, 25 s of signal in 60 s
            keep[a * 16000:b * 16000] = True
        x[~keep] = 0.0
        clips.append(x)
    bufs = [ctx.upload(x) for x in clips]
    total = float(n * args.clips)
    best = None
    for thr in np.linspace(0.05, 0.95, 37):
        with vad.trim_batch(bufs, mwx.vad_params(threshold=float(thr))) as t:
            kept = sum(t.n_samples(i) for i in range(len(t))) / total
        if best is None or abs(kept - 0.5) < abs(best[1] - 0.5):
            best = (float(thr), kept)
    prm = mwx.vad_params(threshold=best[0])
    p = ctx.default_params(mwx.SAMPLING_GREEDY)  # (bench.py's parameters)
    p.language = b"en"
    p.temperature = 0.0
    p.temperature_inc = 0.0
    p.token_timestamps = True
    p.suppress_nst = True
    p.bench_fixed_steps = args.decode_steps
    for i in range(args.clips):
        ctx.state(i)
    windows = {}

    def plain():
        ctx.window_counters(0, reset=True)
        assert ctx.full_batch_device(bufs, p) == 0
        windows["untrimmed"] = ctx.window_counters(0, reset=True)[0]

    def trimmed():
        ctx.window_counters(0, reset=True)
        with vad.trim_batch(bufs, prm) as t:
            assert ctx.full_batch_trimmed([t] * args.clips, list(range(args.clips)), p) == 0
        windows["trimmed"] = ctx.window_counters(0, reset=True)[0]

    w_plain, _ = median_run(plain, 1, args.e2e_runs)
    w_trim, _ = median_run(trimmed, 1, args.e2e_runs)
    for b in bufs:
        b.free()
    return {"clips": args.clips, "clip_seconds": 60, "model": f"{args.arch} {args.wtype}",
            "bench_fixed_steps": args.decode_steps, "threshold": round(best[0], 4),
            "kept_fraction": round(best[1], 4), "runs": args.e2e_runs,
            "untrimmed": {"windows": windows["untrimmed"],
                          "wall_ms_median": round(statistics.median(w_plain), 2)},
            "trimmed": {"windows": windows["trimmed"],
                        "wall_ms_median": round(statistics.median(w_trim), 2)},
            "wall_ratio": round(statistics.median(w_trim) / statistics.median(w_plain), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-runs", type=int, default=3)
    ap.add_argument("--arch", default="large-v3")
    ap.add_argument("--wtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--decode-steps", type=int, default=220)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_trim_timing.json"))
    args = ap.parse_args()
    wt = mwx.GGML_BF16 if args.wtype == "bf16" else mwx.GGML_F16
    # bench.py's model file, shared with it when it ran first
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"mwx_bench_{args.arch}_{args.wtype}.bin")
    if not os.path.exists(path):
        tmp = path + f".tmp{os.getpid()}"
        mwx.write_synthetic_model(tmp, args.arch, wt, 0)
        os.replace(tmp, path)
    out = {"runs": args.runs, "warmup": args.warmup,
           "input": "HBM-resident f32 PCM (synthetic speech-like clips)"}
    with tempfile.TemporaryDirectory() as d:
        vpath = os.path.join(d, "vad.bin")
        mwx.write_synthetic_vad_model(vpath, 3)
        with mwx.Context.open(path) as ctx, mwx.VadContext(vpath) as vad:
            out["kernels"] = kernel_leg(ctx, vad, args)
            if not args.skip_e2e:
                out["end_to_end"] = e2e_leg(ctx, vad, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    k = out["kernels"]
    print(f"trim kernels, {k['clips']} x 30 s: segments {k['segments_ms']:.3f} ms + compaction "
          f"{k['compact_ms']:.3f} ms ({k['compacted_mb']} MB) after front end {k['frontend_ms']:.3f} "
          f"ms + recurrence {k['lstm_ms']:.3f} ms; trim_batch wall {k['wall_ms_median']:.3f} ms")
    if "end_to_end" in out:
        e = out["end_to_end"]
        print(f"end to end, {e['clips']} x 60 s at threshold {e['threshold']} (kept "
              f"{100 * e['kept_fraction']:.1f} %): untrimmed {e['untrimmed']['windows']} windows, "
              f"{e['untrimmed']['wall_ms_median']:.1f} ms; trimmed {e['trimmed']['windows']} "
              f"windows, {e['trimmed']['wall_ms_median']:.1f} ms")


if __name__ == "__main__":
    main()
