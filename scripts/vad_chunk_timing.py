"""Times chunked long-form transcription (mwx_vad_trim_batch_chunked,
mwx_full_batch_chunked) against the trimmed path on one long clip.

One synthetic 10-minute clip: bursts of the bench's speech-like signal, 4 s on
and 1 s of zeros. The threshold is scanned over the device's own probabilities
for the one at which the rule cuts closest to the gaps (segment count nearest
the burst count). bench_fixed_steps, so that every window costs the same.
Three legs in one build, on the same states:
  trimmed        trim_batch + mwx_full_batch_trimmed (the windows in sequence)
  chunked        trim_batch(chunk_s) + mwx_full_batch_chunked(max_batch)
  chunked + fit  the same with audio_ctx_fit
Windows decoded and median wall time of each leg (--warmup warm-ups), and the
device time of vad_chunks_kernel next to vad_segments_kernel. The seeded VAD
net is not a speech detector: the figure shows only that windows of one clip
decoded side by side cost fewer steps.

Writes profiles/vad_chunk_timing.json (--out) and prints the lines for DESIGN.md.
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
    wall = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=int, default=10)
    ap.add_argument("--chunk-s", type=float, default=30.0)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arch", default="large-v3")
    ap.add_argument("--wtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--decode-steps", type=int, default=220)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_chunk_timing.json"))
    args = ap.parse_args()
    wt = mwx.GGML_BF16 if args.wtype == "bf16" else mwx.GGML_F16
    # bench.py's model file, shared with it when it ran first
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"mwx_bench_{args.arch}_{args.wtype}.bin")
    if not os.path.exists(path):
        tmp = path + f".tmp{os.getpid()}"
        mwx.write_synthetic_model(tmp, args.arch, wt, 0)
        os.replace(tmp, path)
    n = args.minutes * 60 * 16000
    x = mwx.pcm16_to_f32(mwx.synth_pcm16(200, n))
    bursts = 0
    for s in range(0, n, 5 * 16000):
        x[s + 4 * 16000:s + 5 * 16000] = 0.0
        bursts += 1
    with tempfile.TemporaryDirectory() as d:
        vpath = os.path.join(d, "vad.bin")
        mwx.write_synthetic_vad_model(vpath, 3)
        with mwx.Context.open(path) as ctx, mwx.VadContext(vpath) as vad:
            buf = ctx.upload(x)
            # as the host derives them: uninterrupted speech is still cut at chunk_s
            best = None
            for thr in np.linspace(0.05, 0.95, 37):
                prm = mwx.vad_params(threshold=float(thr), max_speech_duration_s=args.chunk_s)
                with vad.trim_batch([buf], prm) as t:
                    key = (abs(len(t.segments(0)) - bursts), abs(t.n_samples(0) / n - 0.8))
                    if best is None or key < best[0]:
                        best = (key, float(thr), len(t.segments(0)), t.n_samples(0))
            _, thr, n_seg, kept = best
            prm = mwx.vad_params(threshold=thr, max_speech_duration_s=args.chunk_s)
            p = ctx.default_params(mwx.SAMPLING_GREEDY)  # (bench.py's parameters)
            p.language = b"en"
            p.temperature = 0.0
            p.temperature_inc = 0.0
            p.token_timestamps = True
            p.suppress_nst = True
            p.bench_fixed_steps = args.decode_steps
            info = {}

            def trimmed():
                ctx.window_counters(0, reset=True)
                with vad.trim_batch([buf], prm) as t:
                    assert ctx.full_batch_trimmed([t], [0], p) == 0
                info["trimmed"] = ctx.window_counters(0, reset=True)[0]

            def chunked():
                ctx.window_counters(0, reset=True)
                with vad.trim_batch([buf], prm, chunk_s=args.chunk_s) as t:
                    info["chunks"] = len(t.chunks(0))
                    info["kernels"] = vad.last_trim_kernel_ms()[:1] + (vad.last_chunk_kernel_ms(),)
                    assert ctx.full_batch_chunked([t], [0], p, max_batch=args.max_batch) == 0
                info[leg] = ctx.window_counters(0, reset=True)[0]

            w_trim = timed(trimmed, args.warmup, args.runs)
            leg = "chunked"
            w_chunk = timed(chunked, args.warmup, args.runs)
            p.audio_ctx_fit = True
            leg = "chunked_fit"
            w_fit = timed(chunked, args.warmup, args.runs)
            buf.free()
    med = statistics.median
    out = {"clip_minutes": args.minutes, "bursts": bursts, "model": f"{args.arch} {args.wtype}",
           "bench_fixed_steps": args.decode_steps, "threshold": round(thr, 4), "segments": n_seg,
           "kept_fraction": round(kept / n, 4), "chunk_s": args.chunk_s,
           "max_batch": args.max_batch, "chunks": info["chunks"], "runs": args.runs,
           "warmup": args.warmup,
           "segments_kernel_ms": round(info["kernels"][0], 4),
           "chunks_kernel_ms": round(info["kernels"][1], 4),
           "trimmed": {"windows": info["trimmed"], "wall_ms_median": round(med(w_trim), 2)},
           "chunked": {"windows": info["chunked"], "wall_ms_median": round(med(w_chunk), 2)},
           "chunked_fit": {"windows": info["chunked_fit"], "wall_ms_median": round(med(w_fit), 2)},
           "wall_ratio_chunked": round(med(w_chunk) / med(w_trim), 4),
           "wall_ratio_chunked_fit": round(med(w_fit) / med(w_trim), 4)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{args.minutes}-minute clip, {bursts} bursts, threshold {out['threshold']}: "
          f"{n_seg} segments, kept {100 * out['kept_fraction']:.1f} %, {out['chunks']} chunks of "
          f"<= {args.chunk_s:g} s; vad_segments_kernel {out['segments_kernel_ms']:.3f} ms, "
          f"vad_chunks_kernel {out['chunks_kernel_ms']:.3f} ms")
    for name in ("trimmed", "chunked", "chunked_fit"):
        print(f"{name}: {out[name]['windows']} windows, {out[name]['wall_ms_median']:.1f} ms")


if __name__ == "__main__":
    main()
