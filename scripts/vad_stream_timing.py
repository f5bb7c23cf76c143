"""Times streaming VAD against the whole-buffer gate it replaces.

New path: one mwx_vad_stream_feed_batch of 8000 new samples (the sessions'
0.5-s cadence) per stream from host memory, for 1, 8 and 32 streams in the
call, with the per-kernel split of the median run (staging / front end /
recurrence). Comparison, in the same run: one mwx_vad_detect_speech of a 5-,
15- and 30-s host buffer, which is what the gate costs per partial when every
partial runs it over the whole buffer. 3 warm-up runs, the median of --runs
timed runs, wall clock around the synchronous call.

Writes profiles/vad_stream_timing.json (--out) and prints the two lines for
DESIGN.md.
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

FEED = 8000


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
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_stream_timing.json"))
    args = ap.parse_args()
    assert args.runs >= 10 and args.warmup >= 3
    n_calls = args.runs + args.warmup
    with tempfile.TemporaryDirectory() as d:
        vpath = os.path.join(d, "vad.bin")
        mwx.write_synthetic_vad_model(vpath, 3)
        # clip 0 also serves the one-shot calls: 30 s at least
        clips = [mwx.pcm16_to_f32(mwx.synth_pcm16(k, max(30 * 16000 if k == 0 else 0,
                                                         n_calls * FEED))) for k in range(32)]
        feed, detect = {}, {}
        with mwx.VadContext(vpath) as vad:
            for n_streams in (1, 8, 32):
                streams = [vad.stream() for _ in range(n_streams)]
                kernel, at = [], [0]

                def run():
                    a = at[0]
                    mwx.VadStream.feed_batch(streams, [c[a:a + FEED] for c in clips[:n_streams]])
                    at[0] = a + FEED
                    kernel.append(vad.last_stream_kernel_ms())

                wall = timed(run, args.warmup, args.runs)
                kernel = kernel[args.warmup:]
                mid = sorted(range(len(wall)), key=wall.__getitem__)[len(wall) // 2]
                for s in streams:
                    s.free()
                feed[str(n_streams)] = {
                    "streams": n_streams, "samples_per_stream": FEED,
                    "wall_ms_median": round(statistics.median(wall), 4),
                    "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4),
                    "stage_ms": round(kernel[mid][0], 4), "frontend_ms": round(kernel[mid][1], 4),
                    "lstm_ms": round(kernel[mid][2], 4),
                }
            for seconds in (5, 15, 30):
                x = clips[0][:seconds * 16000]
                kernel = []

                def run():
                    vad.detect(x)
                    kernel.append(vad.last_kernel_ms())

                wall = timed(run, args.warmup, args.runs)
                kernel = kernel[args.warmup:]
                mid = sorted(range(len(wall)), key=wall.__getitem__)[len(wall) // 2]
                detect[str(seconds)] = {
                    "seconds": seconds, "chunks": mwx.lib().mwx_vad_n_chunks(len(x)),
                    "wall_ms_median": round(statistics.median(wall), 4),
                    "wall_ms_min": round(min(wall), 4), "wall_ms_max": round(max(wall), 4),
                    "frontend_ms": round(kernel[mid][0], 4), "lstm_ms": round(kernel[mid][1], 4),
                }
    out = {"runs": args.runs, "warmup": args.warmup,
           "input": "host f32 PCM (synthetic speech-like clips)",
           "stream_feed": feed, "one_shot_detect": detect}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("stream feed of 8000 samples, median wall ms (stage / front end / recurrence): " +
          "; ".join(f"{r['streams']} stream(s) {r['wall_ms_median']:.3f} "
                    f"({r['stage_ms']:.3f} / {r['frontend_ms']:.3f} / {r['lstm_ms']:.3f})"
                    for r in feed.values()))
    print("one-shot detect of the whole buffer, median wall ms (front end / recurrence): " +
          "; ".join(f"{r['seconds']} s {r['wall_ms_median']:.3f} "
                    f"({r['frontend_ms']:.3f} / {r['lstm_ms']:.3f})" for r in detect.values()))


if __name__ == "__main__":
    main()
