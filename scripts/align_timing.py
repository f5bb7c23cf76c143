"""Times transcript alignment (mwx_align_batch).

large-v3 bf16, 32 clips of 30 s: a fixed-step greedy decode (bench_fixed_steps
= --steps) gives every clip its text tokens; mwx_align_batch then aligns each
clip's own tokens in a context with the model's alignment-heads preset.

(a) wall time of mwx_align_batch next to the wall time of the same
    mwx_full_batch call with DTW on and with DTW off (their difference is the
    DTW pass the alignment extends), the three alternating, the median of
    --runs after --warmup (perf classes off);
(b) device time of the perf classes score and logits_gemm of one
    mwx_align_batch call (event pairs around their launches), and the launches.

Prints one JSON line (the line for DESIGN.md).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "sentiric-stt-whisper-service_amd"))
import mwx  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="large-v3")
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    preset = {"large-v3": mwx.AHEADS_LARGE_V3, "base": mwx.AHEADS_BASE}[args.arch]
    wtype = mwx.GGML_BF16 if args.arch == "large-v3" else mwx.GGML_F16
    L = mwx.lib()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, f"{args.arch}.bin")
        mwx.write_synthetic_model(path, args.arch, wtype, 0)
        clips = [mwx.pcm16_to_f32(mwx.synth_pcm16(k, 30 * 16000)) for k in range(args.clips)]
        with mwx.Context.open(path) as off, mwx.Context.open(path, dtw_preset=preset) as on:
            def params(c):
                p = c.default_params(mwx.SAMPLING_GREEDY)
                p.language = b"en"
                p.temperature_inc = 0.0
                p.bench_fixed_steps = args.steps
                return p

            def full(c):
                t0 = time.perf_counter()
                rc = c.full_batch(clips, params(c))
                assert rc == 0, rc
                return (time.perf_counter() - t0) * 1e3

            full(on)
            eot = on.token("eot")
            toks = [[t.id for s in on.segments(i) for t in s.tokens if t.id < eot][:224]
                    for i in range(args.clips)]
            pa = on.default_params(mwx.SAMPLING_GREEDY)
            pa.language = b"en"

            def align():
                t0 = time.perf_counter()
                rc = on.align_batch(clips, toks, pa)
                assert rc == 0, rc
                return (time.perf_counter() - t0) * 1e3

            for _ in range(args.warmup):
                full(off), full(on), align()
            w_off, w_on, w_al = [], [], []
            for _ in range(args.runs):
                w_off.append(full(off))
                w_on.append(full(on))
                w_al.append(align())
            st0 = on.state(0)
            classes = ["score", "logits_gemm"]
            L.mwx_perf_read(st0, None, None)
            L.mwx_perf_enable(st0, ",".join(classes).encode())
            align()
            dev = {}
            for cls in classes:
                ms, n = ctypes.c_double(), ctypes.c_int()
                L.mwx_perf_read_class(st0, cls.encode(), ctypes.byref(ms), ctypes.byref(n))
                dev[cls] = {"ms": round(ms.value, 4), "launches": n.value}
            L.mwx_perf_enable(st0, None)
    med = statistics.median
    print(json.dumps({
        "arch": args.arch, "clips": args.clips, "steps": args.steps,
        "tokens_per_clip": [min(map(len, toks)), max(map(len, toks))],
        "scored_rows": sum(len(t) + 1 for t in toks),
        "wall_ms_align": round(med(w_al), 3), "wall_ms_full_dtw_on": round(med(w_on), 3),
        "wall_ms_full_dtw_off": round(med(w_off), 3),
        "wall_ms_dtw_pass": round(med(w_on) - med(w_off), 3),
        "wall_ms_align_all": [round(x, 2) for x in w_al],
        "wall_ms_on_all": [round(x, 2) for x in w_on],
        "wall_ms_off_all": [round(x, 2) for x in w_off], "device": dev}), flush=True)


if __name__ == "__main__":
    main()
