#!/usr/bin/env python3
"""Timing of the fitted audio context (mwx_full_params.audio_ctx_fit, DESIGN.md
D9) on the GPU, fit on against full context, same build, same process, runs
alternated: one JSON line per leg.

  large-v3: large-v3 bf16, 32 clips of 5 s, bench_fixed_steps 32, greedy;
            device ms of enc_gemm, enc_attn, cross_gemm, dec_attn_cross
            (mwx_perf_enable / mwx_perf_read_class) and the wall per batch.
  base:     base f16, one 3-s clip (C2's shape), default greedy; wall per
            request.

Synthetic weights: the times are the engine's, the transcripts mean nothing.
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

CLASSES = ["enc_gemm", "enc_attn", "cross_gemm", "dec_attn_cross"]


def leg(name, args, d):
    arch, wtype, n_clips, seconds, steps = {
        "large-v3": ("large-v3", mwx.GGML_BF16, 32, 5.0, 32),
        "base": ("base", mwx.GGML_F16, 1, 3.0, 0)}[name]
    path = os.path.join(d, f"{arch}.bin")
    mwx.write_synthetic_model(path, arch, wtype, 0)
    clips = [mwx.pcm16_to_f32(mwx.synth_pcm16(k, int(seconds * 16000))) for k in range(n_clips)]
    L = mwx.lib()
    with mwx.Context.open(path) as c:
        def params(fit):
            p = c.default_params(mwx.SAMPLING_GREEDY)
            p.language = b"en"
            p.temperature_inc = 0.0
            p.bench_fixed_steps = steps
            p.audio_ctx_fit = fit
            return p

        def run(fit):
            t0 = time.perf_counter()
            rc = c.full_batch(clips, params(fit))
            assert rc == 0, rc
            return (time.perf_counter() - t0) * 1e3

        for _ in range(args.warmup):
            run(False), run(True)
        wall = {False: [], True: []}
        for _ in range(args.runs):
            for fit in (False, True):
                wall[fit].append(run(fit))
        st0 = c.state(0)
        dev = {}
        for fit in (False, True):
            L.mwx_perf_read(st0, None, None)
            L.mwx_perf_enable(st0, ",".join(CLASSES).encode())
            run(fit)
            dev[fit] = {}
            for cls in CLASSES:
                ms, n = ctypes.c_double(), ctypes.c_int()
                L.mwx_perf_read_class(st0, cls.encode(), ctypes.byref(ms), ctypes.byref(n))
                dev[fit][cls] = {"ms": round(ms.value, 4), "launches": n.value}
            L.mwx_perf_enable(st0, None)
        n_ctx = c.audio_ctx_for(len(clips[0]), 0, 0, True)
    out = {"leg": name, "clips": n_clips, "seconds": seconds, "steps": steps, "fit_n_ctx": n_ctx}
    for fit, key in ((False, "full"), (True, "fit")):
        out[f"wall_ms_{key}"] = round(statistics.median(wall[fit]), 3)
        out[f"wall_ms_{key}_all"] = [round(x, 2) for x in wall[fit]]
        out[f"device_{key}"] = dev[fit]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="large-v3,base")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        for name in args.legs.split(","):
            leg(name, args, d)


if __name__ == "__main__":
    main()
