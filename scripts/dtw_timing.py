"""Times DTW token timestamps (mwx_context_params.dtw_token_timestamps).

For each leg (base f16, one 30-s clip; large-v3 bf16, 32 clips of 30 s) the
same mwx_full_batch call runs in a context with DTW off and in one with the
model's alignment-heads preset: greedy, bench_fixed_steps = --steps so that
every window decodes the same number of text tokens (the alignment pass then
has steps + 2 rows and 1500 columns).

(a) wall time of the call, DTW off and on, alternating, the median of --runs
    after --warmup (perf classes off);
(b) device time of the perf classes dtw_qk, dtw_cost and dtw_path of one
    call (event pairs around their launches), and the number of launches.

Prints one JSON line per leg (the lines for DESIGN.md).
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

LEGS = {"base": ("base", mwx.GGML_F16, mwx.AHEADS_BASE, 1),
        "large-v3": ("large-v3", mwx.GGML_BF16, mwx.AHEADS_LARGE_V3, 32)}


def leg(name, args, d):
    arch, wtype, preset, n_clips = LEGS[name]
    path = os.path.join(d, f"{arch}.bin")
    mwx.write_synthetic_model(path, arch, wtype, 0)
    clips = [mwx.pcm16_to_f32(mwx.synth_pcm16(k, 30 * 16000)) for k in range(n_clips)]
    L = mwx.lib()
    with mwx.Context.open(path) as off, mwx.Context.open(path, dtw_preset=preset) as on:
        def params(c):
            p = c.default_params(mwx.SAMPLING_GREEDY)
            p.language = b"en"
            p.temperature_inc = 0.0
            p.bench_fixed_steps = args.steps
            return p

        def run(c):
            t0 = time.perf_counter()
            rc = c.full_batch(clips, params(c))
            assert rc == 0, rc
            return (time.perf_counter() - t0) * 1e3

        for _ in range(args.warmup):
            run(off), run(on)
        w_off, w_on = [], []
        for _ in range(args.runs):
            w_off.append(run(off))
            w_on.append(run(on))
        n_dtw = sum(t.t_dtw >= 0 for s in on.segments(0) for t in s.tokens)
        st0 = on.state(0)
        classes = ["dtw_qk", "dtw_cost", "dtw_path"]
        L.mwx_perf_read(st0, None, None)
        L.mwx_perf_enable(st0, ",".join(classes).encode())
        run(on)
        dev = {}
        for cls in classes:
            ms, n = ctypes.c_double(), ctypes.c_int()
            L.mwx_perf_read_class(st0, cls.encode(), ctypes.byref(ms), ctypes.byref(n))
            dev[cls] = {"ms": round(ms.value, 4), "launches": n.value}
        L.mwx_perf_enable(st0, None)
    out = {"leg": name, "clips": n_clips, "steps": args.steps, "tokens_with_t_dtw_clip0": int(n_dtw),
           "wall_ms_dtw_off": round(statistics.median(w_off), 3),
           "wall_ms_dtw_on": round(statistics.median(w_on), 3),
           "wall_ms_off_all": [round(x, 2) for x in w_off],
           "wall_ms_on_all": [round(x, 2) for x in w_on], "device": dev}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="base,large-v3")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        for name in args.legs.split(","):
            leg(name, args, d)


if __name__ == "__main__":
    main()
