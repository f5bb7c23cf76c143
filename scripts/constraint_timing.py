"""Times constrained decoding (DESIGN.md "Constrained decoding").

micro f16, 32 clips of 30 s: greedy (32 rows per step) and beam 5 (160 rows per
step), real decoding (a constraint refuses bench_fixed_steps). Per
configuration the device time per launch of the perf classes
"logits_constrain" (the mask kernel) and "logits_proc" (the three logits
processing kernels it sits in front of): a HIP event pair around the launches on
every 8th step of the graph, one class per call, the median of --runs after
--warmup. Constraints:

  none   no constraint: the unconstrained step of the same build
  five   five choices (two- and three-token texts), every flag
  4095   a 4096-state automaton whose 256 byte columns all differ (256 classes,
         a 2 MB table), every state but 0 accepting, no transition to 0: no
         walk ends early, every token's bytes are walked to the end

The penalty is 100 (the default). With MWX_LIB pointing at the parent commit's
library only "none" runs and only "logits_proc" is read: the off path of this
change must match it within the run-to-run spread.

Every step runs in a child process of its own under a time limit (the parent
never opens the GPU) and the script stops at the first step that fails. Prints
one JSON line per step and writes the table to --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "sentiric-stt-whisper-service_amd"))

STEPS = ("greedy:none", "greedy:five", "greedy:4095", "beam:none", "beam:five", "beam:4095")
STEP_LIMIT_S = 240
N_CLIPS = 32


def big_dfa():
    S = 4096
    s = np.arange(S, dtype=np.int64)[:, None]
    b = np.arange(256, dtype=np.int64)[None, :]
    trans = (1 + (s * 31 + b * 7 + (s * b) % 13) % (S - 1)).astype(np.uint16)
    trans[0, :] = 0
    acc = np.ones(S, np.uint8)
    acc[0] = 0
    return trans, acc, 1


def step(args):
    import mwx

    L = mwx.lib()
    mode, kind = args.step.split(":")
    has = hasattr(L, "mwx_constraint_from_dfa")
    if kind != "none" and not has:
        print(json.dumps({"step": args.step, "skipped": "the library has no constraints"}),
              flush=True)
        return
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "micro.bin")
        mwx.write_synthetic_model(path, "micro", mwx.GGML_F16, 0)
        clips = [mwx.pcm16_to_f32(mwx.synth_pcm16(k, 30 * 16000)) for k in range(N_CLIPS)]
        with mwx.Context.open(path) as ctx:
            p = ctx.default_params(mwx.SAMPLING_BEAM_SEARCH if mode == "beam"
                                   else mwx.SAMPLING_GREEDY)
            p.language = b"en"
            p.temperature_inc = 0.0
            if mode == "beam":
                p.beam_search.beam_size = 5
            else:
                p.greedy.best_of = 1
            con = None
            if kind == "five":
                tb = ctx.token_bytes(range(1000, 1012))
                ch = [tb[0] + tb[1], tb[2], tb[3] + tb[4] + tb[5], tb[6] + tb[7],
                      tb[8] + tb[9] + tb[10]]
                con = mwx.Constraint.from_choices(ch, 7)
            elif kind == "4095":
                con = mwx.Constraint.from_dfa(*big_dfa())
            if con is not None:
                p = mwx.with_constraint(p, con, 100.0)
            st0 = ctx.state(0)

            def call(cls):
                L.mwx_perf_read(st0, None, None)
                L.mwx_perf_enable(st0, cls)
                rc = ctx.full_batch(clips, p)
                ms, n = ctypes.c_double(), ctypes.c_int()
                L.mwx_perf_read_class(st0, cls, ctypes.byref(ms), ctypes.byref(n))
                L.mwx_perf_enable(st0, None)
                assert rc == 0, rc
                return ms.value, n.value

            out = {"step": args.step, "mode": mode, "constraint": kind,
                   "rows": N_CLIPS * (5 if mode == "beam" else 1),
                   "states": con.n_states if con is not None else 0,
                   "lib": os.environ.get("MWX_LIB", "in-tree")}
            classes = [b"logits_proc"] + ([b"logits_constrain"] if con is not None else [])
            for cls in classes:
                for _ in range(args.warmup):
                    call(cls)
                us = []
                for _ in range(args.runs):
                    ms, n = call(cls)
                    assert n > 0, (cls, n)
                    us.append(ms / n * 1e3)
                name = cls.decode()
                out[name + "_us"] = round(statistics.median(us), 2)
                out[name + "_us_min_max"] = [round(min(us), 2), round(max(us), 2)]
            print(json.dumps(out), flush=True)


def table(rows):
    def cell(r, k):
        if k + "_us" not in r:
            return "no launch"
        lo, hi = r[k + "_us_min_max"]
        return f"{r[k + '_us']:.2f} ({lo:.2f} .. {hi:.2f})"
    lines = ["| decode | rows | constraint | library | `logits_constrain` per launch, us "
             "(min .. max) | `logits_proc` per launch, us (min .. max) |",
             "|---|---|---|---|---|---|"]
    for r in rows:
        if "mode" not in r:
            continue
        lib = "parent" if r["lib"] != "in-tree" else "this change"
        lines.append(f"| {r['mode']} | {r['rows']} | {r['constraint']} ({r['states']} states) | "
                     f"{lib} | {cell(r, 'logits_constrain')} | {cell(r, 'logits_proc')} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--parent-lib", default=None,
                    help="the parent commit's libmwx.so: its 'none' rows are measured too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constraint_timing.md"))
    args = ap.parse_args()
    if args.step:
        step(args)
        return 0
    rows = []
    plan = [(s, None) for s in args.steps.split(",")]
    if args.parent_lib:
        plan += [(s, args.parent_lib) for s in args.steps.split(",") if s.endswith(":none")]
    for s, lib in plan:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__),
               "--warmup", str(args.warmup), "--runs", str(args.runs), "--step", s]
        env = dict(os.environ)
        if lib:
            env["MWX_LIB"] = os.path.abspath(lib)
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:  # (a fault, an abort or the time limit: nothing more on the GPU)
            print(json.dumps({"step": s, "failed": r.returncode}), flush=True)
            return 1
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                rows.append(json.loads(line))
    with open(args.out, "w") as f:
        f.write(table(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
