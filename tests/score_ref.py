"""Plain-numpy float64 reference of transcript scoring (k_score.hip
score_rows_kernel), the error bound derived from the kernel's
rounding points, an f32 emulation in the kernel's summation order and in
pairwise order (with named mutants), and the seeded inputs the tests run.
Shared by test_score_ref.py (CPU), test_gpu_score_kernel.py and
test_gpu_align.py; not a test module itself and needs no GPU.

Contract, per active row with raw logits x [V] and target t (an inactive row is
left unwritten; rows without a finite entry and NaN are outside it):
  lse      log sum_i exp(x_i), -inf entries contributing 0
  plog     x_t - lse (-inf when x_t = -inf);  p = exp(plog) (0 then)
  top_id   argmax x, the lowest index among bit-equal values
  top_plog x_top_id - lse
Exact: top_id, which rows are written, plog = -inf and p = 0 at a -inf target.

Bounded. u = 2^-24, E = 3 ulp = 6 u for expf and logf, as logits_ref.py. The
kernel holds the row in registers (thread t of 1024 owns t + 1024 k, k < 52),
takes the maximum M, forms one expf(x_i - M) per finite entry, sums a thread's
<= 52 terms in index order, the wave's 64 threads through the 6-level xor
butterfly, and the 16 wave sums pairwise in wave order (4 levels). Rounding
points of S = sum exp(x_i - M), as relative errors of term i with true weight
w_i = exp(x_i - lse):
  the f32 subtraction x_i - M: u (M - x_i) on the exponent, so on the term;
  the expf: E (one per term: there is no chunk maximum and no rescale);
  the additions: a term passes through at most D = 52 + 6 + 4 = 62 of them.
  rel_S   = sum_i w_i (u (M - x_i) + E) + D u + V 2^-126
  err_lse = rel_S + E |lse - M| + u |lse|             (logf(S); logf(S) + M)
  b_lp_i  = err_lse + u (|x_i - lse| + err_lse)       (x_i - lse), at t and top
  b_p     = p (expm1(b_lp_t) + E) + 2^-126
Pairwise summation (depth ceil(log2 n)) is held to the same D = 62.

Condition on the inputs (margins()): apart from bit-equal ties, which the
lowest index settles, the top-1 / top-2 margin of every row is at least 16 times
its b_lp, and the top's log-prob is not where expf leaves the normal range
(-106 .. -87).
"""
from dataclasses import dataclass

import numpy as np

from logits_ref import E, FLT_MIN, U, exp32, log32

SC_T, SC_W, SC_NPT = 1024, 16, 52
MAX_VOCAB = SC_T * SC_NPT
KERNEL_DEPTH = SC_NPT + 6 + 4
MARGIN = 16.0
P_NORMAL, P_ZERO = -87.0, -106.0
NEG = np.float32(-np.inf)


def err_lse(x64, depth=KERNEL_DEPTH):
    """(lse, M, err_lse) of one row (float64, at least one finite entry)."""
    y = x64[np.isfinite(x64)]
    M = y.max()
    lse = float(np.log(np.exp(y - M).sum()) + M)
    w = np.exp(y - lse)
    rel_s = float((w * (U * (M - y) + E)).sum()) + depth * U + x64.size * FLT_MIN
    return lse, float(M), rel_s + E * abs(lse - M) + U * abs(lse)


def b_lp_at(lp, err):
    return err + U * (abs(lp) + err) if np.isfinite(lp) else 0.0


def reference(x, t, depth=KERNEL_DEPTH):
    """The float64 reference of one row and its bounds."""
    x32 = np.asarray(x, np.float32)
    x64 = x32.astype(np.float64)
    lse, M, err = err_lse(x64, depth)
    top = int(np.argmax(x32))  # the first maximum: the lowest index
    plog = x64[t] - lse if np.isfinite(x64[t]) else -np.inf
    top_plog = M - lse
    rest = x64[x32 != x32[top]]
    rest = rest[np.isfinite(rest)]
    b_lp, b_top = b_lp_at(plog, err), b_lp_at(top_plog, err)
    p = float(np.exp(plog)) if np.isfinite(plog) else 0.0
    return dict(lse=lse, err_lse=err, plog=plog, p=p, top_id=top, top_plog=top_plog,
                b_plog=b_lp, b_top_plog=b_top,
                b_p=p * (np.expm1(b_lp) + E) + FLT_MIN if p > 0 else 0.0,
                gap=float(M - rest.max()) if rest.size else np.inf)


def margins(r):
    """Asserts the condition on the inputs for one row."""
    need = MARGIN * max(r["b_plog"], r["b_top_plog"])
    assert r["gap"] >= need, ("top-1 / top-2", r["gap"], need)
    assert not (P_ZERO <= r["top_plog"] <= P_NORMAL), ("top near underflow", r["top_plog"])


# ------------------------------------------------------------------ emulation

def _sum_kernel(e):
    """[V] terms (0 where the entry is -inf) as the workgroup sums them."""
    a = np.zeros(SC_NPT * SC_T, np.float32)
    a[:e.size] = e
    a = a.reshape(SC_NPT, SC_T)
    s = a[0].copy()
    for k in range(1, SC_NPT):
        s = (s + a[k]).astype(np.float32)
    w = s.reshape(SC_W, 64)
    while w.shape[1] > 1:  # the xor butterfly: offsets 32, 16, ..., 1
        h = w.shape[1] // 2
        w = (w[:, :h] + w[:, h:]).astype(np.float32)
    w = w[:, 0]
    while w.size > 1:      # the wave sums, neighbours first
        w = (w[0::2] + w[1::2]).astype(np.float32)
    return w[0]


def _sum_pair(e):
    n = 1
    while n < max(e.size, 1):
        n *= 2
    v = np.zeros(n, np.float32)
    v[:e.size] = e
    while v.size > 1:
        v = (v[0::2] + v[1::2]).astype(np.float32)
    return v[0]


MUTANTS = ("no_max", "tie_high", "target_twice")


def emulate(x, t, order="kernel", mutant=None, ulp=0):
    """f32 emulation of one row: dict(plog, p, top_id, top_plog). ulp moves
    every expf / logf result by that many f32 steps."""
    x = np.asarray(x, np.float32)
    m = x.max()
    ties = np.nonzero(x == m)[0]
    mi = int(ties[-1] if mutant == "tie_high" else ties[0])
    fin = x > NEG
    sub = np.float32(0) if mutant == "no_max" else m
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.where(fin, exp32(np.where(fin, x - sub, 0).astype(np.float32), ulp), np.float32(0))
    e = e.astype(np.float32)
    S = (_sum_kernel if order == "kernel" else _sum_pair)(e)
    if mutant == "target_twice":
        S = np.float32(S + e[t])
    with np.errstate(over="ignore", invalid="ignore"):
        lse = np.float32(log32(S, ulp) + sub)
        plog = np.float32(x[t] - lse) if x[t] > NEG else NEG
        p = exp32(plog, ulp) if x[t] > NEG else np.float32(0)
        return dict(plog=plog, p=np.float32(p), top_id=mi, top_plog=np.float32(m - lse))


def compare(r, got, ratios=None):
    """The fields of `got` (plog, p, top_id, top_plog) outside the reference's
    bounds or unequal where exactness is required. ratios: |err| / bound."""
    bad = []
    if int(got["top_id"]) != r["top_id"]:
        bad.append(("top_id", int(got["top_id"]), r["top_id"]))
    for name in ("plog", "top_plog", "p"):
        want, b, g = r[name], r["b_" + name], float(got[name])
        if not np.isfinite(want) or b == 0.0:
            if not (g == want):
                bad.append((name, g, want))
            continue
        err = abs(g - want)
        if ratios is not None:
            ratios[name] = max(ratios.get(name, 0.0), err / b)
        if not err <= b:
            bad.append((name, g, want, err / b))
    return bad


# --------------------------------------------------------------------- inputs

@dataclass
class Case:
    name: str
    x: np.ndarray       # [R][V] f32
    target: np.ndarray  # [R] int32
    active: np.ndarray  # [R] int32

    @property
    def R(self):
        return self.x.shape[0]


def settle(x):
    """Lifts the row's maximum so that the top-1 / top-2 margin is 0.01 at
    least (far above 16 b_lp, which stays below 2e-3 on these inputs)."""
    top = int(np.argmax(x))
    rest = np.delete(x, top)
    rest = rest[np.isfinite(rest)]
    if rest.size and x[top] - rest.max() < 0.01:
        x[top] = np.float32(rest.max() + np.float32(0.0125))
    return x


# bit-equal maxima at both ends of a thread's run (k = 0 and the row's last k
# of that thread), of neighbouring lanes, of a wave edge, across waves, at the
# edge between two k (1023 | 1024) and at the ends of the row
def tie_pairs(V):
    last_k = lambda t: t + SC_T * ((V - 1 - t) // SC_T)
    pairs = {"lanes": (5, 6), "wave_edge": (63, 64), "waves": (5, 70), "k_edge": (1023, 1024),
             "thread_ends": (7, last_k(7)), "last_thread": (1023, last_k(1023)),
             "row_ends": (0, V - 1), "last_two": (V - 2, V - 1)}
    return {n: p for n, p in pairs.items() if 0 <= p[0] < p[1] < V}


VOCAB_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 51864, 51865, 51866)


def _rows(V, rng):
    """(x, target, active) rows of one vocabulary size: magnitudes, holes,
    targets at 0 / V - 1 / the argmax / a hole, an inactive row."""
    xs, ts, act = [], [], []

    def add(x, t, a=1):
        xs.append(settle(x.astype(np.float32)))
        ts.append(int(t))
        act.append(a)

    add(rng.standard_normal(V), 0)
    add(20.0 * rng.standard_normal(V), V - 1)
    x = rng.uniform(-80.0, 80.0, V)
    add(x, int(np.argmax(x)))
    add(rng.standard_normal(V), V // 2, a=0)  # inactive
    # (a row far from 0 either way: exp(x) alone would overflow / vanish)
    add(100.0 + rng.standard_normal(V), V - 1)
    add(-120.0 + rng.standard_normal(V), 0)
    if V >= 2:
        for at_hole in (True, False):
            x = (3.0 * rng.standard_normal(V)).astype(np.float32)
            hole = rng.random(V) < 0.3
            hole[int(np.argmax(np.where(hole, -np.inf, x)))] = False  # (a finite entry stays)
            hole[0], hole[V - 1] = True, False
            x[hole] = -np.inf
            add(x, 0 if at_hole else V - 1)
    return np.stack(xs), np.array(ts, np.int32), np.array(act, np.int32)


def _tie_rows(V, rng):
    xs, ts = [], []
    for a, b in tie_pairs(V).values():
        for t in (a, b):
            x = (2.0 * rng.standard_normal(V)).astype(np.float32)
            x[a] = x[b] = np.float32(x.max() + 1.0)
            xs.append(x)
            ts.append(t)
    return np.stack(xs), np.array(ts, np.int32), np.ones(len(ts), np.int32)


# rows of the launch-grid case: one workgroup per row, so the grid's edge is the
# chip's 256 compute units (R = 255, 256, 257 launch its prefixes)
GRID_R, GRID_V = 257, 1025

_cases = None


def cases():
    global _cases
    if _cases is None:
        out = []
        for V in VOCAB_SIZES:
            rng = np.random.default_rng(1000 + V)
            out.append(Case(f"v{V}", *_rows(V, rng)))
        for V in (2049, 51866):
            out.append(Case(f"ties{V}", *_tie_rows(V, np.random.default_rng(7000 + V))))
        rng = np.random.default_rng(99)
        x = np.stack([settle((3.0 * rng.standard_normal(GRID_V)).astype(np.float32))
                      for _ in range(GRID_R)])
        out.append(Case("grid", x, rng.integers(0, GRID_V, GRID_R).astype(np.int32),
                        (np.arange(GRID_R) % 7 != 3).astype(np.int32)))
        _cases = out
    return _cases


_refs = {}


def references(case):
    """The float64 reference of every active row (None for an inactive one);
    computed once per case and shared."""
    if case.name not in _refs:
        _refs[case.name] = [reference(case.x[k], int(case.target[k])) if case.active[k] else None
                            for k in range(case.R)]
    return _refs[case.name]


def log_softmax64(x):
    """float64 log-softmax of the rows of x (-inf entries stay -inf)."""
    x = np.asarray(x, np.float64)
    M = x.max(axis=-1, keepdims=True)
    return x - (np.log(np.exp(x - M).sum(axis=-1, keepdims=True)) + M)
