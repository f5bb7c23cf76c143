"""Plain-numpy float64 reference of language identification (k_lang.hip
lang_probs_kernel, DESIGN.md "Language identification"), the error bound
derived from the kernel's rounding points, an f32 emulation in the kernel's
summation order and in pairwise order (with named mutants), and the seeded
inputs the tests run. Shared by test_lang_ref.py (CPU), test_gpu_lang_kernel.py
and test_gpu_lang_detect.py; not a test module itself and needs no GPU.

Contract, per row with raw logits x [V], over the window x[t0 .. t0 + n),
1 <= n <= 128 (rows without a finite entry in the window and NaN are outside
it; nothing outside the window is read):
  M     max_i x_i
  p_i   exp(x_i - M) / sum_j exp(x_j - M), a -inf entry giving exactly 0
  best  the lowest index among the bit-equal maxima of the logits
Exact: best, and p_i = 0 at a -inf entry.

Bounded. u = 2^-24, E = 3 ulp = 6 u for expf, as logits_ref.py. One wave holds
the row (lane l owns entries l and l + 64), takes the maximum M, forms one
e_i = expf(x_i - M) per finite entry, adds a lane's two terms, sums the 64 lanes
through the 6-level xor butterfly and divides every e_i by the sum S. Rounding
points, as relative errors, with true weight w_i = p_i:
  the f32 subtraction x_i - M: u (M - x_i) on the exponent, so on the term;
  the expf: E (one per term);
  the additions: a term passes through at most D = ceil(n / 64) - 1 + 6;
  the division: u.
  a_i   = u (M - x_i) + E                                   (term i)
  rel_S = sum_i w_i a_i + D u + n 2^-126                     (S >= 1)
  b_p_i = p_i ((1 + a_i) (1 + u) / (1 - rel_S) - 1) + 2^-126 (flushed results)
  b_lp_i = a_i + rel_S + u                                   (on log p_i)
Pairwise summation (depth ceil(log2 n) <= 7) is held to the same D.

Condition on the inputs (margins()): apart from bit-equal ties, which the
lowest index settles, the top-1 / top-2 logit gap of every row is at least 16
times the larger b_lp of the two. The rows of the "near" case alone are exempt,
on purpose: two logits one f32 step apart, the larger at the higher index,
whose probabilities round to the same float. `best` comes from exact
comparisons of the logits, so it is exact there too, and a best taken from the
rounded probabilities (mutant best_from_probs) is wrong there and only there.
"""
from dataclasses import dataclass

import numpy as np

from logits_ref import E, FLT_MIN, U, exp32

MAX_N = 128
MARGIN = 16.0
NEG = np.float32(-np.inf)
T0_MODEL = 50259  # token_sot + 1 of the 51865- and 51866-entry vocabularies
N_LANG = 100      # lang_max_id() + 1: what the engine passes


def depth(n):
    return (n + 63) // 64 - 1 + 6


def reference(x, t0, n):
    """The float64 reference of one row and its bounds."""
    w32 = np.asarray(x, np.float32)[t0:t0 + n]
    w = w32.astype(np.float64)
    fin = np.isfinite(w)
    M = w[fin].max()
    with np.errstate(under="ignore"):
        e = np.where(fin, np.exp(np.where(fin, w - M, 0.0)), 0.0)
    p = e / e.sum()
    a = np.where(fin, U * (M - np.where(fin, w, M)) + E, 0.0)
    rel_s = float((p * a).sum()) + depth(n) * U + n * FLT_MIN
    b_p = np.where(fin, p * ((1 + a) * (1 + U) / (1 - rel_s) - 1) + FLT_MIN, 0.0)
    b_lp = a + rel_s + U
    best = int(np.argmax(w32))  # the first maximum: the lowest index
    rest = np.nonzero(fin & (w32 != w32[best]))[0]
    second = int(rest[np.argmax(w[rest])]) if rest.size else -1
    return dict(p=p, b_p=b_p, best=best, b_lp=b_lp, rel_s=rel_s,
                gap=float(M - w[second]) if second >= 0 else np.inf,
                need=MARGIN * max(b_lp[best], b_lp[second] if second >= 0 else 0.0))


def margins(r):
    """Asserts the condition on the inputs for one row."""
    assert r["gap"] >= r["need"], ("top-1 / top-2", r["gap"], r["need"])


# ------------------------------------------------------------------ emulation

def _sum_kernel(e):
    """[n] terms (0 where the entry is -inf) as the wave sums them."""
    a = np.zeros(MAX_N, np.float32)
    a[:e.size] = e
    w = (a[:64] + a[64:]).astype(np.float32)
    while w.size > 1:  # the xor butterfly: offsets 32, 16, ..., 1
        h = w.size // 2
        w = (w[:h] + w[h:]).astype(np.float32)
    return w[0]


def _sum_pair(e):
    m = 1
    while m < max(e.size, 1):
        m *= 2
    v = np.zeros(m, np.float32)
    v[:e.size] = e
    while v.size > 1:
        v = (v[0::2] + v[1::2]).astype(np.float32)
    return v[0]


MUTANTS = ("no_max", "t0_minus", "t0_plus", "n_minus", "n_plus", "tie_high", "best_from_probs")


def emulate(x, t0, n, order="kernel", mutant=None, ulp=0):
    """f32 emulation of one row: dict(p [n], best), or None where the mutant's
    window does not fit the row. ulp moves every expf result by that many f32
    steps."""
    x = np.asarray(x, np.float32)
    a0 = t0 + {"t0_minus": -1, "t0_plus": 1}.get(mutant, 0)
    m = n + {"n_minus": -1, "n_plus": 1}.get(mutant, 0)
    if a0 < 0 or m < 1 or m > MAX_N or a0 + m > x.size:
        return None
    w = x[a0:a0 + m]
    M = w.max()
    ties = np.nonzero(w == M)[0]
    best = int(ties[-1] if mutant == "tie_high" else ties[0])
    fin = w > NEG
    sub = np.float32(0) if mutant == "no_max" else M
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.where(fin, exp32(np.where(fin, w - sub, 0).astype(np.float32), ulp), np.float32(0))
        e = e.astype(np.float32)
        S = (_sum_kernel if order == "kernel" else _sum_pair)(e)
        p = (e / S).astype(np.float32)
    if mutant == "best_from_probs":
        best = int(np.argmax(p))
    # (the caller's view: n entries from t0 of the row)
    out = np.zeros(n, np.float32)
    lo, hi = max(a0, t0), min(a0 + m, t0 + n)
    out[lo - t0:hi - t0] = p[lo - a0:hi - a0]
    return dict(p=out, best=best + a0 - t0)


def compare(r, got, ratios=None):
    """What of `got` (p [n], best) lies outside the reference's bounds or is
    unequal where exactness is required. ratios["p"]: the largest |err| / bound."""
    bad = []
    if int(got["best"]) != r["best"]:
        bad.append(("best", int(got["best"]), r["best"]))
    g = np.asarray(got["p"], np.float64)
    zero = r["b_p"] == 0.0
    if not (g[zero] == 0.0).all():
        bad.append(("p at -inf", np.nonzero(zero & (g != 0.0))[0][:4].tolist()))
    err = np.abs(g - r["p"])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, r["b_p"]))
    if not np.isfinite(g).all():
        bad.append(("p not finite",))
    elif ratios is not None:
        ratios["p"] = max(ratios.get("p", 0.0), float(ratio.max()))
    if not (ratio <= 1.0).all():  # (NaN fails)
        k = int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)))
        bad.append(("p", k, float(g[k]), float(r["p"][k]), float(ratio[k])))
    return bad


# --------------------------------------------------------------------- inputs

@dataclass
class Case:
    name: str
    V: int
    t0: int
    n: int
    win: np.ndarray   # [R][n] f32: the window of every row
    seed: int
    leak: tuple = ()  # rows with large values just outside the window

    @property
    def R(self):
        return self.win.shape[0]

    def x(self):
        """[R][V] f32: the windows in a seeded background of the window's own
        scale; the leak rows carry values far above the window's maximum in
        the entries next to it."""
        if self.V == self.n:
            return self.win.copy()
        rng = np.random.default_rng(self.seed)
        x = (5.0 * rng.standard_normal((self.R, self.V))).astype(np.float32)
        for k in self.leak:
            hi = np.float32(np.nanmax(np.where(np.isfinite(self.win[k]), self.win[k], np.nan)))
            if self.t0 > 0:
                x[k, max(0, self.t0 - 3):self.t0] = hi + np.float32(50.0)
            if self.t0 + self.n < self.V:
                x[k, self.t0 + self.n:self.t0 + self.n + 3] = hi + np.float32(50.0)
        x[:, self.t0:self.t0 + self.n] = self.win
        return x


def settle(w):
    """Lifts the row's maximum so that the top-1 / top-2 gap is 0.01 at least
    (far above 16 b_lp, which stays below 2e-4 on these inputs)."""
    top = int(np.argmax(w))
    rest = np.delete(w, top)
    rest = rest[np.isfinite(rest)]
    if rest.size and w[top] - rest.max() < 0.01:
        w[top] = np.float32(rest.max() + np.float32(0.0125))
    return w


def tie_pairs(n):
    """Bit-equal maxima in one lane's two entries, in neighbouring lanes,
    across the two halves and at indices 0 and n - 1."""
    pairs = {"lane": (5, 69), "lanes": (5, 6), "halves": (7, 70), "ends": (0, n - 1),
             "last_two": (n - 2, n - 1)}
    return {k: p for k, p in pairs.items() if 0 <= p[0] < p[1] < n}


def _windows(n, rng):
    """(win [R][n], leak rows): magnitudes, offsets, holes, ties."""
    rows, leak = [], []

    def add(w, is_leak=False):
        if is_leak:
            leak.append(len(rows))
        rows.append(settle(np.asarray(w, np.float32).copy()))

    add(rng.standard_normal(n))
    add(20.0 * rng.standard_normal(n))
    add(rng.uniform(-80.0, 80.0, n))
    add(100.0 + rng.standard_normal(n))   # exp(x) alone would overflow
    add(-120.0 + rng.standard_normal(n))  # ... or vanish
    add(3.0 * rng.standard_normal(n), is_leak=True)
    if n >= 2:
        w = (3.0 * rng.standard_normal(n)).astype(np.float32)
        hole = rng.random(n) < 0.3
        hole[0] = True
        hole[1 + int(np.argmax(w[1:]))] = False  # (a finite entry stays)
        w[hole] = -np.inf
        add(w)
        for keep in (0, n - 1, n // 2):  # every entry but one
            w = np.full(n, -np.inf, np.float32)
            w[keep] = np.float32(rng.standard_normal())
            add(w)
    for a, b in tie_pairs(n).values():
        w = (2.0 * rng.standard_normal(n)).astype(np.float32)
        w[a] = w[b] = np.float32(w.max() + 1.0)
        rows.append(w)  # (not settled: the tie is the point)
    return np.stack(rows), tuple(leak)


N_SIZES = (1, 2, 63, 64, 65, 99, 100, 127, 128)

# the launch-grid case: four rows per workgroup, so R = 3, 4, 5 sit around a
# workgroup and R = 1023, 1024, 1025 around the chip's 256 compute units
GRID_R, GRID_V, GRID_T0, GRID_N = 1025, 131, 17, N_LANG
GRID_PREFIXES = (1, 3, 4, 5, 1023, 1024)

_cases = None


def cases():
    global _cases
    if _cases is None:
        out = []
        for n in N_SIZES:
            shapes = [(n, 0)]
            for V in (51865, 51866):
                shapes += [(V, 0), (V, T0_MODEL), (V, V - n)]
            for V, t0 in shapes:
                seed = 100000 * n + (V % 1000) * 10 + (0 if t0 == 0 else 1 if t0 == T0_MODEL else 2)
                win, leak = _windows(n, np.random.default_rng(seed))
                out.append(Case(f"n{n}_v{V}_t{t0}", V, t0, n, win, seed + 7, leak))
        # one f32 step apart, the larger at the higher index (exempt from
        # margins(): see the module docstring)
        rng = np.random.default_rng(4242)
        rows = []
        for a, b in ((3, 4), (5, 69), (0, N_LANG - 1)):
            w = (0.001 * rng.standard_normal(N_LANG) - 1.0).astype(np.float32)
            w[a] = np.float32(0.01)
            w[b] = np.nextafter(np.float32(0.01), np.float32(1.0))
            rows.append(w)
        out.append(Case("near", 51866, T0_MODEL, N_LANG, np.stack(rows), 4243))
        rng = np.random.default_rng(99)
        win = np.stack([settle((3.0 * rng.standard_normal(GRID_N)).astype(np.float32))
                        for _ in range(GRID_R)])
        out.append(Case("grid", GRID_V, GRID_T0, GRID_N, win, 98, tuple(range(0, GRID_R, 5))))
        _cases = out
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


_refs = {}


def references(c):
    """The float64 reference of every row; computed once per case and shared.
    It reads the window alone."""
    if c.name not in _refs:
        _refs[c.name] = [reference(c.win[k], 0, c.n) for k in range(c.R)]
    return _refs[c.name]
