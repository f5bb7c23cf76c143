"""Plain-numpy float64 reference of the logits-processing stage (k_misc.hip
lp_filter_kernel / lp_probs_kernel / lp_pick_row), the error bounds derived
from the kernels' rounding points, an f32 emulation of the stage in several
summation orders (with named mutants), and the seeded inputs the tests run.
Shared by test_logits_ref.py (CPU) and test_gpu_logits_kernels.py; not a test
module itself and needs no GPU.

Stage contract, per row with active and sample set (any other row is left
unwritten), x the raw logits, T the row's temperature:
  kill_i    the static mask (smask_i < 0), suppress_blank at the initial step
            (eot and " "), the timestamp-pair rule (last two tokens (ts, ts):
            no timestamp; (text, ts): no id below eot), max_initial_ts at the
            initial step (no id above max_initial_tid) and monotonic
            timestamps (has_ts: no id in [beg, beg + seek_delta / 2))
  y_i       f32(x_i / T) for T > 0, else x_i; flt_i = kill_i ? -inf : y_i
  lse       log sum_{not kill} exp(y_i)
  kill_text log sum_{not kill, i >= beg} exp(y_i) > max_{not kill, i < beg} y_i
            (strict; whisper.cpp's order: the logprobs of the timestamps are
            not renormalised afterwards)
  logprob_i (kill_i or (kill_text and i < beg)) ? -inf : y_i - lse
  prob_i    exp(logprob_i), 0 where logprob_i = -inf
  id, tid   argmax prob over all ids / over i >= beg, the lowest index among
            equal f32 probabilities, 0 when no probability is > 0
  p, plog   prob_id, logprob_id
  ptsum     sum_{i >= beg} prob_i;  pt = prob_tid / (ptsum + 1e-10)
  nosp      want_nosp: softmax(x)[nosp_id] over the raw, untempered, unmasked
            logits; else 0
(the host, not this stage, sets tid = id and pt = p for id >= beg).

Exact quantities: the -inf positions of flt, its surviving values (one IEEE
division: the build has no fast-math and -ffp-contract=off), the -inf
positions of logprobs (so the kill_text decision), id, tid, and which rows
were written. Exact *decisions* need inputs that settle them: see margins().

Bounded quantities. u = 2^-24 (f32 unit roundoff), E = 3 ulp = 6 u (the
error allowed to expf and logf: OpenCL's full-profile limit, which covers the
device library's documented 1 ulp), w_i = exp(y_i - lse) the true weights,
M = max y. The kernel forms, per survivor, expf(y_i - m_g) in its chunk g
(m_g the chunk maximum), sums 13 of them per thread, 64 threads per wave
through a 6-level tree, the 4 waves as (a + b) + (c + d), and the 16 chunk
sums s_g in index order as s_g * expf(m_g - M). Rounding points of S, as
relative errors of term i:
  the two f32 subtractions y_i - m_g and m_g - M: u (|y_i - m_g| + |m_g - M|)
      = u (M - y_i) on the exponent, so the same on the term;
  the two expf: 2 E;  the product s_g * expf(.): u;
  the additions: every term passes through at most D = 13 + 6 + 2 + 16 = 37
      of them: D u. (Another summation order has another D: pairwise
      ceil(log2 n), sequential n - 1; sum_depth() gives it. The kernel, its
      own order and the pairwise order are held to D = 37. Sequential f32
      summation cannot be: each of its n - 1 additions rounds the whole
      running sum, and on these inputs it lands up to 12.5 times outside the
      D = 37 bound (69 rows over it). It is held to the formula at its own
      depth, which for n near 50000 constrains little beyond the exact
      quantities; the CPU oracle, which sums that way, likewise.)
  rel_S   = sum_i w_i (u (M - y_i) + 2 E + u) + D u + V 2^-126
      (the last term: expf results in the subnormal range or flushed)
  err_lse = rel_S + E |lse - M| + u |lse|           (logf(S); logf(S) + M)
  b_lp_i  = err_lse + u (|logprob_i| + err_lse)     (y_i - lse)
  b_p_i   = prob_i (expm1(b_lp_i) + E) + 2^-126     (expf; a result below
      FLT_MIN may be rounded to a subnormal or flushed to zero)
  plog, p: b_lp and b_p at id
  b_ptsum = sum_{i >= beg} b_p_i + u ptsum          (double sum of f32
      probabilities, rounded to f32 once)
  b_pt    = b_p_tid / (ptsum - b_ptsum + c) + prob_tid b_ptsum /
            ((ptsum - b_ptsum + c) (ptsum + c)) + u pt,  c = 1e-10
  b_nosp  = as b_p, from the err_lse of the raw logits
Second-order terms (u^2) are dropped: they are below 1e-12 of each bound.

The condition on the inputs (margins()): apart from bit-equal ties, which the
lowest index settles, and the constructed timestamp-mass ties, every discrete
decision (top-1 / top-2, best / second timestamp, timestamp mass / best
text) has a margin of at least 16 max_i b_lp_i in log units, and no deciding
probability lies where expf leaves the normal range (logprob in [-106, -87]).
The constructed mass ties (one surviving timestamp bit-equal to the best
text logit, or one ulp off) are decided by two f32 subtractions of the same
lse; they are exact when lse / 2 <= y <= 2 lse (Sterbenz), which margins()
asserts for them.
"""
from dataclasses import dataclass

import numpy as np

import mwx

LP_G, LP_CHUNK, LP_T, LP_NPT = 16, 3328, 256, 13
MAX_VOCAB = LP_G * LP_CHUNK
U = 2.0 ** -24
E = 6.0 * U
FLT_MIN = 2.0 ** -126
KERNEL_DEPTH = 13 + 6 + 2 + 16
MARGIN = 16.0
P_NORMAL, P_ZERO = -87.0, -106.0   # logprob above: a normal f32 prob; below: expf gives 0

CTL = mwx.LOGITS_CTL   # the hook's row record (RowCtl as plain ints plus the temperature)
REC = ("id", "tid", "p", "plog", "pt", "ptsum", "nosp")

# whisper.cpp v1.8.2 non_speech_tokens (suppress_nst)
NST = ["\"", "#", "(", ")", "*", "+", "/", ":", ";", "<", "=", ">", "@", "[", "\\", "]", "^",
       "_", "`", "{", "|", "}", "~", "「", "」", "『", "』", "<<", ">>", "<<<", ">>>", "--",
       "---", "-(", "-[", "('", "(\"", "((", "))", "(((", ")))", "[[", "]]", "{{", "}}", "♪♪",
       "♪♪♪", "♩", "♪", "♫", "♬", "♭", "♮", "♯"]
N_LANG = 100


@dataclass(frozen=True)
class LC:
    """The kernels' LogitsConst."""
    n_vocab: int
    eot: int
    beg: int
    space_id: int
    suppress_blank: int
    max_initial_tid: int
    nosp_id: int


def ctl_row(active=1, sample=1, is_initial=0, last_ts=0, penult_ts=0, has_ts=0, seek_delta=0,
            want_probs=1, want_nosp=0, temperature=0.0):
    return (active, sample, is_initial, last_ts, penult_ts, has_ts, seek_delta, want_probs,
            want_nosp, temperature)


def ctl_of_history(hist, beg):
    """RowCtl rule fields of a decoder whose sampled tokens are hist (the
    whisper_full token loop: has_ts / seek_delta are set by ids > beg)."""
    has_ts, sd = 0, 3000
    for t in hist:
        if t > beg:
            has_ts, sd = 1, 2 * (t - beg)
    return dict(is_initial=int(not hist), last_ts=int(bool(hist) and hist[-1] >= beg),
                penult_ts=int(len(hist) < 2 or hist[-2] >= beg), has_ts=has_ts, seek_delta=sd)


def static_mask(V, sp, *, nst_ids=(), suppress_nst=False, no_timestamps=False, tdrz=False,
                bench_fixed_steps=0):
    """whisper_process_logits' unconditional suppressions for a vocabulary
    with the special ids sp (eot, sot, translate, transcribe, solm, prev, nosp,
    not, beg): 0 or -inf per id."""
    m = np.zeros(V, np.float32)
    kill = {sp["not"], sp["sot"], sp["nosp"], sp["translate"], sp["transcribe"], sp["prev"]}
    if not tdrz:
        kill.add(sp["solm"])
    kill.update(t for t in (sp["sot"] + 1 + i for i in range(N_LANG)) if t < V)
    if suppress_nst:
        kill.update(nst_ids)
    if bench_fixed_steps > 0:
        kill.add(sp["eot"])
    m[sorted(kill)] = -np.inf
    if no_timestamps or bench_fixed_steps > 0:
        m[sp["beg"]:] = -np.inf
    return m


def oracle_vocab(o):
    """(special ids, suppress_nst ids, id of " ") of an orc.Oracle's vocabulary."""
    tok2id = {}
    for i in range(o.eot):
        tok2id.setdefault(o.token_bytes(i), i)
    sp = dict(eot=o.eot, sot=o.sot, translate=o.translate, transcribe=o.transcribe, solm=o.solm,
              prev=o.prev, nosp=o.nosp, beg=o.beg)
    sp["not"] = o.not_
    nst = [tok2id[w.encode()] for t in NST for w in (t, " " + t) if w.encode() in tok2id]
    nst += [tok2id[w] for w in (b" -", b" '") if w in tok2id]
    return sp, nst, tok2id[b" "]


def kill_mask(smask, c, lc):
    """The rule's mask decisions for one row (True: suppressed)."""
    V = lc.n_vocab
    i = np.arange(V)
    kill = np.asarray(smask) < 0
    if c["is_initial"] and lc.suppress_blank:
        kill = kill | (i == lc.eot) | (i == lc.space_id)
    if c["last_ts"]:
        kill = kill | ((i >= lc.beg) if c["penult_ts"] else (i < lc.eot))
    if c["is_initial"] and lc.max_initial_tid >= 0:
        kill = kill | (i > lc.max_initial_tid)
    if c["has_ts"]:
        kill = kill | ((i >= lc.beg) & (i < lc.beg + int(c["seek_delta"]) // 2))
    return kill


def tempered(x, c):
    x = np.asarray(x, np.float32)
    t = np.float32(c["temperature"])
    return (x / t).astype(np.float32) if t > 0 else x


def _lse64(y):
    """(lse, M) of the float64 values y (non-empty)."""
    M = y.max()
    return float(np.log(np.exp(y - M).sum()) + M), float(M)


def _err_lse(y, depth, V):
    """(lse, err_lse) of the survivors y (float64, non-empty): the docstring's terms."""
    lse, M = _lse64(y)
    w = np.exp(y - lse)
    rel_s = float((w * (U * (M - y) + 2 * E + U)).sum()) + depth * U + V * FLT_MIN
    return lse, rel_s + E * abs(lse - M) + U * abs(lse)


def reference(x, smask, c, lc, depth=KERNEL_DEPTH):
    """The float64 reference of one row and its bounds. Returns a dict; for a
    row the kernel does not write, {"written": False}."""
    if not (c["active"] and c["sample"]):
        return {"written": False}
    V, beg = lc.n_vocab, lc.beg
    kill = kill_mask(smask, c, lc)
    y32 = tempered(x, c)
    flt = np.where(kill, np.float32(-np.inf), y32).astype(np.float32)
    y = y32.astype(np.float64)
    live = ~kill
    ts = np.arange(V) >= beg
    r = {"written": True, "kill": kill, "flt": flt, "depth": depth,
         "want_probs": bool(c["want_probs"])}
    lp = np.full(V, -np.inf)
    b_lp = np.zeros(V)
    kill_text, mass_margin = False, np.inf
    if live.any():
        lse, err = _err_lse(y[live], depth, V)
        lts, ltx = live & ts, live & ~ts
        if lts.any():
            ts_mass = _lse64(y[lts])[0]
            tx_max = y[ltx].max() if ltx.any() else -np.inf
            kill_text = bool(ts_mass > tx_max)
            mass_margin = abs(ts_mass - tx_max)
        fin = live & ~(kill_text & ~ts)
        lp[fin] = y[fin] - lse
        b_lp[fin] = err + U * (np.abs(lp[fin]) + err)
        r["lse"], r["err_lse"] = lse, err
    p = np.where(np.isfinite(lp), np.exp(np.where(np.isfinite(lp), lp, 0.0)), 0.0)
    b_p = p * (np.expm1(b_lp) + E) + FLT_MIN
    r.update(kill_text=kill_text, mass_margin=mass_margin, lp=lp, b_lp=b_lp, p=p, b_p=b_p)

    def argmax_lowest(sel):
        """(index, margin to the next distinct value, its logprob): lowest
        index among the bit-equal maxima of the selection; 0 if it is empty or
        its best probability underflows to zero."""
        idx = np.nonzero(sel & np.isfinite(lp))[0]
        if idx.size == 0:
            return 0, np.inf, -np.inf
        v = lp[idx]
        top = v.max()
        rest = v[y32[idx] != y32[idx[int(v.argmax())]]]
        gap = top - rest.max() if rest.size else np.inf
        if top < P_ZERO:
            return 0, np.inf, top
        return int(idx[int(v.argmax())]), gap, top   # argmax: the first, so the lowest index

    r["id"], r["gap_id"], r["top_lp"] = argmax_lowest(np.ones(V, bool))
    r["tid"], r["gap_tid"], r["top_ts_lp"] = argmax_lowest(ts)
    sum_ts = float(p[ts].sum())
    b_sum = float(b_p[ts].sum()) + U * sum_ts if ts.any() else 0.0
    ptid = p[r["tid"]] if np.isfinite(r["top_ts_lp"]) and r["top_ts_lp"] >= P_ZERO else 0.0
    b_ptid = b_p[r["tid"]] if ptid > 0 else FLT_MIN
    cc = 1e-10
    lo = sum_ts - b_sum + cc
    pt = ptid / (sum_ts + cc)
    r["rec"] = {"id": r["id"], "tid": r["tid"], "p": p[r["id"]], "plog": lp[r["id"]],
                "pt": pt, "ptsum": sum_ts, "nosp": 0.0}
    r["b_rec"] = {"p": b_p[r["id"]], "plog": b_lp[r["id"]],
                  "pt": b_ptid / lo + ptid * b_sum / (lo * (sum_ts + cc)) + U * pt,
                  "ptsum": b_sum + FLT_MIN, "nosp": 0.0}
    if c["want_nosp"]:
        x64 = np.asarray(x, np.float64)
        rlse, rerr = _err_lse(x64, depth, V)
        d = x64[lc.nosp_id] - rlse
        r["rec"]["nosp"] = float(np.exp(d))
        r["b_rec"]["nosp"] = float(np.exp(d) * (np.expm1(rerr + U * (abs(d) + rerr)) + E) + FLT_MIN)
    return r


def margins(r, x, c, lc, mass_tie=False):
    """Asserts the condition on the inputs for one written row: every discrete
    decision is settled by the reference alone (module docstring)."""
    fin = np.isfinite(r["lp"])
    need = MARGIN * (float(r["b_lp"][fin].max()) if fin.any() else 0.0)
    # (a mass tie's text and timestamp logprobs differ by exactly one ulp of
    # the logit, see below: two expf within E of the truth keep their order
    # when the gap exceeds 2 E)
    assert r["gap_id"] >= (2.02 * E if mass_tie else need), ("top-1 / top-2", r["gap_id"], need)
    assert r["gap_tid"] >= need, ("timestamp best / second", r["gap_tid"], need)
    for top in (r["top_lp"], r["top_ts_lp"]):
        assert not (P_ZERO <= top <= P_NORMAL), ("deciding probability near underflow", top)
    if mass_tie:
        kill = r["kill"]
        y = tempered(x, c).astype(np.float64)
        ts = np.arange(lc.n_vocab) >= lc.beg
        assert int((~kill & ts).sum()) == 1, "a constructed mass tie has one timestamp"
        for v in (y[~kill & ts].max(), y[~kill & ~ts].max()):
            assert r["lse"] / 2 <= v <= 2 * r["lse"], ("Sterbenz", v, r["lse"])
    else:
        assert r["mass_margin"] >= need, ("timestamp mass / best text", r["mass_margin"], need)


# ------------------------------------------------------------------ emulation

def _shift(v, ulp):
    for _ in range(abs(ulp)):
        v = np.nextafter(v, np.float32(np.inf if ulp > 0 else -np.inf))
    return v


def exp32(a, ulp=0):
    """expf: correctly rounded, then moved by `ulp` f32 steps (an expf that
    errs by up to |ulp| + 1/2 ulp in one direction)."""
    a = np.asarray(a, np.float32)
    with np.errstate(under="ignore"):
        v = np.exp(a.astype(np.float64)).astype(np.float32)
    return np.where(v > 0, _shift(v, ulp), v).astype(np.float32) if ulp else v


def log32(a, ulp=0):
    a = np.asarray(a, np.float32)
    with np.errstate(divide="ignore"):
        v = np.log(a.astype(np.float64)).astype(np.float32)
    return np.where(np.isfinite(v) & (v != 0), _shift(v, ulp), v).astype(np.float32) if ulp else v


def _sum_seq(e):
    return np.cumsum(e, dtype=np.float32)[-1] if e.size else np.float32(0)


def _sum_pair(e):
    n = 1
    while n < max(e.size, 1):
        n *= 2
    v = np.zeros(n, np.float32)
    v[:e.size] = e
    while v.size > 1:
        v = (v[:v.size // 2] + v[v.size // 2:]).astype(np.float32)
    return v[0]


def _sum_chunk(e):
    """One chunk's [LP_CHUNK] terms as the workgroup sums them: thread t owns
    t + 256 k; 13 sequential additions, the xor butterfly, the 4 wave slots."""
    a = e.reshape(LP_NPT, LP_T)
    s = a[0].copy()
    for k in range(1, LP_NPT):
        s = (s + a[k]).astype(np.float32)
    w = s.reshape(4, 64)
    while w.shape[1] > 1:
        h = w.shape[1] // 2
        w = (w[:, :h] + w[:, h:]).astype(np.float32)
    w = w[:, 0]
    return np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3]))


def sum_depth(order, n):
    """The longest chain of f32 additions of a summation order over n terms."""
    if order == "chunked":
        return KERNEL_DEPTH
    if order == "pairwise":
        return max(1, int(np.ceil(np.log2(max(n, 2)))))
    return max(1, n - 1)


MUTANTS = ("drop_chunk", "chunk_max", "plog_no_lse", "tie_high", "mass_ge", "split_gt",
           "pad_text", "temp_after")
NEG = np.float32(-np.inf)


def _lse32(v, sel, order, ulp, mutant=None, pad=None):
    """f32 (S, M) of the entries v[sel] (v = -inf elsewhere) in a summation
    order. pad = (count, value): mutant pad_text's extra terms."""
    vv = np.where(sel, v, NEG).astype(np.float32)
    if order != "chunked":
        M = vv.max() if vv.size else NEG
        if M == NEG:
            return np.float32(0), NEG
        live = vv > NEG
        e = exp32((vv[live] - M).astype(np.float32), ulp)
        return (_sum_seq(e) if order == "sequential" else _sum_pair(e)), M
    full = np.full(MAX_VOCAB, NEG, np.float32)
    full[:vv.size] = vv
    if pad is not None and pad[0] > 0:
        full[vv.size:] = pad[1]
    ch = full.reshape(LP_G, LP_CHUNK)
    m = ch.max(axis=1)
    M = m.max()
    S = np.float32(0)
    for g in range(LP_G):
        if m[g] == NEG or (mutant == "drop_chunk" and g == 1):
            continue
        live = ch[g] > NEG
        e = np.where(live, exp32(np.where(live, ch[g] - m[g], 0).astype(np.float32), ulp),
                     np.float32(0)).astype(np.float32)
        sc = np.float32(1) if (mutant == "chunk_max" and g == 1) else \
            exp32(np.float32(m[g] - M), ulp)
        S = np.float32(S + np.float32(_sum_chunk(e) * sc))
    return S, M


def emulate(x, smask, c, lc, order="chunked", mutant=None, ulp=0):
    """The stage in f32 as a correct kernel may compute it: the summation
    order `order` (sequential, chunked = the kernel's, pairwise), expf / logf
    off by `ulp` steps in one direction. mutant: one of MUTANTS, a kernel that
    is subtly wrong. Returns None for an unwritten row, else (flt, probs,
    logprobs, rec dict); probs / logprobs are None without want_probs."""
    if not (c["active"] and c["sample"]):
        return None
    V, beg = lc.n_vocab, lc.beg
    x = np.asarray(x, np.float32)
    i = np.arange(V)
    ts = (i > beg) if mutant == "split_gt" else (i >= beg)
    kill = kill_mask(smask, c, lc)
    y = tempered(x, c)
    flt = np.where(kill, NEG, y).astype(np.float32)
    rule_v = np.where(kill, NEG, x).astype(np.float32) if mutant == "temp_after" else flt
    live = flt > NEG
    pad = None
    if mutant == "pad_text":
        pad = (MAX_VOCAB - V, flt[V - 1])
    S, M = _lse32(flt, live, order, ulp, mutant, pad)
    with np.errstate(invalid="ignore"):
        lse = np.float32(log32(S, -ulp) + M)
    if mutant == "temp_after":
        S_r, M_r = _lse32(rule_v, live, order, ulp)
        with np.errstate(invalid="ignore"):
            lse_r = np.float32(log32(S_r, -ulp) + M_r)
    else:
        lse_r = lse
    Sts, Mts = _lse32(rule_v, live & ts, order, ulp)
    tx = rule_v[live & ~ts]
    Mtext = tx.max() if tx.size else NEG
    if pad is not None and pad[0] > 0:
        Mtext = max(Mtext, pad[1])
    ts_lp = np.float32(np.float32(log32(Sts, ulp) + Mts) - lse_r) if Sts > 0 else NEG
    txmax = np.float32(Mtext - lse_r) if Mtext > NEG else NEG
    kill_text = bool(ts_lp >= txmax) if mutant == "mass_ge" else bool(ts_lp > txmax)
    dead = ~live | (kill_text & ~ts)
    with np.errstate(invalid="ignore"):
        lp = np.where(dead, NEG, (flt - lse).astype(np.float32)).astype(np.float32)
    p = np.where(dead, np.float32(0), exp32(np.where(dead, 0, lp).astype(np.float32), ulp))
    p = p.astype(np.float32)

    def pick(sel):
        idx = np.nonzero(sel)[0]
        if idx.size == 0 or p[idx].max() <= 0:
            return 0, np.float32(0)
        q = p[idx]
        k = (q.size - 1 - int(q[::-1].argmax())) if mutant == "tie_high" else int(q.argmax())
        return int(idx[k]), q[k]

    bid, best = pick(np.ones(V, bool))
    tid, tbest = pick(ts)
    sum_ts = float(p[ts].astype(np.float64).sum())
    plog = flt[bid] if mutant == "plog_no_lse" else \
        (NEG if (flt[bid] == NEG or (kill_text and not ts[bid])) else np.float32(flt[bid] - lse))
    rec = {"id": bid, "tid": tid, "p": best, "plog": plog,
           "pt": np.float32(float(tbest) / (sum_ts + 1e-10)), "ptsum": np.float32(sum_ts),
           "nosp": np.float32(0)}
    if c["want_nosp"]:
        RS, RM = _lse32(x, np.ones(V, bool), order, ulp)
        rlse = np.float32(log32(RS, -ulp) + RM)
        rec["nosp"] = exp32(np.float32(x[lc.nosp_id] - rlse), ulp)
    if not c["want_probs"]:
        return flt, None, None, rec
    return flt, p, lp, rec


# ------------------------------------------------------------------ comparison

def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(r, got, ratios=None):
    """One row of a kernel (or emulation) against reference r. got: None for
    an unwritten row, else (flt, probs, logprobs, rec), probs / logprobs None
    when the row carries none. Returns the list of violated checks (empty: the
    row passes); ratios (a dict) collects the worst |err| / bound per quantity."""
    bad = []
    if not r["written"]:
        return [] if got is None else ["row written"]
    if got is None:
        return ["row not written"]
    flt, probs, lps, rec = got
    if not np.array_equal(np.isneginf(flt), r["kill"]):
        bad.append("flt -inf set")
    elif not np.array_equal(bits(flt)[~r["kill"]], bits(r["flt"])[~r["kill"]]):
        bad.append("flt values")

    def bounded(name, g, ref, bound):
        g = np.asarray(g, np.float64)
        if not np.isfinite(g).all():
            bad.append(name + " not finite")
            return
        q = float(np.max(np.abs(g - ref) / bound)) if g.size else 0.0
        if ratios is not None:
            ratios[name] = max(ratios.get(name, 0.0), q)
        if q > 1.0:
            bad.append(f"{name} {q:.3g} x bound")

    if r["want_probs"] != (probs is not None):
        bad.append("probs rows")
    elif probs is not None:
        dead = ~np.isfinite(r["lp"])
        if not np.array_equal(np.isneginf(lps), dead):
            bad.append("logprobs -inf set (kill_text)")
        else:
            bounded("logprobs", lps[~dead], r["lp"][~dead], r["b_lp"][~dead])
        if (probs[dead] != 0).any():
            bad.append("probs of masked ids")
        bounded("probs", probs, r["p"], r["b_p"])
    for k in ("id", "tid"):
        if int(rec[k]) != r["rec"][k]:
            bad.append(f"{k} {int(rec[k])} != {r['rec'][k]}")
    for k in ("p", "plog", "pt", "ptsum", "nosp"):
        ref = r["rec"][k]
        if np.isneginf(ref) or r["b_rec"][k] == 0.0:
            if float(rec[k]) != ref:
                bad.append(f"{k} {float(rec[k])} != {ref}")
        else:
            bounded(k, np.float64(rec[k]), ref, r["b_rec"][k])
    return bad


# ------------------------------------------------------------------ inputs

@dataclass
class Case:
    name: str
    lc: LC
    smask: np.ndarray      # [V]
    x: np.ndarray          # [R][V] f32
    ctl: np.ndarray        # [R] of CTL
    mass_tie: tuple = ()   # rows that are constructed timestamp-mass ties

    @property
    def R(self):
        return self.x.shape[0]


def _layout(V, beg=None, eot=None):
    """A LogitsConst for a made-up vocabulary of V ids: eot, " " and nosp in
    different places, beg at 3/4 unless given."""
    beg = (3 * V) // 4 if beg is None else beg
    eot = max(0, min(beg, V) - 1 - min(beg, V) // 8) if eot is None else eot
    return LC(V, eot, beg, min(V - 1, V // 5), 1, -1, min(V - 1, eot + 1 if eot + 1 < beg else 0))


def _settle(x, smask, c, lc, mass_tie=False):
    """Moves the deciding logits of a seeded row apart until the reference
    alone settles every decision (margins()); the row is changed, never
    dropped."""
    x = np.array(x, np.float32)
    V, beg = lc.n_vocab, lc.beg
    ts = np.arange(V) >= beg
    t = np.float32(c["temperature"]) if c["temperature"] > 0 else np.float32(1)
    if mass_tie or not (c["active"] and c["sample"]):   # constructed bit for bit: only checked
        if c["active"] and c["sample"]:
            margins(reference(x, smask, c, lc), x, c, lc, True)
        return x
    for _ in range(12):
        r = reference(x, smask, c, lc)
        try:
            margins(r, x, c, lc, mass_tie)
            return x
        except AssertionError as e:
            what = e.args[0][0]
        fin = np.isfinite(r["lp"])
        step = np.float32(max(1.0, 64 * MARGIN * float(r["b_lp"][fin].max()))) * t
        live = ~r["kill"]
        if what.startswith("top-1"):
            x[r["id"]] += step
        elif what.startswith("timestamp best"):
            x[r["tid"]] += step
        elif what.startswith("timestamp mass"):
            tx = np.nonzero(live & ~ts)[0]
            x[tx[int(x[tx].argmax())]] += 2 * step
        else:   # a deciding probability near underflow: lift the best timestamp
            tsl = np.nonzero(live & ts)[0]
            x[tsl[int(x[tsl].argmax())]] += np.float32(40) * t
    raise AssertionError("input not settled")


STATES = [dict(is_initial=1, last_ts=0, penult_ts=1, has_ts=0)] + \
    [dict(is_initial=0, last_ts=a, penult_ts=b, has_ts=h)
     for a in (0, 1) for b in (0, 1) for h in (0, 1)]
TEMPS = (0.0, 0.2, 1.0, 0.7)


def _seek_deltas(V, beg):
    """0, 1, 2, odd, the last timestamp, beyond the end."""
    n = max(V - beg, 1)
    return (0, 1, 2, 7, 2 * (n - 1), 2 * n + 10)


# the four has_ts states, then two of them again: six has_ts rows per case, one
# for each seek_delta
STATES_SD = STATES + [STATES[2], STATES[6]]


def _rows(name, lc, smask, rng, states, scale=3.0, extra=None, inactive=True):
    """One row per state (seek_delta, temperature, want_probs and want_nosp
    cycling), seeded normal logits with a lifted text id and a lifted
    timestamp, unwritten rows in between."""
    V = lc.n_vocab
    xs, cs = [], []
    sds = _seek_deltas(V, lc.beg)
    n_has = 0   # seek_delta cycles over the has_ts rows alone, so every value occurs
    for k, st in enumerate(states):
        c = dict(zip(CTL.names, ctl_row(**st)))
        c["seek_delta"] = sds[n_has % len(sds)] if st["has_ts"] else 3000
        n_has += st["has_ts"]
        c["temperature"] = TEMPS[k % len(TEMPS)]
        c["want_probs"] = int(k % 3 != 2)
        c["want_nosp"] = int(k % 2 == 0)
        t = c["temperature"] if c["temperature"] > 0 else 1.0
        x = (rng.normal(0.0, scale, V) * t).astype(np.float32)
        x[int(rng.integers(0, V))] += np.float32(6 * t)
        if lc.beg < V:
            x[int(rng.integers(lc.beg, V))] += np.float32(5 * t)
        if extra is not None:
            extra(x, k)
        xs.append(_settle(x, smask, c, lc))
        cs.append(tuple(c[n] for n in CTL.names))
        if inactive and k % 4 == 1:   # a row the launch must leave alone
            xs.append(rng.normal(0.0, scale, V).astype(np.float32))
            off = dict(c)
            off["active" if k % 8 == 1 else "sample"] = 0
            cs.append(tuple(off[n] for n in CTL.names))
    return Case(name, lc, smask, np.stack(xs), np.array(cs, CTL))


def _mk(name, lc, smask, rows, mass_tie=()):
    """rows: [(x, ctl dict)]; every written row is settled."""
    xs, cs = [], []
    for k, (x, kw) in enumerate(rows):
        c = dict(zip(CTL.names, ctl_row(**kw)))
        xs.append(_settle(x, smask, c, lc, k in mass_tie))
        cs.append(tuple(c[n] for n in CTL.names))
    return Case(name, lc, smask, np.stack(xs), np.array(cs, CTL), tuple(mass_tie))


# bit-equal maxima at two ids (rows of the tie_* cases, in this order; tie_tid
# shifts them by TIE_TID_OFF and leaves the last out)
TIE_V = 2 * LP_CHUNK + 40
TIE_PAIRS = {"lanes": (5, 6), "waves": (5, 70), "slots": (5, 5 + LP_T),
             "chunks": (5, LP_CHUNK + 5), "chunk_edge": (LP_CHUNK - 1, LP_CHUNK),
             "last_id": (6, TIE_V - 1)}
TIE_TID_OFF = 100


def tie_place(i):
    """(chunk, slot of the 13, wave, lane) that handles vocabulary id i."""
    off = i % LP_CHUNK
    return i // LP_CHUNK, off // LP_T, (off % LP_T) // 64, off % 64


VOCAB_SIZES = (1, 255, 256, 257, 3327, 3328, 3329, 6656, 6657, 51864, 51865, 51866, 53247, 53248)
REAL = {51864: (50363, 50256), 51865: (50364, 50257), 51866: (50365, 50257)}
_cache = {}


def cases():
    """Every shared input, built once."""
    if "all" in _cache:
        return _cache["all"]
    out = []
    rng = np.random.default_rng(20240607)
    zeros = lambda V: np.zeros(V, np.float32)   # noqa: E731

    # vocabulary sizes: every chunk edge, the real layouts, the largest size
    for V in VOCAB_SIZES:
        if V in REAL:
            beg, eot = REAL[V]
            lc = LC(V, eot, beg, 220, 1, beg + 50, eot + 105)
            sm = zeros(V)
            sm[[eot + 1, eot + 104, eot + 105, eot + 106]] = -np.inf
            st = [STATES[0], STATES[1], STATES[6], STATES[4], STATES[8]]
        else:
            lc = _layout(V) if V > 1 else LC(1, 0, 0, 0, 0, -1, 0)
            sm = zeros(V)
            if V > 300:
                sm[rng.integers(0, V, 20)] = -np.inf
            st = [STATES[1], STATES[6]] if V > 1 else [STATES[1]]
            if V > 3000:
                st = [STATES[0], STATES[1], STATES[6], STATES[2]]
        out.append(_rows(f"V{V}", lc, sm, rng, st, inactive=V > 3000 and V < 10000))

    # beg / eot placement, every rule state, seek_delta and max_initial_tid
    V = 3 * LP_CHUNK + 100
    mits = (-1, None, None, V - 1, V + 10)
    for k, beg in enumerate((LP_CHUNK, LP_CHUNK - 1, LP_CHUNK + 1, 2 * LP_CHUNK, 3 * LP_CHUNK + 50,
                             V, None)):
        eot = 5000 if beg is None else (min(beg, V) - 1 - 1700) % min(beg, V)
        b = eot + 1 if beg is None else beg
        mit = mits[k % len(mits)]
        mit = (b if k % 2 else b + 50) if mit is None else mit
        lc = LC(V, eot, b, (eot + LP_CHUNK + 7) % min(b, V), int(k != 2), mit, (eot + 3) % V)
        sm = zeros(V)
        sm[rng.integers(0, V, 30)] = -np.inf
        out.append(_rows(f"beg{b}", lc, sm, rng, STATES_SD))
    b = 2 * LP_CHUNK + 11
    for mit in (-1, b, b + 50, V - 1, V + 10):   # initial rows under every cap
        lc = LC(V, b - 400, b, 17, 1, mit, b - 3)

        def late(x, k, b=b):
            x[b + 60 + k] += np.float32(9)   # a strong timestamp the cap may or may not allow
        out.append(_rows(f"mit{mit}", lc, zeros(V), rng, [STATES[0]] * 3, extra=late,
                         inactive=False))

    # chunk structure
    V = 4 * LP_CHUNK + 77
    lc = LC(V, 2 * LP_CHUNK - 9, 2 * LP_CHUNK, 3, 1, -1, 11)    # chunks 0, 1 text; 2, 3, 4 ts
    plain = dict(is_initial=0, last_ts=0, penult_ts=0, has_ts=0, want_nosp=1)
    g = lambda s=3.0: rng.normal(0.0, s, V).astype(np.float32)   # noqa: E731

    def spike(at, h=9.0):
        x = g()
        x[at] += np.float32(h)
        return x
    sm = zeros(V)
    sm[LP_CHUNK:2 * LP_CHUNK] = -np.inf
    out.append(_mk("chunk_masked", lc, sm, [(g(), plain), (spike(5), plain)]))
    sm = zeros(V)
    sm[lc.beg:] = -np.inf
    out.append(_mk("no_timestamps", lc, sm, [(g(), plain), (spike(V - 1), plain)]))
    sm = zeros(V)
    sm[:lc.beg] = -np.inf
    out.append(_mk("no_text", lc, sm, [(g(), plain), (spike(lc.beg), plain)]))
    for at in (0, LP_CHUNK + 1, 3 * LP_CHUNK - 1, V - 1):
        sm = np.full(V, -np.inf, np.float32)
        sm[at] = 0
        out.append(_mk(f"one_survivor_{at}", lc, sm, [(g(), plain)]))
    out.append(_mk("max_place", lc, zeros(V),
                   [(spike(at, 12.0), dict(plain, temperature=t))
                    for at, t in ((7, 0.0), (LP_CHUNK + 300, 0.7), (2 * LP_CHUNK + 5, 1.0),
                                  (4 * LP_CHUNK + 3, 0.2), (V - 1, 0.0), (V - 1, 0.7))]))

    # magnitudes
    V = 2 * LP_CHUNK + 1
    lc = LC(V, 3000, 5000, 40, 1, -1, 3001)
    flat = np.full(V, 1.25, np.float32)
    hot_tx, hot_ts = np.full(V, -80, np.float32), np.full(V, -80, np.float32)
    hot_tx[LP_CHUNK + 9] = 80
    hot_ts[V - 1] = 80
    far = g()[:V] * np.float32(0.5)
    far[LP_CHUNK:2 * LP_CHUNK] -= 120          # chunk maxima more than 100 apart
    far[2 * LP_CHUNK:] -= 240
    far2 = far[::-1].copy()
    big = (rng.normal(0.0, 1.0, V) * 1e4).astype(np.float32)
    out.append(_mk("magnitudes", lc, zeros(V),
                   [(flat, plain), (flat, dict(plain, temperature=0.7)), (hot_tx, plain),
                    (hot_ts, plain), (far, plain), (far2, dict(plain, temperature=0.7)),
                    (big, dict(plain, temperature=0.2)),
                    (big[::-1].copy(), dict(plain, temperature=0.2, last_ts=1))]))
    V = 51866
    lc = LC(V, 50257, 50365, 220, 1, -1, 50363)
    big = (rng.normal(0.0, 1.0, V) * 1e4).astype(np.float32)
    out.append(_mk("magnitudes_v3", lc, zeros(V),
                   [(np.full(V, -3.5, np.float32), plain), (big, dict(plain, temperature=0.2))]))

    # the timestamp-mass rule
    V = 3 * LP_CHUNK + 5
    lc = LC(V, 2000, LP_CHUNK + 10, 50, 1, -1, 2001)
    base = np.full(V, -20, np.float32)
    base += (rng.normal(0.0, 0.5, V)).astype(np.float32)
    one_ts = zeros(V)
    one_ts[lc.beg:] = -np.inf
    one_ts[2 * LP_CHUNK + 3] = 0               # one surviving timestamp, in another chunk

    def tie(d, tx_at=LP_CHUNK - 2):
        x = base.copy()
        x[tx_at] = 16.0
        v = np.float32(16.0)
        x[2 * LP_CHUNK + 3] = _shift(v, d) if d else v
        return x
    out.append(_mk("mass_tie", lc, one_ts, [(tie(0), plain), (tie(1), plain), (tie(-1), plain),
                                            (tie(0, 7), plain)], mass_tie=(0, 1, 2, 3))
               )

    def spread(tx, tsv, n):
        x = base.copy()
        x[LP_CHUNK - 2] = tx
        x[rng.choice(np.arange(lc.beg, V), n, replace=False)] = tsv
        return x
    out.append(_mk("mass_spread", lc, zeros(V),
                   [(spread(5.0, 1.0, 400), plain),                          # log 400 + 1 > 5
                    (spread(9.0, 1.0, 400), plain),                          # < 9
                    (spread(5.0, 1.0, 400), dict(plain, temperature=0.2)),   # 25 > log 400 + 5
                    (spread(1.2, 0.2, 400) * np.float32(0.2), dict(plain, temperature=0.2))]))

    # argmax ties: two lanes, two waves, two slots of a thread, two chunks
    V = TIE_V
    pairs = tuple(TIE_PAIRS.values())

    def tied(off, a, b, h=7.0):
        x = g()[:V] * np.float32(0.3)
        x[off + a] = x[off + b] = np.float32(h)
        return x
    lc = LC(V, 10, V, 20, 0, -1, 11)           # no timestamp: ties among text
    out.append(_mk("tie_text", lc, zeros(V), [(tied(0, a, b), plain) for a, b in pairs]))
    lc = LC(V, 0, 0, 0, 0, -1, 0)              # timestamps only: id and tid tie alike
    out.append(_mk("tie_ts", lc, zeros(V), [(tied(0, a, b), plain) for a, b in pairs]))
    lc = LC(V, 10, TIE_TID_OFF, 20, 0, -1, 11)  # a text maximum, ties among the timestamps
    rows = []
    for a, b in pairs[:5]:
        x = tied(TIE_TID_OFF, a, b, 5.0)   # (above the other timestamps' largest, about 3.5)
        x[50] = 12.0
        rows.append((x, plain))
    out.append(_mk("tie_tid", lc, zeros(V), rows))
    _cache["all"] = out
    return out


def references(case, depth=KERNEL_DEPTH):
    """The float64 reference of every row of a case, computed once per depth."""
    key = (case.name, depth)
    if key not in _cache:
        _cache[key] = [reference(case.x[k], case.smask, case.ctl[k], case.lc, depth)
                       for k in range(case.R)]
    return _cache[key]


def check_margins(case):
    for k, r in enumerate(references(case)):
        if r["written"]:
            try:
                margins(r, case.x[k], case.ctl[k], case.lc, k in case.mass_tie)
            except AssertionError as e:
                raise AssertionError(f"{case.name} row {k}: {e.args[0]}") from None
