"""Plain-numpy reference of the encoder stages that have a kernel of their own
(encoder attention, the 256 x 256 GEMM with its staged epilogues, LayerNorm, the
GELU table), the error bounds derived from the kernels' rounding points, f32 /
f16 emulations of those roundings, and the seeded inputs the tests run. Shared
by test_encoder_ref.py (CPU) and test_gpu_encoder_kernels.py; the sibling of
decode_ref.py, whose f16 / bf16_round / round_t / hu it reuses. Not a test
module itself and needs no GPU. No constant here is fitted to a GPU result,
except TANH_ULPS (below), which cannot be derived.

Attention contract (k_attn.hip enc_attn_kernel), per query, keys in tiles of 64:
  s_j      f32 MFMA dot of the f16 q . k_j
  x_j      (s_j * c) - m, c = f32(scale * log2 e), m the running max of s * c:
           two f32 roundings
  p_j      exp2(x_j)                       (v_exp_f32, <= 1 ulp)
  l        l * alpha + sum of the tile's unrounded f32 p_j, alpha = exp2(m_old - m_new)
  P_j      f16(p_j), relative to the running max
  O        O * alpha + V^T P in f32
  o        T(O * (1 / l))
compared with float64 attention over the f16 values, per element e:
  bound_e = rel sum_j p_j |v_je| + 2^-25 sum_j |v_je| + hu |o64_e| + 2^-25
  rel     = 2^-11 + 2^-20 (1 + max|s|) + 2 n 2^-24 + nt 2^-21 + 2^-22
2^-11: P rounded to f16 (normal range); 2^-25 sum |v|: P in f16's subnormal
range, absolute half-ulp 2^-25 in running-max units, which the later alpha <= 1
only shrink, and l >= 1 in final-max units (the maximal key contributes exactly
1 and every alpha after it is exp2(0) = 1), so the division does not enlarge it;
2^-20 (1 + max|s|): the f32 score chain (dot, times c, minus m, and the
m_old - m_new differences, whose sum is at most the climb of the running max)
and exp2, as a relative error of p (decode_ref's term); 2 n 2^-24: the f32
accumulation of V^T P and, here, of l too (a double in the decode kernel);
nt 2^-21, nt = ceil(n / 64) tiles: per tile alpha's exp2 (2^-23) and the
multiply by it (2^-24), once for O and once for l (3 2^-23 < 2^-21);
2^-22: 1 / l (<= 1 ulp) and the final multiply; hu |o64|: the output's
half-ulp; 2^-25: an f16 output in the subnormal range.
Keys >= the clip's length get p = 0 exactly and are multiplied with the V^T
columns there: those must be finite, nothing else is asked of them.

GEMM (k_gemm.hip gemm_big): float64 product of the T-rounded operands,
  beta = Kn 2^-24 sum_k |a_mk| |w_nk| + 2^-24 |ref|        (decode_ref.gemm_ref)
and per epilogue the half-ulp of each IEEE operation applied to acc:
  EPI_ENC_QKV   f16(acc + bias): x = ref + bias, bx = beta + 2^-24 (|x| + beta)
                (the f32 add), bound = bx + 2^-11 (|x| + bx) + 2^-25 (f16)
  EPI_CROSS_KV  K = f16(acc * kscale): the same with x = ref kscale and
                bx = beta |kscale| + 2^-24 (|x| + beta |kscale|); V as ENC_QKV
  EPI_RES       (acc + b) + res: bx as above, bound = bx + 2^-24 (|x + res| + bx)
  EPI_GELU / EPI_CONV2: gelu_ggml is a function from f16 to f16, taken from the
                device table (gelu_candidates_ok): an output is right iff it is
                T(tab[h]) (EPI_CONV2: f32(pe + tab[h])) for an f16 h in
                [f16(x - bx), f16(x + bx)] widened by one f16 neighbour each
                way, or a saturation value where the interval reaches |x| >= 10.

GELU table (gelu_table_kernel), all 2 x 0x4901 entries against float64:
  |tab[h] - gelu64(h)| <= half an f16 ulp of gelu64(h) (2^-25 in the subnormal
  range) + 0.5 |h| TANH_ULPS 2^-24
the second term being the error of 1 + tanhf(u) under cancellation. TANH_ULPS
is the device tanhf's error in f32 ulps of 1; it is measured on the GPU as the
smallest value this inequality admits over the whole domain, and asserted as
ceil(measured) + 1 (one ulp for another build of the device math library).

LayerNorm contract (k_misc.hip ln_kernel; ln_dec_kernel is bit-identical):
  s = double sum of v; mean = (float)(s / N); d = v - mean (f32);
  s2 = double sum of (double)(d * d); var = (float)(s2 / N);
  r = 1 / sqrtf(var + 1e-5f); y = T(((v - mean) * r) * w + b)
  with P: x = (sum P in ks order + pbias) + x, written back (bit-exact).
Against float64 (m, var, r = 1 / sqrt(var + eps), d = x - m, y = d r w + b):
  bound = |w| r (2^-24 (|x| + 2 |m|) + |d| (rho + 2^-23)) + 2^-24 |y|
          + hu (|y| + the terms before) + 2^-25
  rho   = 0.5 (2^-22 var + 2^-48 m^2 + 2^-24 (var + eps)) / (var + eps) + 2^-22
2^-24 (|x| + 2 |m|): the f32 mean (2^-24 |m|) and the rounding of v - mean
(2^-24 |d| <= 2^-24 (|x| + |m|)), amplified by r |w| (the cancellation term);
rho: the relative error of r: variance from the rounded d (2^-23 var: the
subtraction's rounding enters twice), d * d (2^-24) and the float cast
(2^-24), the shift of the f32 mean (its square only, sum d = 0: 2^-48 m^2),
the f32 add of eps, halved by the square root, then sqrtf and the division
(<= 1 ulp each: 2^-22); 2^-23: the two multiplies; 2^-24 |y|: the add of b.
"""
import numpy as np

from decode_ref import KQS, f16, bf16_round, round_t, hu, worst_ratio  # noqa: F401

GELU_TAB_HALF = 0x4901
# the device tanhf's error in f32 ulps admitted by gelu_table_bound (see above):
# ceil(measured) + 1. (observed on MI355X: gelu_table_admits = 0.798, reached at
# h = 2^-24, where the f32 product 0.5 h (1 + tanhf(u)) rounds onto an f16 tie:
# an f32 rounding of gelu_f32's own multiplies, which this term absorbs too)
TANH_ULPS = 2.0
LOG2E = 1.4426950408889634

ATTN_LENS = (1, 8, 9, 63, 64, 65, 127, 128, 129, 192, 200, 1500)
VL_L, VL_LENS = 200, (200, 1, 64, 65, 129)
F16_MAX = 65504.0


# --------------------------------------------------------------- attention

def attn_case(L, regime, seed=0, B=1, H=2):
    """q, k [B][H][L][64] f16, v [B][H][L][64] f16 (the caller lays out V^T),
    scale. regime 'diffuse': scores of std about 1. 'sharp_first' /
    'sharp_last': scores of std about 8 (|s| up to ~30) and one key, number
    min(5, L - 1) / L - 1, that every query scores near 40: exp2 underflows,
    P falls into f16's subnormal range, and the running max (alpha) jumps in
    the first / in the last, masked, tile."""
    rng = np.random.default_rng([seed, L, B, H, len(regime)])
    shp = (B, H, L, 64)
    v = f16(rng.standard_normal(shp))
    if regime == "diffuse":
        return dict(q=f16(rng.standard_normal(shp)), k=f16(rng.standard_normal(shp)), v=v,
                    scale=0.125, L=L, B=B, H=H)
    u = rng.standard_normal((B, H, 1, 64))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    q = 4.0 * u + 0.5 * rng.standard_normal(shp)
    k = 12.0 * rng.standard_normal(shp)
    j = min(5, L - 1) if regime == "sharp_first" else L - 1
    k[:, :, j] = 80.0 * u[:, :, 0]
    return dict(q=f16(q), k=f16(k), v=v, scale=0.125, L=L, B=B, H=H)


def vt_layout(v, pad):
    """[B][H][L][64] -> V^T [B][H][64][Lp]; pad columns: 0.0, or 'max' for
    +-65504 in alternating signs."""
    B, H, L, _ = v.shape
    Lp = (L + 7) & ~7
    vt = np.zeros((B, H, 64, Lp), np.float16)
    if pad == "max":
        vt[:] = np.where((np.arange(64)[:, None] + np.arange(Lp)[None]) & 1, -F16_MAX, F16_MAX)
    vt[..., :L] = np.swapaxes(v, 2, 3)
    return vt


def vl_case(seed=0, H=2):
    """The variable-length launch: B = 5 clips of lens VL_LENS in buffers of
    L = 200 rows. Q and K rows >= lens[b] hold NaN, V rows >= lens[b] +-65504
    (finite: the kernel multiplies them by zero)."""
    B, L = len(VL_LENS), VL_L
    c = attn_case(L, "diffuse", seed + 100, B=B, H=H)
    sign = np.where((np.arange(L)[:, None] + np.arange(64)[None]) & 1, -F16_MAX, F16_MAX)
    for b, n in enumerate(VL_LENS):
        c["q"][b, :, n:] = np.nan
        c["k"][b, :, n:] = np.nan
        c["v"][b, :, n:] = sign[n:].astype(np.float16)
    c["lens"] = np.asarray(VL_LENS, np.int32)
    return c


def attention_ref(q, k, v, scale, bf16):
    """float64 attention of one (clip, head): q [Lq][64], k, v [n][64] (f16
    values). Returns (o64 [Lq][64], bound [Lq][64])."""
    q64, k64, v64 = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    n = k64.shape[0]
    s = (q64 @ k64.T) * float(np.float32(scale))
    smax = np.abs(s).max(axis=1, keepdims=True)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    o = p @ v64
    nt = (n + 63) // 64
    rel = 2.0 ** -11 + 2.0 ** -20 * (1.0 + smax) + 2 * n * 2.0 ** -24 + nt * 2.0 ** -21 + 2.0 ** -22
    bound = rel * (p @ np.abs(v64)) + 2.0 ** -25 * np.abs(v64).sum(axis=0)[None] \
        + hu(bf16) * np.abs(o) + 2.0 ** -25
    return o, bound


def attention_emulate(q, k, vt_row, n, scale, bf16, broken=None):
    """enc_attn_kernel's roundings for one (clip, head) in numpy f32: 64-key
    tiles, running max, alpha rescale, unrounded f32 row sum, P = f16(p).
    q [Lq][64], k [>= n][64], vt_row [64][Lp] (V^T with its pad columns), n keys.
    broken: None, or one of 'drop_last' (the last key never scored), 'mask+1'
    (the last tile's mask admits key n: the clamped K row n - 1 and V^T column
    n), 'no_alpha' (the rescale skipped), 'swap8' (P of keys j and j + 8
    exchanged before P.V)."""
    q32 = np.asarray(q, dtype=np.float32)
    k32 = np.asarray(k, dtype=np.float32)
    vt = np.asarray(vt_row, dtype=np.float32)
    c = np.float32(np.float32(scale) * np.float32(LOG2E))
    Lq = q32.shape[0]
    m = np.full(Lq, -np.inf, np.float32)
    l = np.zeros(Lq, np.float32)
    O = np.zeros((Lq, 64), np.float32)
    nkeys = n - 1 if broken == "drop_last" and n > 1 else n
    admit = nkeys + 1 if broken == "mask+1" and nkeys % 64 else nkeys
    for k0 in range(0, nkeys, 64):
        idx = np.arange(k0, min(k0 + 64, admit))
        kt = k32[np.minimum(idx, n - 1)]
        vcol = np.zeros((64, len(idx)), np.float32)
        ok = idx < vt.shape[1]
        vcol[:, ok] = vt[:, idx[ok]]
        s = (q32 @ kt.T).astype(np.float32)
        mnew = np.maximum(m, s.max(axis=1) * c)
        with np.errstate(invalid="ignore"):
            alpha = np.exp2(m - mnew).astype(np.float32)
        if broken == "no_alpha":
            alpha = np.ones_like(alpha)
        x = (s * c).astype(np.float32) - mnew[:, None]
        p = np.exp2(x.astype(np.float32)).astype(np.float32)
        rs = np.cumsum(p, axis=1, dtype=np.float32)[:, -1]
        l = l * alpha + rs
        m = mnew
        P = f16(p).astype(np.float32)
        if broken == "swap8" and len(idx) > 8:
            P[:, [0, 8]] = P[:, [8, 0]]
        O = O * alpha[:, None] + (P @ vcol.T).astype(np.float32)
    inv = (np.float32(1.0) / l).astype(np.float32)
    return round_t(O * inv[:, None], bf16)


def attn_query_blocks(L, n):
    """(blocks that run, blocks zero-filled) of a clip of n frames in a launch
    of L rows: 128 queries per workgroup (enc_attention)."""
    nqb = (L + 127) // 128
    run = sum(1 for i in range(nqb) if i * 128 < n)
    return run, nqb - run


# -------------------------------------------------------------------- GEMM

BM = BN = 256  # gemm_big's output tile


def gemm_tile_map(M, N, group_m=8, xcd_remap=True):
    """gemm_big's workgroup id -> (row tile, column tile), restated."""
    nbm, nbn = (M + BM - 1) // BM, (N + BN - 1) // BN
    nwg = nbm * nbn
    out = []
    for wg in range(nwg):
        w = wg
        if xcd_remap:
            xcd, q, r = w % 8, nwg // 8, nwg % 8
            w = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + w // 8
        mt, nt = w // nbn, w % nbn
        if group_m > 0:
            per = group_m * nbn
            g, i = w // per, w % per
            gm = min(group_m, nbm - g * group_m)
            mt, nt = g * group_m + i % gm, i // gm
        out.append((mt, nt))
    return out


def gemm_inputs(seed, M, N, K, a_rows=None):
    """a [a_rows or M][K] of std 1, w [N][K] of std K^-1/2 (outputs of std 1),
    bias of std 2 and a residual of std 4: a dropped bias or residual shows."""
    rng = np.random.default_rng([seed, M, N, K])
    a = rng.standard_normal((a_rows or M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = (2.0 * rng.standard_normal(N)).astype(np.float32)
    res = (4.0 * rng.standard_normal((M, N))).astype(np.float32)
    return a, w, bias, res


def gemm_acc_ref(a, w, bf16):
    """(ref, beta) of a [M][K] . w [N][K]^T over the T-rounded operands."""
    a64 = round_t(a, bf16).astype(np.float64)
    w64 = round_t(w, bf16).astype(np.float64)
    ref = a64 @ w64.T
    beta = a.shape[1] * 2.0 ** -24 * (np.abs(a64) @ np.abs(w64).T) + 2.0 ** -24 * np.abs(ref)
    return ref, beta


def gemm_emulate(a, w, bf16, drop_tile=None):
    """Sequential f32 accumulation of the exact products (small shapes only);
    drop_tile: the 64-deep K tile left out (a broken prologue)."""
    a32, w32 = round_t(a, bf16), round_t(w, bf16)
    if drop_tile is not None:
        a32 = a32.copy()
        a32[:, drop_tile * 64:(drop_tile + 1) * 64] = 0.0
    prod = a32[:, None, :] * w32[None, :, :]
    return np.cumsum(prod, axis=2, dtype=np.float32)[:, :, -1]


def add_bound(ref, beta, addend):
    """x = ref + addend computed as one f32 add of acc: (x64, bound)."""
    x = ref + addend
    return x, beta + 2.0 ** -24 * (np.abs(x) + beta)


def f16_store_bound(x, bx):
    return bx + 2.0 ** -11 * (np.abs(x) + bx) + 2.0 ** -25


def res_ref(ref, beta, bias, res):
    x, bx = add_bound(ref, beta, 0.0 if bias is None else np.asarray(bias, np.float64)[None])
    y = x + np.asarray(res, np.float64)
    return y, bx + 2.0 ** -24 * (np.abs(y) + bx)


def kscale_bound(ref, beta, kscale):
    ks = float(np.float32(kscale))
    x, b = ref * ks, beta * abs(ks)
    return x, b + 2.0 ** -24 * (np.abs(x) + b)


def mx_encode(x):
    """The MX-fp8 block rule (kcommon.h mx_exp / e4m3_rne, the rule
    test_quant_format.np_mx_round restates as values) as codes and scales:
    x [..., 32 n] f32 -> (e4m3fn codes uint8 of x's shape, E8M0 scales uint8
    [..., n]). Per 32 elements E = the smallest integer with amax <= 448 2^E
    (0 for an all-zero block), scale byte 127 + E, code = e4m3fn nearest-even of
    x / 2^E with the sign bit of x < 0."""
    x = np.asarray(x, np.float32)
    blk = x.reshape(-1, 32)
    amax = np.abs(blk).max(axis=1)
    E = np.zeros(len(blk), np.int64)
    nz = amax > 0
    E[nz] = np.ceil(np.log2(amax[nz].astype(np.float64) / 448.0)).astype(np.int64)
    E = np.clip(E, -127, 127)
    v = blk.astype(np.float64) / np.ldexp(1.0, E)[:, None]
    a = np.abs(v)
    e = np.floor(np.log2(np.where(a > 0, a, 1.0))).astype(np.int64)
    e = np.maximum(e, -6)
    qm = np.rint(a / np.ldexp(1.0, e - 3)).astype(np.int64)  # mantissa in units of 2^(e-3)
    up = qm == 16
    qm, e = np.where(up, 8, qm), np.where(up, e + 1, e)
    code = np.where(qm < 8, qm, ((e + 7) << 3) | (qm - 8))  # qm < 8: subnormal, step 2^-9
    code = (code | np.where(v < 0, 0x80, 0)).astype(np.uint8)
    return code.reshape(x.shape), (127 + E).astype(np.uint8).reshape(x.shape[:-1] + (-1,))


def mx_decode(codes, scales):
    """The values (f32) of mx_encode's output."""
    c = np.asarray(codes, np.uint8).astype(np.int64)
    ex, man = (c >> 3) & 15, c & 7
    mag = np.where(ex == 0, man * 2.0 ** -9, (8 + man) * np.ldexp(1.0, ex - 10))
    val = np.where(c & 0x80, -mag, mag).reshape(-1, 32)
    X = np.ldexp(1.0, np.asarray(scales, np.uint8).astype(np.int64).reshape(-1) - 127)
    return (val * X[:, None]).astype(np.float32).reshape(np.shape(codes))


def mx_gemm_ref(a, w, bf16):
    """MX operands: float64 product of the MX rounding of the T-rounded
    operands, and the accumulator criterion of test_mx_gemm_exact (5e-5 of
    sum |a| |w|: the project's own number for the block-scaled MFMA, whose
    internal accumulation is not a plain f32 chain)."""
    aq = mx_decode(*mx_encode(round_t(a, bf16))).astype(np.float64)
    wq = mx_decode(*mx_encode(round_t(w, bf16))).astype(np.float64)
    return aq @ wq.T, 5e-5 * (np.abs(aq) @ np.abs(wq).T)


def im2col(x, taps=3, stride=1):
    """x [T + 2][C] (a zero row at each end already there) -> [T / stride][taps C]:
    what the conv-stem GEMMs read through lda = stride C, K = taps C."""
    T = (x.shape[0] - (taps - 1)) // stride
    return np.stack([x[t * stride:t * stride + taps].reshape(-1) for t in range(T)])


# -------------------------------------------------------------------- GELU

def gelu64(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + np.tanh(0.7978845608028654 * x * (1.0 + 0.044715 * x * x)))


def gelu_table_inputs():
    """The f16 value of every table entry, in table order."""
    i = np.arange(GELU_TAB_HALF, dtype=np.uint16)
    return np.concatenate([i.view(np.float16), (i | 0x8000).view(np.float16)]).astype(np.float64)


def f16_half_ulp(x):
    """Half an f16 ulp at |x| (2^-25 in the subnormal range)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 11)


def gelu_table_bound(tanh_ulps=None):
    h = gelu_table_inputs()
    g = gelu64(h)
    t = TANH_ULPS if tanh_ulps is None else tanh_ulps
    return g, f16_half_ulp(g) + 0.5 * np.abs(h) * t * 2.0 ** -24


def gelu_table_admits(tab_bits):
    """The smallest tanhf error (f32 ulps) under which the table satisfies
    gelu_table_bound, over the whole domain."""
    tab = np.asarray(tab_bits[:2 * GELU_TAB_HALF], np.uint16).view(np.float16).astype(np.float64)
    h = gelu_table_inputs()
    g = gelu64(h)
    excess = np.abs(tab - g) - f16_half_ulp(g)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(excess > 0, excess / (0.5 * np.abs(h) * 2.0 ** -24), 0.0)
    return float(np.nanmax(t))


def _ord(h):
    """f16 array -> integers in value order (-0 and +0 both 0)."""
    b = np.asarray(h, np.float16).view(np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def gelu_candidates_ok(out, x64, bx, tab_bits, finish):
    """The set-membership check of a GELU epilogue. out: the kernel's values
    (f64 / f32 array); x64, bx: the float64 pre-activation and its bound;
    finish(g, sel) maps table values g (f32, one per flat output index in sel)
    to the stored value: T rounding, or the add of pe.reshape(-1)[sel].
    Returns a bool array of out's shape."""
    tab = np.asarray(tab_bits[:2 * GELU_TAB_HALF], np.uint16).view(np.float16).astype(np.float32)
    lo, hi = x64 - bx, x64 + bx
    with np.errstate(over="ignore"):
        olo = np.clip(_ord(f16(lo)) - 1, -0x4900, 0x4900)
        ohi = np.clip(_ord(f16(hi)) + 1, -0x4900, 0x4900)
    shape = np.shape(out)
    out = np.asarray(out, np.float32).reshape(-1)
    lo, hi, olo, ohi = (np.broadcast_to(v, shape).reshape(-1) for v in (lo, hi, olo, ohi))
    ok = np.zeros(out.shape, bool)
    every = np.arange(out.size)
    # candidate h = olo + step, tried only where nothing matched yet and the
    # interval still has one (long intervals occur only next to zero)
    live = every
    step = 0
    while live.size:
        o = olo[live] + step
        g = tab[np.where(o >= 0, o, GELU_TAB_HALF - o)]
        hit = finish(g, live) == out[live]
        ok[live[hit]] = True
        step += 1
        live = live[~hit]
        live = live[olo[live] + step <= ohi[live]]
    # saturation: gelu_ggml(x) = 0 for x <= -10 and x for x >= 10 (x the f32
    # pre-activation, anywhere in [lo, hi])
    ok |= (lo <= -10.0) & (finish(np.zeros_like(out), every) == out)
    sat = hi >= 10.0
    if sat.any():
        a = finish(np.maximum(lo, 10.0).astype(np.float32) * np.float32(1 - 2.0 ** -23), every)
        b = finish(hi.astype(np.float32) * np.float32(1 + 2.0 ** -23), every)
        ok |= sat & (out >= np.minimum(a, b)) & (out <= np.maximum(a, b))
    return ok.reshape(shape)


def gelu_emulate(x32, tab_bits):
    """gelu_ggml_tab on f32 pre-activations."""
    tab = np.asarray(tab_bits[:2 * GELU_TAB_HALF], np.uint16).view(np.float16).astype(np.float32)
    x32 = np.asarray(x32, np.float32)
    o = _ord(f16(np.clip(x32, -10.0, 10.0)))
    g = tab[np.where(o >= 0, o, GELU_TAB_HALF - o)]
    neg0 = (f16(x32).view(np.uint16) == 0x8000)
    g = np.where(neg0, tab[GELU_TAB_HALF], g)
    return np.where(x32 <= -10.0, np.float32(0), np.where(x32 >= 10.0, x32, g)).astype(np.float32)


def host_gelu_table():
    """A stand-in table for the CPU tests: f16(gelu64(h)) (the device's differs
    from it within gelu_table_bound)."""
    return np.asarray(gelu64(gelu_table_inputs()), np.float32).astype(np.float16).view(np.uint16)


# --------------------------------------------------------------- LayerNorm

LN_NS = (64, 384, 512, 768, 1024, 1280, 2048)
LN_M = 37
LN_EPS = float(np.float32(1e-5))


def ln_case(N, seed=0, M=LN_M):
    """x [M][N]: row kinds by r % 4: unit normal; mean 100 with std 0.01 (the
    cancellation in v - mean); a constant row (variance 0: y = T(b)); values
    2^60 N(0, 1) (d * d stays below f32's maximum, 2^124 at four sigma, and
    float64 is nowhere near its own: the reference is finite). Rows with
    r % 5 == 3 are inactive."""
    rng = np.random.default_rng([seed, N, M])
    x = rng.standard_normal((M, N)).astype(np.float32)
    for r in range(M):
        if r % 4 == 1:
            x[r] = (100.0 + 0.01 * x[r]).astype(np.float32)
        elif r % 4 == 2:
            x[r] = np.float32(3.0 + r)
        elif r % 4 == 3:
            x[r] = x[r] * np.float32(2.0 ** 60)
    w = (1.0 + 0.5 * rng.standard_normal(N)).astype(np.float32)
    b = (0.5 * rng.standard_normal(N)).astype(np.float32)
    active = (np.arange(M) % 5 != 3).astype(np.int32)
    return dict(x=x, w=w, b=b, active=active)


def ln_slabs(x, KS, seed=0):
    """P [KS][M][N] and pbias [N] of the size of x's unit-normal rows."""
    rng = np.random.default_rng([seed, KS, x.shape[1]])
    P = rng.standard_normal((KS,) + x.shape).astype(np.float32)
    return P, (0.3 * rng.standard_normal(x.shape[1])).astype(np.float32)


def ln_fold(x, P, pbias):
    """x = (sum P in ks order + pbias) + x in f32 (bit-exact contract)."""
    acc = P[0].copy()
    for ks in range(1, P.shape[0]):
        acc = acc + P[ks]
    out = (acc + pbias[None]) + x
    assert out.dtype == np.float32
    return out


def ln_ref(x, w, b, bf16):
    """(y64, bound) [M][N]."""
    x64, w64, b64 = (np.asarray(a, np.float64) for a in (x, w, b))
    m = x64.mean(axis=1, keepdims=True)
    d = x64 - m
    var = (d * d).mean(axis=1, keepdims=True)
    r = 1.0 / np.sqrt(var + LN_EPS)
    y = d * r * w64 + b64
    rho = 0.5 * (2.0 ** -22 * var + 2.0 ** -48 * m * m + 2.0 ** -24 * (var + LN_EPS)) \
        / (var + LN_EPS) + 2.0 ** -22
    pre = np.abs(w64) * r * (2.0 ** -24 * (np.abs(x64) + 2 * np.abs(m))
                              + np.abs(d) * (rho + 2.0 ** -23)) + 2.0 ** -24 * np.abs(y)
    return y, pre + hu(bf16) * (np.abs(y) + pre) + 2.0 ** -25


def ln_emulate(x, w, b, bf16, ddof=0):
    """ln_kernel's roundings; ddof = 1: the broken variance over N - 1."""
    x = np.asarray(x, np.float32)
    N = x.shape[1]
    mean = (x.astype(np.float64).sum(axis=1) / N).astype(np.float32)[:, None]
    d = x - mean
    var = ((d * d).astype(np.float64).sum(axis=1) / (N - ddof)).astype(np.float32)[:, None]
    scale = (np.float32(1.0) / np.sqrt(var + np.float32(1e-5))).astype(np.float32)
    y = ((x - mean) * scale) * np.asarray(w, np.float32) + np.asarray(b, np.float32)
    assert y.dtype == np.float32
    return round_t(y, bf16)
