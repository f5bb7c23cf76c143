"""Plain-numpy reference of the decode attention and decode GEMM stages, the
error bounds derived from the kernels' rounding points, an f32 / f16 emulation
of those roundings, and the seeded inputs the tests run. Shared by
test_decode_ref.py (CPU) and test_gpu_decode_kernels.py; not a test module
itself and needs no GPU.

Stage contract (k_attn.hip dec_attn_kernel / dec_xattn_kernel / kv_append):
  slab sum   acc = P[0] + P[1] + ... in f32, in ks order
  q          f16((acc + bias) * qscale)       (two f32 operations, one rounding)
  k_new      f16(acc * kscale)                (no bias)
  v_new      f16(acc + bias)
  scores     f32 dot of the f16 values, times scale
  P          f16(expf(s - max) * (float)(1 / double sum))
  o          T(f32 sum of P_j v_j)            (T = f16 or bf16)
The values appended to the cache are single IEEE operations on the f32 slab
sum, so they are compared bit for bit. The output is compared with float64
attention over those f16 values, per element e:

  bound_e = (2^-11 + 2^-20 (1 + max|s|) + n 2^-24) sum_j p_j |v_je|
            + 2^-25 sum_j |v_je| + hu |o64_e| + 2^-25

2^-11: P rounded to f16 (normal range); 2^-25 sum |v|: P in f16's subnormal
range (absolute half-ulp 2^-25); 2^-20 (1 + max|s|): the f32 score (dot,
scale, subtraction of the max) and expf, as a relative error of P; n 2^-24:
the f32 accumulation of P.V in any order; hu |o64|: the output's half-ulp
(2^-11 f16, 2^-8 bf16); 2^-25: an f16 output in the subnormal range.

GEMM: float64 product of the T-rounded operands; per element
  bound = Kn 2^-24 sum_k |a_mk| |w_nk| + 2^-24 |ref|
(Kn = the number of k summed: products of two 16-bit values are exact in f32,
each of the at most Kn f32 additions rounds once, in any order).

MX-fp8 weights (W8 kernels): the e4m3 codes of a lane's 8 k are widened to bf16
under the E8M0 scale of (column, k / 32), exactly, and the bf16 chain runs
unchanged: the reference is gemm_ref on mx_decode(codes, scales), the same
bound, and the kernel's bits are those of the 16-bit kernel on those values
(w8_widen restates the addressing, with deliberately broken variants).
The FFN1 epilogue stores T(gelu_ggml(acc + bias)) at pack_index(m, n, N) of a
buffer of ceil64(M) rows (pack_store / packed_store_ok). splitk_factor,
skinny_split and ln_fold_serves restate the launchers' K rules.
"""
import numpy as np

F16_NAN = np.uint16(0x7E00)
KQS = float(np.float32(64.0) ** np.float32(-0.25))  # the engine's q / k scale, 64^-1/4
SELF_LENS = (1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 255, 256, 257, 384, 385, 447, 448)
CROSS_LENS = (1, 8, 9, 17, 255, 256, 257, 513, 777, 1499, 1500, 1501, 1536)
SPLITK_KS = {128: 1, 512: 4, 1280: 5, 3072: 8, 4096: 8, 5120: 8}  # splitk_factor(K)


def hu(bf16):
    return 2.0 ** -8 if bf16 else 2.0 ** -11


def f16(x):
    """f32 -> f16, round to nearest even (numpy's conversion)."""
    return np.asarray(x, dtype=np.float32).astype(np.float16)


def bf16_round(x):
    """f32 -> bf16 (round to nearest even) -> f32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def round_t(x, bf16):
    """f32 -> T -> f32 (T = bf16 or f16)."""
    x = np.asarray(x, dtype=np.float32)
    return bf16_round(x) if bf16 else x.astype(np.float16).astype(np.float32)


def slab_sum(P):
    """[KS][R][pcols] f32 -> [R][pcols], summed in ks order in f32."""
    P = np.asarray(P, dtype=np.float32)
    acc = P[0].copy()
    for ks in range(1, P.shape[0]):
        acc = acc + P[ks]
    assert acc.dtype == np.float32
    return acc


def form_qkv(P, bias, H, qscale, kscale, self_attn):
    """The f16 query (and, self: the new key / value) of every row, [R][H][64]."""
    s = slab_sum(P)
    bias = np.asarray(bias, dtype=np.float32)
    D = H * 64
    R = s.shape[0]
    q = f16((s[:, :D] + bias[:D]) * np.float32(qscale)).reshape(R, H, 64)
    if not self_attn:
        return q, None, None
    k = f16(s[:, D:2 * D] * np.float32(kscale)).reshape(R, H, 64)
    v = f16(s[:, 2 * D:] + bias[2 * D:]).reshape(R, H, 64)
    return q, k, v


def attention_ref(q, K, V, scale, bf16):
    """float64 attention of one row. q [H][64], K / V [n][H][64] (f16 values).
    Returns (o64 [H*64], bound [H*64])."""
    q64 = np.asarray(q, dtype=np.float64)
    K64 = np.asarray(K, dtype=np.float64)
    V64 = np.asarray(V, dtype=np.float64)
    n = K64.shape[0]
    s = np.einsum("he,nhe->hn", q64, K64) * float(np.float32(scale))
    smax = np.abs(s).max(axis=1)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    o = np.einsum("hn,nhe->he", p, V64)
    pav = np.einsum("hn,nhe->he", p, np.abs(V64))
    av = np.abs(V64).sum(axis=0)
    rel = 2.0 ** -11 + 2.0 ** -20 * (1.0 + smax) + n * 2.0 ** -24
    bound = rel[:, None] * pav + 2.0 ** -25 * av + hu(bf16) * np.abs(o) + 2.0 ** -25
    return o.reshape(-1), bound.reshape(-1)


def attention_emulate(q, K, V, scale, bf16):
    """The kernel's roundings in numpy: f32 scores (sequential f32 dot), f32
    expf, double sum, P = f16(e * (float)(1 / sum)), sequential f32 P.V, T
    output. Returns o [H*64] f32."""
    q32 = np.asarray(q, dtype=np.float32)
    K32 = np.asarray(K, dtype=np.float32)
    V32 = np.asarray(V, dtype=np.float32)
    prod = K32 * q32[None]                                      # exact in f32
    d = np.cumsum(prod, axis=2, dtype=np.float32)[:, :, -1]     # [n][H]
    s = d * np.float32(scale)
    e = np.exp((s - s.max(axis=0, keepdims=True)).astype(np.float32)).astype(np.float32)
    inv = (1.0 / e.astype(np.float64).sum(axis=0)).astype(np.float32)
    p = f16(e * inv[None]).astype(np.float32)                   # [n][H]
    o = np.cumsum(p[:, :, None] * V32, axis=0, dtype=np.float32)[-1]
    return round_t(o, bf16).reshape(-1)


def worst_ratio(o, o64, bound):
    return float(np.max(np.abs(np.asarray(o, dtype=np.float64) - o64) / bound))


# ------------------------------------------------------------------ inputs

def _slabs(rng, target, KS):
    """KS f32 slabs whose sum is near `target`: random shares of it, of both
    signs, so the f32 sum depends on the order and on every slab."""
    g = 0.5 * rng.standard_normal(target.shape + (KS,))
    w = (g - g.mean(axis=-1, keepdims=True) + 1.0 / KS).astype(np.float32)  # sums to 1
    return np.ascontiguousarray(np.moveaxis(w * target[..., None], -1, 0), dtype=np.float32)


def nan_cache(slots, H, cap):
    return np.full((slots, H, cap, 64), F16_NAN, np.uint16).view(np.float16)


def self_case(seed, qs, KS, H=2, lens=SELF_LENS, cap=448):
    """One self-attention launch with one row per length in `lens`: row r
    attends positions 0 .. lens[r]-1, the last being the one it appends. Every
    cache position >= pos of a row (its own included) holds f16 NaN. Raw
    projections have std qs (query) and 1 (key, value); q and k carry the
    engine's 64^-1/4 each, so the scores have std about qs."""
    rng = np.random.default_rng([seed, KS, int(qs * 1000)])
    R, D = len(lens), H * 64
    pos = np.asarray(lens, np.int32) - 1
    target = rng.standard_normal((R, 3 * D)).astype(np.float32)
    target[:, :D] *= np.float32(qs)
    bias = (0.1 * rng.standard_normal(3 * D)).astype(np.float32)
    kc, vc = nan_cache(R, H, cap), nan_cache(R, H, cap)
    for r in range(R):
        kc[r, :, :pos[r]] = f16(rng.standard_normal((H, pos[r], 64)) * KQS)
        vc[r, :, :pos[r]] = f16(rng.standard_normal((H, pos[r], 64)))
    return dict(P=_slabs(rng, target, KS), bias=bias, kc=kc, vc=vc, pos=pos,
                active=np.ones(R, np.int32), H=H, cap=cap, qscale=KQS, kscale=KQS, scale=1.0)


def self_rows(case, kvmap=None, own_from=None, map_row0=0, kv_index=None):
    """Per row of a self case: (q [H][64], K [n][H][64], V, k_new, v_new), the
    history gathered through kv_index / the position map as the kernel does."""
    q, kn, vn = form_qkv(case["P"], case["bias"], case["H"], case["qscale"], case["kscale"], True)
    out = []
    for r, p in enumerate(case["pos"]):
        slot = r if kv_index is None else int(kv_index[r])
        src = np.full(p, slot)
        if own_from is not None:
            src[:own_from[r]] = kvmap[r, :own_from[r]] - map_row0
        j = np.arange(p)
        K = np.concatenate([case["kc"][src, :, j], kn[r][None]], axis=0)
        V = np.concatenate([case["vc"][src, :, j], vn[r][None]], axis=0)
        out.append((q[r], K, V, kn[r], vn[r]))
    return out


def cross_case(seed, n, R, H, KS, slots, kv_index=None, cap=1536, qs=(0.02, 3.0, 0.5)):
    """One cross-attention launch over n keys: row r has query std qs[r % 3],
    the cache keys carry 64^-1/4 and scale = 64^-1/4 (scores of std about qs),
    rows >= n of every slot hold f16 NaN."""
    rng = np.random.default_rng([seed, n, R, KS])
    D = H * 64
    target = rng.standard_normal((R, D)).astype(np.float32)
    target *= np.asarray([qs[r % len(qs)] for r in range(R)], np.float32)[:, None]
    bias = (0.1 * rng.standard_normal(D)).astype(np.float32)
    kc, vc = nan_cache(slots, H, cap), nan_cache(slots, H, cap)
    kc[:, :, :n] = f16(rng.standard_normal((slots, H, n, 64)) * KQS)
    vc[:, :, :n] = f16(rng.standard_normal((slots, H, n, 64)))
    kvi = np.arange(R, dtype=np.int32) if kv_index is None else np.asarray(kv_index, np.int32)
    return dict(P=_slabs(rng, target, KS), bias=bias, kc=kc, vc=vc, kv_index=kvi, n=n,
                active=np.ones(R, np.int32), H=H, cap=cap, qscale=1.0, kscale=1.0, scale=KQS)


def cross_rows(case):
    q, _, _ = form_qkv(case["P"], case["bias"], case["H"], case["qscale"], 1.0, False)
    n = case["n"]
    return [(q[r], np.moveaxis(case["kc"][s, :, :n], 0, 1), np.moveaxis(case["vc"][s, :, :n], 0, 1))
            for r, s in enumerate(case["kv_index"])]


# -------------------------------------------------------------------- GEMM

def gemm_inputs(seed, M, N, K):
    rng = np.random.default_rng([seed, M, N, K])
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    return a, w


def gemm_ref(a, w, bf16, k0=0, k1=None):
    """float64 product of the T-rounded operands over k0 <= k < k1, and its
    bound. Returns (ref [M][N], bound [M][N])."""
    k1 = a.shape[1] if k1 is None else k1
    a64 = round_t(a, bf16)[:, k0:k1].astype(np.float64)
    w64 = round_t(w, bf16)[:, k0:k1].astype(np.float64)
    ref = a64 @ w64.T
    bound = (k1 - k0) * 2.0 ** -24 * (np.abs(a64) @ np.abs(w64).T) + 2.0 ** -24 * np.abs(ref)
    return ref, bound


def gemm_emulate(a, w, bf16, k0=0, k1=None):
    """Sequential f32 accumulation of the exact products."""
    k1 = a.shape[1] if k1 is None else k1
    a32 = round_t(a, bf16)[:, k0:k1]
    w32 = round_t(w, bf16)[:, k0:k1]
    prod = a32[:, None, :] * w32[None, :, :]
    return np.cumsum(prod, axis=2, dtype=np.float32)[:, :, -1]


# ------------------------------------------------- the kernels' K splits

def splitk_factor(K):
    """k_gemm.hip splitk_factor: the largest KS <= 8 whose slices are four
    waves of 1 .. 5 32-deep k-steps; 0: K not served by the split-K kernels."""
    if K % 128:
        return 0
    S = K // 32
    for ks in range(8, 0, -1):
        if S % ks == 0 and (S // ks) % 4 == 0 and S // ks // 4 <= 5:
            return ks
    return 0


def skinny_split(K):
    """k_gemm.hip skinny_split: (waves, k-steps per wave) of the full-K
    kernels, the most waves <= 16 with 1 / 2 / 3 / 4 / 6 / 8 / 10 k-steps
    each; None: K not served."""
    if K % 32:
        return None
    S = K // 32
    for w in range(16, 0, -1):
        if S % w == 0 and S // w in (1, 2, 3, 4, 6, 8, 10):
            return w, S // w
    return None


def ln_fold_serves(K, mode):
    """Whether gemm_splitk_ln (mode 0) / gemm_decode_ln (mode 3) take the
    width: the row in 2048 elements of LDS, and the K split above (the full-K
    kernel's prologue needs four waves)."""
    if K > 2048 or K % 8:
        return False
    if mode == 0:
        return splitk_factor(K) > 0
    s = skinny_split(K)
    return s is not None and s[0] >= 4


# ------------------------------------------------------- fragment tiles

def pack_index(n, k, K):
    """kernels.h pack_index: element (n, k) of a [rows][K] operand in fragment
    tiles: 16-row strip nt, 32-deep k-step kt, lane (k % 32 / 8) 16 + n % 16,
    8 consecutive k per lane."""
    n, k = np.asarray(n, np.int64), np.asarray(k, np.int64)
    return (((n >> 4) * (K >> 5) + (k >> 5)) * 64 + ((k & 31) >> 3) * 16 + (n & 15)) * 8 + (k & 7)


SENT16 = np.uint16(0xFFFF)  # the packed output buffer's words before the launch


def pack_store(vals, broken=None):
    """The packed store of the decode FFN1 epilogue on a 16-bit [M][N] array:
    the buffer of ceil64(M) N words it leaves. broken 'transposed': the store
    at pack_index(n, m, N) (stores past the buffer dropped); 'drop64': rows
    >= 64 not stored."""
    vals = np.asarray(vals, np.uint16)
    M, N = vals.shape
    buf = np.full((M + 63) // 64 * 64 * N, SENT16)
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    idx = pack_index(n, m, N) if broken == "transposed" else pack_index(m, n, N)
    keep = idx < buf.size
    if broken == "drop64":
        keep &= m < 64
    buf[idx[keep]] = vals[keep]
    return buf


def packed_rows(buf, M, N):
    """The packed buffer as [ceil64(M)][N] words in (row, column) order."""
    M64 = (M + 63) // 64 * 64
    m, n = np.meshgrid(np.arange(M64), np.arange(N), indexing="ij")
    return np.asarray(buf, np.uint16)[pack_index(m, n, N)]


def packed_store_ok(buf, M, N):
    """Every word of rows < M written, every word of the pad rows M ..
    ceil64(M) - 1 still the sentinel. Returns (ok, rows [M][N])."""
    assert np.size(buf) == (M + 63) // 64 * 64 * N
    rows = packed_rows(buf, M, N)
    return bool((rows[:M] != SENT16).all() and (rows[M:] == SENT16).all()), rows[:M]


# ------------------------------------------------ MX-fp8 decode weights

FINITE_CODES = np.asarray([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)  # e4m3fn: 254


def mx_decode(codes, scales):
    """encoder_ref.mx_decode (that module imports this one): e4m3fn codes
    [N][K] under E8M0 scales [N][K/32], code x 2^(s - 127), exact in f32."""
    from encoder_ref import mx_decode as decode
    return decode(codes, scales)


def mx_dec_weights(seed, N, K, span=(-30, 8)):
    """codes [N][K] drawn from the finite e4m3fn codes and scales [N][K/32]
    with the block exponents s - 127 uniform over span (both ends included):
    neighbouring blocks differ by many binades, so a scale taken from the
    wrong block is no rounding error."""
    rng = np.random.default_rng([seed, N, K, span[0] + 1000, span[1] + 1000])
    codes = FINITE_CODES[rng.integers(0, len(FINITE_CODES), (N, K))]
    scales = (127 + rng.integers(span[0], span[1] + 1, (N, K // 32))).astype(np.uint8)
    return codes, scales


def mx_probe_weights(seed, N, K, span=(-100, 100)):
    """The identity probe's weights: every finite code and every exponent of
    span that N K / 32 blocks can hold (evenly spread, both ends included),
    each as often as the other, in a seeded shuffle."""
    rng = np.random.default_rng([seed, N, K])
    codes = np.resize(FINITE_CODES, N * K)
    nb = N * K // 32
    exps = np.round(np.linspace(span[0], span[1], min(nb, span[1] - span[0] + 1))).astype(np.int64)
    scales = np.resize(127 + exps, nb).astype(np.uint8)
    return rng.permutation(codes).reshape(N, K), rng.permutation(scales).reshape(N, K // 32)


W8_BROKEN = ("scale_kt+1", "scale_n^1", "scale_per_64", "codes_reversed", "halves_swapped")


def w8_widen(codes, scales, broken=None):
    """What the W8 kernels feed the MFMA for element (n, k): the lane holding
    k % 32 / 8 of column n widens its 8 codes under the scale word of (n,
    k / 32). broken: 'scale_kt+1' the scale of the next k-step (the last of a
    row wraps to its first), 'scale_n^1' of the neighbouring column,
    'scale_per_64' of the even k-step of each pair, 'codes_reversed' a lane's
    8 codes in reverse order, 'halves_swapped' the two halves of a lane's
    first 4-byte word swapped."""
    codes, scales = np.asarray(codes, np.uint8), np.asarray(scales, np.uint8)
    N, K = codes.shape
    n, kt, k = np.arange(N)[:, None], np.arange(K // 32)[None], np.arange(K)
    if broken == "scale_kt+1":
        scales = scales[n, (kt + 1) % (K // 32)]
    elif broken == "scale_n^1":
        scales = scales[np.minimum(n ^ 1, N - 1), kt]
    elif broken == "scale_per_64":
        scales = scales[n, kt & ~1]
    elif broken == "codes_reversed":
        codes = codes[:, k ^ 7]
    elif broken == "halves_swapped":
        codes = codes[:, np.where(k & 4, k, k ^ 2)]
    else:
        assert broken is None, broken
    return mx_decode(codes, scales)


def w8_emulate(a, codes, scales, k0=0, k1=None, broken=None):
    """The W8 path in f32: the codes widened to bf16 exactly, then the 16-bit
    chain (gemm_emulate) on bf16 activations."""
    return gemm_emulate(a, w8_widen(codes, scales, broken), True, k0, k1)
