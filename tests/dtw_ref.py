"""Plain-numpy restatement of the DTW token-timestamp rule (DESIGN.md D8,
steps 2-6), in f64 and f32, the error bounds of the device stages and the
seeded inputs the tests run. Shared by test_dtw_ref.py (CPU) and
test_gpu_dtw.py; not a test module itself and needs no GPU.

Stage contract (k_dtw.hip):
  probs   q = f16((sum of the split-K slabs + bias) * qscale); s_j = f32 dot of
          the f16 values, times scale; p_j = expf(s_j - max) * (float)(1 / double
          sum), kept in f32 (align_qk_kernel)
  cost    per (head, column): mean and population variance over the rows in f32,
          sequentially; z = (w - mean) / sqrt(var), 0 where var == 0; median of
          7 along the columns, reflect padding (skipped when T <= 3);
          cost = -(sum over the heads in order) / A (dtw_cost_kernel)
  path    HF transformers' _dynamic_time_warping recurrence in f32, exact
          (dtw_path_kernel)

Bounds, u = 2^-24 (f32 unit round-off):

probs, against f64 softmax of the same f16 q and K. The f32 dot is 4 chained
v_dot2 steps and a 3-level lane tree: at most 12 roundings on a path, each at
most u times the sum of |q_e k_e|; the scale and the subtraction of the max
round once each (u |s|, 2 u max|s|); expf is taken as 4 u accurate. With
  E = max_j (12 u scale sum_e |q_e k_je|) + 3 u max|s| + 4 u
numerator and denominator of p_j each carry a relative error of at most E, the
reciprocal and the product round once each:
  bound_j = (2 E + 3 u) p_j + 2^-126          (2^-126: results flushed to zero)

cost, against the f64 restatement fed the same f32 probabilities. Column c of a
head has N values w >= 0 with mean m and std s. The sequential f32 sum gives
|dm| <= (N + 1) u m. The deviations d = w - m^ carry -dm each, which cancels to
first order in sum d^2 (sum d = 0), so the variance has relative error at most
(N + 4) u + (dm / s)^2 and the std half of that plus u. With zmax = max|w - m| / s
  ez_c = dm / s + zmax ((N + 8) u / 2 + 3 u + (dm / s)^2 / 2),  dm = (N + 1) u m
(0 for a column whose variance is exactly 0 in both). The median selects one of
its 7 inputs, so its error is at most the largest ez of the 7 columns; the head
sum adds (A + 1) u mean_a |median|:
  bound[n][t] = mean_a max_{|o| <= 3} ez_{a, t+o} + (A + 1) u mean_a |med_a[n][t]| + 2^-126
"""
import numpy as np

U = 2.0 ** -24
MEDIAN_WIDTH = 7
PATH_NS = (2, 3, 63, 64, 65, 226)
PATH_TS = (1, 3, 4, 7, 749, 1500)


# ------------------------------------------------------------------ the rule

def n_columns(n_audio_ctx, remaining_mel_frames):
    """Step 2: T = min(n_audio_ctx, ceil(remaining mel frames / 2))."""
    return max(1, min(n_audio_ctx, (remaining_mel_frames + 1) // 2))


def reflect_index(T):
    """[T][7] column indices of the median window (reflect padding by 3)."""
    t = np.arange(T)[:, None] + np.arange(-3, 4)[None, :]
    t = np.abs(t)
    t = np.where(t >= T, 2 * (T - 1) - t, t)
    return np.clip(t, 0, T - 1)


def normalise(w, dtype=np.float64):
    """Step 4 up to z: w [A][N][T] -> z. f64: numpy's mean / var; f32: the
    kernel's sequential sums."""
    w = np.asarray(w, dtype=dtype)
    N = w.shape[1]
    if dtype == np.float64:
        mean = w.mean(axis=1, keepdims=True)
        var = ((w - mean) ** 2).mean(axis=1, keepdims=True)
    else:
        s = np.zeros_like(w[:, 0])
        for n in range(N):
            s = s + w[:, n]
        mean = (s / dtype(N))[:, None]
        v = np.zeros_like(s)
        for n in range(N):
            d = w[:, n] - mean[:, 0]
            v = v + d * d
        var = (v / dtype(N))[:, None]
    std = np.sqrt(var)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(std > 0, (w - mean) / std, dtype(0))
    return z.astype(dtype), mean[:, 0], std[:, 0]


def median_filter(z):
    """Median of 7 along the last axis with reflect padding; skipped for
    T <= 3 (HF _median_filter). Selects an input element."""
    T = z.shape[-1]
    if T <= MEDIAN_WIDTH // 2:
        return z
    win = z[..., reflect_index(T)]                    # [..., T, 7]
    return np.sort(win, axis=-1)[..., MEDIAN_WIDTH // 2]


def cost_matrix(w, dtype=np.float64):
    """Steps 3-4: probabilities w [A][N][T] (already cut to T columns) ->
    cost [N][T] = -mean_a median7(z)."""
    z, _, _ = normalise(w, dtype)
    med = median_filter(z)
    if dtype == np.float64:
        return -med.mean(axis=0)
    acc = np.zeros_like(med[0])
    for a in range(med.shape[0]):
        acc = acc + med[a]
    return -(acc / dtype(med.shape[0]))


def cost_bound(w):
    """(cost64 [N][T], bound [N][T]) of f32 probabilities w [A][N][T]."""
    w64 = np.asarray(w, dtype=np.float64)
    A, N, T = w64.shape
    z, mean, std = normalise(w64)
    with np.errstate(divide="ignore", invalid="ignore"):
        zmax = np.where(std > 0, np.abs(w64 - mean[:, None]).max(axis=1) / std, 0.0)
        dm = np.where(std > 0, (N + 1) * U * np.abs(mean) / std, 0.0)
    ez = dm + zmax * ((N + 8) * U / 2 + 3 * U + dm * dm / 2)           # [A][T]
    med = median_filter(z)
    if T > MEDIAN_WIDTH // 2:
        ez = ez[:, reflect_index(T)].max(axis=-1)
    bound = ez.mean(axis=0)[None, :] + (A + 1) * U * np.abs(med).mean(axis=0) + 2.0 ** -126
    return -med.mean(axis=0), bound


def dtw(cost, dtype=np.float32):
    """Step 5: HF's _dynamic_time_warping in `dtype`, by anti-diagonals.
    cost [N][T]. Returns (text_indices, time_indices) in path order."""
    m = np.asarray(cost, dtype=dtype)
    N, T = m.shape
    D = np.full((N + 1, T + 1), np.inf, dtype=dtype)
    tr = np.full((N + 1, T + 1), -1, dtype=np.int8)
    D[0, 0] = 0
    for k in range(2, N + T + 1):
        i = np.arange(max(1, k - T), min(N, k - 1) + 1)
        j = k - i
        c0, c1, c2 = D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]
        diag = (c0 < c1) & (c0 < c2)
        up = ~diag & (c1 < c0) & (c1 < c2)
        c = np.where(diag, c0, np.where(up, c1, c2))
        D[i, j] = m[i - 1, j - 1] + c
        tr[i, j] = np.where(diag, 0, np.where(up, 1, 2))
    tr[0, :] = 2
    tr[:, 0] = 1
    i, j = N, T
    ti, tj = [], []
    while i > 0 or j > 0:
        ti.append(i - 1)
        tj.append(j - 1)
        t = tr[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(ti[::-1], np.int64), np.array(tj[::-1], np.int64)


def frames_of_path(text_indices, time_indices, N):
    """Step 6: the column of the path's first step in each row."""
    jumps = np.pad(np.diff(text_indices), (1, 0), constant_values=1).astype(bool)
    fr = time_indices[jumps]
    assert len(fr) == N, (len(fr), N)
    return fr


def frames(cost, dtype=np.float32):
    ti, tj = dtw(cost, dtype)
    return frames_of_path(ti, tj, np.shape(cost)[0])


def token_times(cost, seek, dtype=np.float32):
    """t_dtw of the text tokens of a window (rows 1 .. N-2): seek + 2 frame."""
    return seek + 2 * frames(cost, dtype)[1:-1]


def validate_heads(preset, n_top, heads, n_layer, n_head, preset_geometry=None):
    """The context parameter check (mwx_init_from_file_with_params): the list
    of (layer, head) or None. preset: 'n_top_most', 'custom' or 'model' (then
    preset_geometry = (layers, heads) the preset was made for)."""
    if preset == "n_top_most":
        if not 1 <= n_top <= n_layer:
            return None
        heads = [(l, h) for l in range(n_layer - n_top, n_layer) for h in range(n_head)]
    elif preset == "custom":
        if not heads:
            return None
    elif preset == "model":
        if preset_geometry != (n_layer, n_head):
            return None
    else:
        return None
    if any(not (0 <= l < n_layer and 0 <= h < n_head) for l, h in heads):
        return None
    return list(heads)


# ------------------------------------------------------------------- probs

def probs_ref(q, K, scale):
    """f64 softmax(scale q.K^T) of one (row, head) and its bound. q [64], K
    [n][64]: the f16 values the kernel sees (as any float type)."""
    q64 = np.asarray(q, dtype=np.float64)
    K64 = np.asarray(K, dtype=np.float64)
    sc = float(np.float32(scale))
    s = K64 @ q64 * sc
    p = np.exp(s - s.max())
    p /= p.sum()
    E = 12 * U * sc * (np.abs(K64) @ np.abs(q64)).max() + 3 * U * np.abs(s).max() + 4 * U
    return p, (2 * E + 3 * U) * p + 2.0 ** -126


def e4m3_value(codes):
    """OCP e4m3fn code -> value (no NaN codes expected)."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int32)
    sign = np.where(c & 0x80, -1.0, 1.0)
    ex = (c >> 3) & 0xF
    man = c & 0x7
    return sign * np.where(ex == 0, man * 2.0 ** -9, (1 + man / 8.0) * 2.0 ** (ex - 7.0))


def mx_widen(codes, e8):
    """codes [...][64] with E8M0 exponents e8 [...][2] (one per 32-element
    half) -> the f16 values the kernels widen them to (exact for the ranges
    the tests use)."""
    sc = 2.0 ** (np.asarray(e8, dtype=np.float64) - 127.0)
    v = e4m3_value(codes) * np.repeat(sc, 32, axis=-1)
    h = v.astype(np.float16)
    assert np.array_equal(h.astype(np.float64), v), "widening must be exact in f16"
    return h


# ------------------------------------------------------------------ inputs

def path_cost(kind, seed, N, T):
    """'int': integer values in [-3, 3] (every partial sum exact, ties
    plentiful); 'f32': standard normal f32."""
    rng = np.random.default_rng([seed, N, T, 0 if kind == "int" else 1])
    if kind == "int":
        return rng.integers(-3, 4, size=(N, T)).astype(np.float32)
    return rng.standard_normal((N, T)).astype(np.float32)


def path_shapes():
    """All PATH_NS x PATH_TS shapes in groups of 3 different (N, T): one
    launch each."""
    shapes = [(n, t) for n in PATH_NS for t in PATH_TS]
    order = [shapes[(7 * i) % len(shapes)] for i in range(len(shapes))]   # 7 coprime to 36
    return [tuple(order[i:i + 3]) for i in range(0, len(order), 3)]


def staircase(N, T):
    """Planted alignment: row n owns columns [edge[n], edge[n + 1])."""
    return np.floor(np.linspace(0, T, N + 1)).astype(np.int64)


def planted_probs(seed, A, N, T, n_keys=None, noise=0.05):
    """[A][N][n_keys] f32 rows that sum to 1: each row's mass lies on its
    staircase step (columns < T), over a noise floor on all n_keys columns."""
    n_keys = T if n_keys is None else n_keys
    rng = np.random.default_rng([seed, A, N, T])
    edge = staircase(N, T)
    w = noise * rng.random((A, N, n_keys))
    for n in range(N):
        lo, hi = edge[n], max(edge[n] + 1, edge[n + 1])
        w[:, n, lo:hi] += 1.0 + 0.2 * rng.random((A, hi - lo))
    w /= w.sum(axis=-1, keepdims=True)
    return w.astype(np.float32), edge


def random_probs(seed, A, N, n_keys, temp=2.0):
    """[A][N][n_keys] f32 softmax rows of normal scores (std temp)."""
    rng = np.random.default_rng([seed, A, N, n_keys, 7])
    s = temp * rng.standard_normal((A, N, n_keys))
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    return p.astype(np.float32)
