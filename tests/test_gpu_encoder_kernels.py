"""The encoder kernels one launch at a time against float64 references:
enc_attn_kernel (with its per-clip lens instantiation), gemm_big with the staged
epilogues the encoder uses (conv-stem addressing, tile maps, MX-fp8 operands
and the MX-fp8 cross cache), ln_kernel / ln_dec_kernel and the GELU table.
tests/encoder_ref.py states the contracts, the bounds and the inputs;
test_encoder_ref.py checks the bounds on the CPU. Every case runs the f16 and
the bf16 instantiation through one f16 context (the hooks take the type as a
flag), except the conv stem, which is always f16.

Worst |err| / bound ratios observed on MI355X: see the (observed ...) comments
at each test."""
import numpy as np
import pytest

import encoder_ref as er
import mwx

pytestmark = pytest.mark.gpu

TYPES = [pytest.param(False, id="f16"), pytest.param(True, id="bf16")]
NAN16 = np.uint16(0xFFFF)          # NaN as f16 and as bf16: "not written"
SENT16 = np.uint16(0x7C55)         # an f16 NaN no kernel produces: "untouched"


@pytest.fixture(scope="module")
def ctx(make_model):
    c = mwx.Context.open(make_model("micro"))
    yield c
    c.close()


@pytest.fixture(scope="module")
def gelu_tab(ctx):
    return ctx.test_gelu_table()


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def widen(u16, bf16):
    """16-bit words of type T -> f32."""
    u16 = np.ascontiguousarray(u16, dtype=np.uint16)
    if bf16:
        return (u16.astype(np.uint32) << 16).view(np.float32)
    return u16.view(np.float16).astype(np.float32)


def within(name, got, ref, bound):
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    ratio = np.abs(np.asarray(got, np.float64) - ref) / bound
    i = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert ratio.max() <= 1.0, f"{name}: |err| / bound = {ratio.max():.3f} at {i}"
    return float(ratio.max())


# ---------------------------------------------------------------- attention

def attn_launch(ctx, case, bf16, pad, lens=None):
    return ctx.test_enc_attn(case["q"], case["k"], er.vt_layout(case["v"], pad), bf16=bf16,
                             scale=case["scale"], lens=lens)


def attn_check(o, case, bf16, b, n, name):
    """Rows < n of clip b against float64 attention over n keys."""
    L, H = case["L"], case["H"]
    worst = 0.0
    for h in range(H):
        q, k, v = (case[c][b, h, :n] for c in "qkv")
        o64, bound = er.attention_ref(q, k, v, case["scale"], bf16)
        got = o[b * L:b * L + n, h * 64:(h + 1) * 64]
        worst = max(worst, within(f"{name} head {h}", got, o64, bound))
    return worst


@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("regime", ["diffuse", "sharp_first", "sharp_last"])
def test_attention_every_length(ctx, bf16, regime):
    """A single key, masked and unmasked last tiles, one and two query blocks,
    and the model's own 1500 (a 28-key masked tile, a 92-row last block), with
    the V^T pad columns at +-65504.
    (observed: f16 0.56 / 0.48 / 0.57, bf16 0.81 / 0.88 / 0.88 for diffuse /
    sharp_first / sharp_last)"""
    worst = 0.0
    for L in er.ATTN_LENS:
        case = er.attn_case(L, regime)
        o = attn_launch(ctx, case, bf16, "max")
        worst = max(worst, attn_check(o, case, bf16, 0, L, f"L {L}"))
    print(f"attention {regime}: worst |o - o64| / bound = {worst:.3f}")


@pytest.mark.parametrize("bf16", TYPES)
def test_vt_pad_columns_are_multiplied_by_zero(ctx, bf16):
    """The pad columns [L, Lp) of V^T are read, and must be finite, but never
    reach the output: zeros and +-65504 there give the same bits."""
    for L in (1, 9, 63, 65, 129, 1500):
        case = er.attn_case(L, "sharp_last")
        o0 = attn_launch(ctx, case, bf16, 0.0)
        o1 = attn_launch(ctx, case, bf16, "max")
        assert np.isfinite(o0).all()
        assert np.array_equal(bits(o0), bits(o1)), f"L {L}: the pad columns reached the output"


@pytest.fixture(scope="module")
def vl():
    return er.vl_case()


@pytest.mark.parametrize("bf16", TYPES)
def test_variable_lengths(ctx, vl, bf16):
    """Per-clip lens in one launch: NaN in the Q / K rows and +-65504 in the
    V^T columns past a clip's frames reach no valid row; the valid rows are the
    bits of the clip launched alone; query blocks wholly past the clip are
    zero-filled; every row is finite.
    (observed: f16 0.41, bf16 0.89)"""
    L, H, lens = vl["L"], vl["H"], vl["lens"]
    o = attn_launch(ctx, vl, bf16, 0.0, lens=lens)
    assert np.isfinite(o).all(), "a row past a clip's frames is not finite"
    worst = 0.0
    for b, n in enumerate(lens):
        worst = max(worst, attn_check(o, vl, bf16, b, n, f"clip {b} (lens {n})"))
        first_zero = (n + 127) // 128 * 128
        assert not o[b * L + first_zero:(b + 1) * L].any(), f"clip {b}: block past the clip not zero"
        Ls = (n + 7) & ~7
        alone = dict(q=vl["q"][b:b + 1, :, :Ls], k=vl["k"][b:b + 1, :, :Ls], v=vl["v"][b:b + 1, :, :Ls],
                     scale=vl["scale"], L=Ls, H=H)
        oa = attn_launch(ctx, alone, bf16, 0.0, lens=lens[b:b + 1])
        assert np.array_equal(bits(oa[:n]), bits(o[b * L:b * L + n])), f"clip {b}: differs from alone"
    print(f"attention, variable lengths: worst |o - o64| / bound = {worst:.3f}")


@pytest.mark.parametrize("bf16", TYPES)
def test_lens_equal_to_L_is_the_plain_kernel(ctx, bf16):
    case = er.attn_case(200, "diffuse", B=3)
    o0 = attn_launch(ctx, case, bf16, "max")
    o1 = attn_launch(ctx, case, bf16, "max", lens=np.full(3, 200, np.int32))
    assert np.array_equal(bits(o0), bits(o1))


def test_attention_refusals(ctx):
    case = er.attn_case(64, "diffuse", B=2)
    for lens in ([64, 65], [0, 64], [-1, 3]):
        with pytest.raises(ValueError):
            attn_launch(ctx, case, False, 0.0, lens=np.asarray(lens, np.int32))
    big = er.attn_case(8, "diffuse", B=33, H=2)
    with pytest.raises(ValueError):
        attn_launch(ctx, big, False, 0.0)


# ------------------------------------------------------ GEMM and epilogues

@pytest.fixture
def both_loops():
    """Runs the body under the 2-stage ring and the 8-phase main loop."""
    L = mwx.lib()

    def run(fn):
        out = []
        prev = L.mwx_test_set_gemm_8ph(0)
        try:
            for on in (0, 1):
                L.mwx_test_set_gemm_8ph(on)
                out.append(fn())
        finally:
            L.mwx_test_set_gemm_8ph(-1 if prev < 0 else prev)
        return out
    return run


def gemm_ref(a, w, bf16, mx):
    return er.mx_gemm_ref(a, w, bf16) if mx else er.gemm_acc_ref(a, w, bf16)


def run_res(ctx, a, w, bias, res, bf16, mx=False, ldc=None):
    M, N = res.shape
    ldc = N if ldc is None else ldc
    c = np.full((M, ldc), np.float32(np.nan), np.float32)
    c[:, :N] = res
    c.view(np.uint32)[:, N:] = 0x7FC12345
    out = ctx.test_gemm_enc(mwx.EPI_RES, a, w, bf16=bf16, M=M, bias=bias, c32=c.reshape(-1),
                            ldc=ldc, mx=mx).reshape(M, ldc)
    assert (out.view(np.uint32)[:, N:] == 0x7FC12345).all(), "a word past column N was written"
    return out[:, :N]


def check_res(ctx, a, w, bias, res, bf16, name, mx=False, ldc=None):
    ref, beta = gemm_ref(a, w, bf16, mx)
    y64, by = er.res_ref(ref, beta, bias, res)
    return within(name, run_res(ctx, a, w, bias, res, bf16, mx, ldc), y64, by)


@pytest.mark.parametrize("bf16", TYPES)
def test_gemm_k_pipeline(ctx, both_loops, bf16):
    """The K loop's prologue, steady state and drain from one 64-deep tile to
    80 (an odd tile count too), by both main loops, with the bias and the
    residual in the epilogue. (observed: f16 0.059, bf16 0.053)"""
    worst = 0.0
    for K in (64, 128, 192, 1280, 5120):
        a, w, bias, res = er.gemm_inputs(0, 260, 256, K)
        ref, beta = er.gemm_acc_ref(a, w, bf16)
        y64, by = er.res_ref(ref, beta, bias, res)
        outs = both_loops(lambda: run_res(ctx, a, w, bias, res, bf16))
        worst = max(worst, within(f"K {K}", outs[0], y64, by))
        assert np.array_equal(bits(outs[0]), bits(outs[1])), f"K {K}: the 8-phase loop differs"
        nobias, _ = er.res_ref(ref, beta, None, res)
        assert (np.abs(nobias - y64) > by).mean() > 0.9  # (the inputs would show a dropped bias)
    print(f"GEMM K pipeline: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("bf16", TYPES)
def test_gemm_tile_maps(ctx, gelu_tab, both_loops, bf16):
    """10 x 2 tiles: XCD remainder 4, a last group of two row tiles, a 4-row
    and a 64-column tail. In place (EPI_RES) a tile run twice or not at all
    leaves a wrong value; EPI_GELU starts from NaN words. Nothing outside
    [M][N] is written (row stride N + 8, the hook's guard bands).
    (observed: EPI_RES f16 0.028, bf16 0.028)"""
    M, N, K = 2308, 320, 128
    a, w, bias, res = er.gemm_inputs(1, M, N, K)
    outs = both_loops(lambda: check_res(ctx, a, w, bias, res, bf16, "EPI_RES", ldc=N + 8))
    print(f"GEMM tile maps, EPI_RES: worst |err| / bound = {max(outs):.3f}")
    gelu_check(ctx, gelu_tab, a, w, bias, bf16, ldc=N + 8)


def gelu_check(ctx, tab, a, w, bias, bf16, out16=False, mx=False, ldc=None, use_table=True):
    M, N = a.shape[0], w.shape[0]
    ldc = N if ldc is None else ldc
    c = np.full((M, ldc), NAN16)
    c[:, N:] = SENT16
    out = ctx.test_gemm_enc(mwx.EPI_GELU, a, w, bf16=bf16, M=M, bias=bias, c16=c.reshape(-1),
                            ldc=ldc, out16=out16, mx=mx, use_table=use_table).reshape(M, ldc)
    assert (out[:, N:] == SENT16).all(), "a word past column N was written"
    f16_out = out16 or not bf16
    got = widen(out[:, :N], not f16_out)
    assert np.isfinite(got).all(), "an output was not written"
    ref, beta = gemm_ref(a, w, bf16, mx)
    x64, bx = er.add_bound(ref, beta, bias.astype(np.float64)[None])
    ok = er.gelu_candidates_ok(got, x64, bx, tab, lambda g, sel: er.round_t(g, not f16_out))
    assert ok.all(), (f"{(~ok).sum()} outputs are no table value of an f16 input within the "
                      f"bound, first at {np.argwhere(~ok)[0]}")
    return out[:, :N]


@pytest.mark.parametrize("bf16", TYPES)
def test_gelu_epilogue_is_the_table(ctx, gelu_tab, bf16):
    """FFN1's epilogue with pre-activations spread over [-14, 14] (both
    saturation branches and every f16 exponent between): every output is the
    table's value at an f16 input within the accumulator bound, by table lookup
    and by tanhf alike."""
    a, w, _, _ = er.gemm_inputs(2, 300, 256, 128)
    bias = np.linspace(-14.0, 14.0, 256).astype(np.float32)
    t = gelu_check(ctx, gelu_tab, a, w, bias, bf16)
    f = gelu_check(ctx, gelu_tab, a, w, bias, bf16, use_table=False)
    assert np.array_equal(t, f)


def test_gelu_table_exhaustive(gelu_tab):
    """Every entry of the device-built table against float64 GELU: half an f16
    ulp plus the tanhf term (encoder_ref.TANH_ULPS).
    (observed: the table admits 0.798 ulps: an f16 tie of 0.5 h at the
    smallest subnormal, the f32 rounding of gelu_f32 itself; tanhf adds nothing
    beyond it)"""
    assert len(gelu_tab) >= 2 * er.GELU_TAB_HALF and not gelu_tab[2 * er.GELU_TAB_HALF:].any()
    t = er.gelu_table_admits(gelu_tab)
    print(f"GELU table: the smallest tanhf error the float64 reference admits = {t:.3f} ulps")
    tab = gelu_tab[:2 * er.GELU_TAB_HALF].view(np.float16).astype(np.float64)
    g, bound = er.gelu_table_bound()
    assert np.isfinite(tab).all()
    bad = np.abs(tab - g) > bound
    assert not bad.any(), f"{bad.sum()} entries, first h = {er.gelu_table_inputs()[bad][0]}"


def qkv_check(ctx, bf16, B, L, H, K, ldv, mx=False, seed=3):
    d, M = H * 64, B * L
    N = 3 * d
    a, w, bias, _ = er.gemm_inputs(seed, M, N, K)
    sent = lambda n: np.full(n, SENT16)
    q, k, v = ctx.test_gemm_enc(mwx.EPI_ENC_QKV, a, w, bf16=bf16, M=M, bias=bias, L=L, H=H, d=d,
                                ldv=ldv, q=sent(M * d), k=sent(M * d), v=sent(B * d * ldv), mx=mx)
    ref, beta = gemm_ref(a, w, bf16, mx)
    x64, bx = er.add_bound(ref, beta, bias.astype(np.float64)[None])
    bound = er.f16_store_bound(x64, bx)
    # [M][3][H][64] -> [B][H][L][64]
    part = lambda p: np.moveaxis(p.reshape(B, L, 3, H, 64), 1, 3)
    x64, bound = part(x64), part(bound)
    worst = within("q", widen(q, False).reshape(B, H, L, 64), x64[:, 0], bound[:, 0])
    worst = max(worst, within("k", widen(k, False).reshape(B, H, L, 64), x64[:, 1], bound[:, 1]))
    v = v.reshape(B, H, 64, ldv)
    assert (v[..., L:] == SENT16).all(), "a V^T pad column was written"
    worst = max(worst, within("V^T", widen(v[..., :L], False), np.swapaxes(x64[:, 2], 2, 3),
                              np.swapaxes(bound[:, 2], 2, 3)))
    return worst


@pytest.mark.parametrize("bf16", TYPES)
def test_enc_qkv_epilogue(ctx, bf16):
    """Head-major q and k, V^T by 8-byte stores at [b][h][e][t] with row stride
    104 > L = 100 (the pad columns keep their sentinel), and L = 8 with 33
    clips, whose boundaries fall inside one wave's 128 t.
    (observed: f16 0.968, bf16 0.968: the f16 store's half-ulp)"""
    worst = max(qkv_check(ctx, bf16, 3, 100, 2, 128, 104), qkv_check(ctx, bf16, 33, 8, 2, 128, 8))
    print(f"EPI_ENC_QKV: worst |err| / bound = {worst:.3f}")


def cross_inputs(seed, B, L, K, d, layers):
    """A clip row of zeros and biases chosen so that row's V holds one MX
    block of all zeros and one whose amax is exactly 448 2^-3."""
    N = layers * 2 * d
    a, w, bias, _ = er.gemm_inputs(seed, B * L, N, K)
    a[L + 5] = 0.0
    bias[d:d + 32] = 0.0
    bias[d + 32:d + 64] = np.clip(bias[d + 32:d + 64], -50.0, 50.0)
    bias[d + 40] = 56.0
    return a, w, bias


def cross_ref(a, w, bias, bf16, mx, kscale, B, L, H, layers):
    """(x64, bound) as [layers][2][B][H][L][64]."""
    ref, beta = gemm_ref(a, w, bf16, mx)
    d = H * 64
    isv = (np.arange(ref.shape[1]) % (2 * d)) >= d
    xk, bk = er.kscale_bound(ref, beta, kscale)
    xv, bv = er.add_bound(ref, beta, bias.astype(np.float64)[None])
    x, bx = np.where(isv, xv, xk), np.where(isv, bv, bk)
    lay = lambda p: np.transpose(p.reshape(B, L, layers, 2, H, 64), (2, 3, 0, 4, 1, 5))
    return lay(x), lay(er.f16_store_bound(x, bx))


CROSS = dict(B=3, L=96, lcap=104, ncap=5, slot=(4, 0, 2), H=2, layers=2)


def cross_launch(ctx, a, w, bias, bf16, kscale, mx=False, kv8=False, B=3, L=96, lcap=104, ncap=5,
                 slot=(4, 0, 2), H=2, layers=2):
    d = H * 64
    n = layers * ncap * H * lcap * 64
    args = dict(bf16=bf16, M=B * L, bias=bias, L=L, H=H, d=d, lcap=lcap, ncap=ncap,
                slot=np.asarray(slot, np.int32), kscale=kscale, mx=mx)
    shape = (layers, ncap, H, lcap, 64)
    if kv8:
        k8, v8, ks8, vs8 = ctx.test_gemm_enc(
            mwx.EPI_CROSS_KV, a, w, kv8=(np.full(n, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8),
                                         np.full(n // 32, 0x5A, np.uint8),
                                         np.full(n // 32, 0x5A, np.uint8)), **args)
        return k8.reshape(shape), v8.reshape(shape), ks8.reshape(shape[:4] + (2,)), \
            vs8.reshape(shape[:4] + (2,))
    k, v = ctx.test_gemm_enc(mwx.EPI_CROSS_KV, a, w, k=np.full(n, SENT16), v=np.full(n, SENT16),
                             **args)
    return k.reshape(shape), v.reshape(shape)


def cross_check(ctx, bf16, K, mx=False, **geo):
    g = dict(CROSS, **geo)
    B, L, H, layers, slot = g["B"], g["L"], g["H"], g["layers"], g["slot"]
    kscale = er.KQS
    a, w, bias = cross_inputs(4, B, L, K, H * 64, layers)
    k, v = cross_launch(ctx, a, w, bias, bf16, kscale, mx=mx, **g)
    x64, bound = cross_ref(a, w, bias, bf16, mx, kscale, B, L, H, layers)
    worst = 0.0
    written = np.zeros(k.shape[:4], bool)
    for b, s in enumerate(slot):
        written[:, s, :, :L] = True
        for kv, c in enumerate((k, v)):
            worst = max(worst, within(f"{'KV'[kv]} clip {b}", widen(c[:, s, :, :L], False),
                                      x64[:, kv, b], bound[:, kv, b]))
    for c in (k, v):
        assert (c[~written] == SENT16).all(), "a cache row outside the clips' rows was written"
    assert not v[0, slot[1], 0, 5, :32].any() and widen(v[0, slot[1], 0, 5, 40], False) == 56.0
    return worst, (a, w, bias, kscale, k, v, written)


@pytest.mark.parametrize("bf16", TYPES)
def test_cross_kv_epilogue(ctx, bf16):
    """All layers' cross K / V in one GEMM into permuted cache slots: rows
    96 .. 103 of every slot and the unused slots keep their sentinel. With the
    MX-fp8 cache, the codes and scales are the host block rule applied to the
    f16 cache's values (the same accumulations), bit for bit, including an
    all-zero block and one with amax on the 448 2^e edge.
    (observed: f16 0.967, bf16 0.962)"""
    worst, (a, w, bias, kscale, k, v, written) = cross_check(ctx, bf16, 128)
    print(f"EPI_CROSS_KV: worst |err| / bound = {worst:.3f}")
    k8, v8, ks8, vs8 = cross_launch(ctx, a, w, bias, bf16, kscale, kv8=True)
    for name, c16, c8, s8 in (("K", k, k8, ks8), ("V", v, v8, vs8)):
        codes, scales = er.mx_encode(widen(c16[written], False))
        assert np.array_equal(c8[written], codes), f"{name}: e4m3 codes differ from the block rule"
        assert np.array_equal(s8[written], scales), f"{name}: E8M0 scales differ"
        assert (c8[~written] == 0xA5).all() and (s8[~written] == 0x5A).all()
    s1 = CROSS["slot"][1]  # the clip whose row 5 is zero in A
    assert (vs8[0, s1, 0, 5] == (127, 127 - 3)).all() and not v8[0, s1, 0, 5, :32].any()


@pytest.mark.parametrize("bf16", TYPES)
def test_small_tiles_every_epilogue(ctx, gelu_tab, bf16):
    """(300, 192, 64): one K tile, a column tile of 192 (one wave column idle)
    and a 44-row tail, through every flat epilogue and EPI_ENC_QKV (d = 64).
    EPI_CROSS_KV needs N % 128 == 0: (300, 256, 64) with one layer.
    (observed: f16 0.979, bf16 0.978)"""
    M, N, K = 300, 192, 64
    a, w, bias, res = er.gemm_inputs(5, M, N, K)
    worst = check_res(ctx, a, w, bias, res, bf16, "EPI_RES")
    ref, beta = er.gemm_acc_ref(a, w, bf16)
    y64, by = er.res_ref(ref, beta, None, res)
    worst = max(worst, within("EPI_RES, no bias", run_res(ctx, a, w, None, res, bf16), y64, by))
    gelu_check(ctx, gelu_tab, a, w, bias, bf16)
    gelu_check(ctx, gelu_tab, a, w, bias, bf16, out16=True)
    conv2_check(ctx, gelu_tab, a, w, bias, res, bf16)
    worst = max(worst, qkv_check(ctx, bf16, 3, 100, 1, 64, 100, seed=5))
    w2, _ = cross_check(ctx, bf16, 64, B=3, L=100, lcap=100, ncap=3, slot=(2, 1, 0), H=2, layers=1)
    print(f"small tiles: worst |err| / bound = {max(worst, w2):.3f}")


def conv2_check(ctx, tab, a, w, bias, pe, bf16, **kw):
    """EPI_CONV2 on a [M][K] (or a strided view given by kw): every output is
    f32(pe + table value) for an f16 input within the bound."""
    M, N = pe.shape
    out = ctx.test_gemm_enc(mwx.EPI_CONV2, kw.pop("a_flat", a), w, bf16=bf16, M=M, bias=bias, pe=pe,
                            c32=np.full(M * N, np.float32(np.nan)), **kw).reshape(M, N)
    assert np.isfinite(out).all(), "an output was not written"
    ref, beta = er.gemm_acc_ref(a, w, bf16)
    x64, bx = er.add_bound(ref, beta, bias.astype(np.float64)[None])
    ok = er.gelu_candidates_ok(out, x64, bx, tab, lambda g, sel: pe.reshape(-1)[sel] + g)
    assert ok.all(), f"{(~ok).sum()} outputs, first at {np.argwhere(~ok)[0]}"
    return out


def test_conv_stem_forms(ctx, gelu_tab):
    """The conv stem as the engine runs it (always f16): conv1 reads
    overlapping rows (lda = 128 < K = 384) of three clips (a_bstride) and writes
    f16 rows 1 .. 200 of each clip's [202][d] buffer (c16 offset d), leaving
    the zero-pad rows 0 and 201 alone; conv2 reads that layout with stride 2
    (lda = 2 d, K = 3 d) and adds the positional embedding. Against float64
    im2col references; a batched launch equals three single launches."""
    cp, d, T2, B = 128, 128, 200, 3
    rng = np.random.default_rng(6)
    x = rng.standard_normal((B, T2 + 2, cp)).astype(np.float32)
    x[:, 0] = x[:, -1] = 0.0
    _, w1, _, _ = er.gemm_inputs(6, T2, d, 3 * cp)
    bias = np.linspace(-12.0, 12.0, d).astype(np.float32)
    blank = np.full((B, T2 + 2, d), SENT16)
    conv1 = dict(bf16=False, M=T2, lda=cp, bias=bias, ldc=d, c_off=d, out16=True)
    y = ctx.test_gemm_enc(mwx.EPI_GELU, x, w1, batch=B, a_bstride=(T2 + 2) * cp,
                          c_bstride=(T2 + 2) * d, c16=blank.reshape(-1), **conv1).reshape(blank.shape)
    assert (y[:, 0] == SENT16).all() and (y[:, -1] == SENT16).all(), "a pad row was written"
    finish = lambda g, sel: er.round_t(g, False)
    for b in range(B):
        ref, beta = er.gemm_acc_ref(er.im2col(er.round_t(x[b], False)), w1, False)
        x64, bx = er.add_bound(ref, beta, bias.astype(np.float64)[None])
        assert er.gelu_candidates_ok(widen(y[b, 1:-1], False), x64, bx, gelu_tab, finish).all(), b
        one = ctx.test_gemm_enc(mwx.EPI_GELU, x[b], w1, c16=blank[0].reshape(-1), **conv1)
        assert np.array_equal(one.reshape(blank[0].shape), y[b]), f"clip {b}: batched != single"
    # conv2 over conv1's layout, its pad rows zero as the engine keeps them
    h = widen(y, False).reshape(y.shape)
    h[:, 0] = h[:, -1] = 0.0
    M2 = T2 // 2
    _, w2, bias2, pe = er.gemm_inputs(7, M2, d, 3 * d)
    conv2 = dict(M=M2, lda=2 * d)
    out = ctx.test_gemm_enc(mwx.EPI_CONV2, h, w2, bf16=False, bias=bias2, pe=pe, batch=B,
                            a_bstride=(T2 + 2) * d, c_bstride=M2 * d,
                            c32=np.full(B * M2 * d, np.float32(np.nan)), **conv2).reshape(B, M2, d)
    for b in range(B):
        one = conv2_check(ctx, gelu_tab, er.im2col(h[b], stride=2), w2, bias2, pe, False,
                          a_flat=h[b], lda=2 * d)
        assert np.array_equal(bits(one), bits(out[b])), f"clip {b}: batched != single"


@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("K", [128, 256])
def test_mx_operands(ctx, gelu_tab, bf16, K):
    """The MX-fp8 compute mode (device activation quantizer, host weight
    quantizer, block-scaled MFMA) through the four epilogues it serves, with
    test_mx_gemm_exact's accumulator criterion.
    (observed: 0.890 at K 128, 0.911 at K 256, f16 and bf16 alike)"""
    M = 300
    a, w, bias, res = er.gemm_inputs(8, M, 384, K)
    worst = check_res(ctx, a, w, bias, res, bf16, "EPI_RES", mx=True)
    gelu_check(ctx, gelu_tab, a, w, bias, bf16, mx=True)
    worst = max(worst, qkv_check(ctx, bf16, 3, 100, 2, K, 104, mx=True))
    w2, _ = cross_check(ctx, bf16, K, mx=True, B=3, L=100, lcap=104)
    print(f"MX operands K {K}: worst |err| / bound = {max(worst, w2):.3f}")


def test_gemm_refusals(ctx):
    """Every refusal is decided on the host: nothing is launched."""
    a, w, bias, res = er.gemm_inputs(9, 96, 128, 64)
    qkv = dict(bf16=False, M=96, bias=np.zeros(192, np.float32), H=1, d=64)
    w3 = np.zeros((192, 64), np.float32)
    sent = lambda n: np.full(n, SENT16)
    with pytest.raises(ValueError):   # L % 4: a 4-t group would straddle two clips
        ctx.test_gemm_enc(mwx.EPI_ENC_QKV, np.zeros((98, 64), np.float32), w3, L=98, ldv=104,
                          q=sent(98 * 64), k=sent(98 * 64), v=sent(64 * 104), **dict(qkv, M=98))
    with pytest.raises(ValueError):   # M % L
        ctx.test_gemm_enc(mwx.EPI_ENC_QKV, a, w3, L=64, ldv=64, q=sent(64 * 64), k=sent(64 * 64),
                          v=sent(64 * 64), **qkv)
    cross = dict(bf16=False, M=96, bias=bias, L=32, H=1, d=64, lcap=32, ncap=3,
                 k=sent(3 * 32 * 64), v=sent(3 * 32 * 64))
    for slot in ([0, 1, 3], [0, -1, 2], [0, 1, 1]):
        with pytest.raises(ValueError):
            ctx.test_gemm_enc(mwx.EPI_CROSS_KV, a, w, slot=slot, **cross)
    c32 = np.zeros(96 * 128, np.float32)
    with pytest.raises(ValueError):   # a too short for lda
        ctx.test_gemm_enc(mwx.EPI_RES, a, w, bf16=False, M=96, lda=72, c32=c32)
    with pytest.raises(ValueError):   # a too short for a_bstride
        ctx.test_gemm_enc(mwx.EPI_RES, a, w, bf16=False, M=96, batch=2, a_bstride=64,
                          c_bstride=96 * 128, c32=np.zeros(2 * 96 * 128, np.float32))
    with pytest.raises(ValueError):   # N % 64
        ctx.test_gemm_enc(mwx.EPI_RES, a, w[:100], bf16=False, M=96, c32=np.zeros(9600, np.float32))
    with pytest.raises(ValueError):   # c too short
        ctx.test_gemm_enc(mwx.EPI_RES, a, w, bf16=False, M=96, c32=c32[:-1])


# ---------------------------------------------------------------- LayerNorm

def ln_check(case, y, x1, bf16, x_in, name):
    """Active rows within the bound of the reference over x_in; inactive rows:
    y not written, x unchanged; constant rows give T(b) exactly."""
    act = case["active"].astype(bool)
    assert np.isnan(y[~act]).all(), f"{name}: an inactive row was written"
    assert np.array_equal(bits(x1[~act]), bits(case["x"][~act])), f"{name}: inactive x changed"
    assert np.array_equal(bits(x1[act]), bits(x_in[act])), f"{name}: x differs"
    y64, bound = er.ln_ref(x_in, case["w"], case["b"], bf16)
    assert np.isfinite(y64).all()
    return within(name, y[act], y64[act], bound[act])


@pytest.mark.parametrize("bf16", TYPES)
def test_layer_norm_shapes(ctx, bf16):
    """Every NPT instantiation and a partial last pass; unit-normal rows, rows
    of mean 100 and std 0.01, constant rows and rows near 2^60; an active mask.
    The decode kernel gives the same bits.
    (observed: f16 0.997, bf16 0.996: the output's half-ulp)"""
    worst = 0.0
    for N in er.LN_NS:
        c = er.ln_case(N)
        y, x1 = ctx.test_layer_norm(c["x"], c["w"], c["b"], bf16=bf16, active=c["active"])
        worst = max(worst, ln_check(c, y, x1, bf16, c["x"], f"N {N}"))
        const = (np.arange(er.LN_M) % 4 == 2) & c["active"].astype(bool)
        assert np.array_equal(y[const], np.broadcast_to(er.round_t(c["b"], bf16), y.shape)[const])
        yd, xd = ctx.test_layer_norm(c["x"], c["w"], c["b"], bf16=bf16, active=c["active"], dec=True)
        assert np.array_equal(bits(yd), bits(y)) and np.array_equal(bits(xd), bits(x1)), N
        yn, _ = ctx.test_layer_norm(c["x"], c["w"], c["b"], bf16=bf16)
        assert np.isfinite(yn).all() and np.array_equal(bits(yn[const]), bits(y[const]))
    print(f"LayerNorm: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("KS", [1, 5, 8])
def test_layer_norm_split_k_input(ctx, bf16, KS):
    """x = (sum of the slabs in ks order + pbias) + x, written back bit for bit,
    then normalised; the decode kernel gives the same bits.
    (observed: f16 0.995, bf16 0.995 / 0.994 / 0.994 for KS 1 / 5 / 8)"""
    worst = 0.0
    for N in (64, 768, 2048):
        c = er.ln_case(N, seed=1)
        P, pb = er.ln_slabs(c["x"], KS)
        x_in = er.ln_fold(c["x"], P, pb)
        y, x1 = ctx.test_layer_norm(c["x"], c["w"], c["b"], bf16=bf16, active=c["active"], P=P,
                                    pbias=pb)
        worst = max(worst, ln_check(c, y, x1, bf16, x_in, f"N {N} KS {KS}"))
        yd, xd = ctx.test_layer_norm(c["x"], c["w"], c["b"], bf16=bf16, active=c["active"], P=P,
                                     pbias=pb, dec=True)
        assert np.array_equal(bits(yd), bits(y)) and np.array_equal(bits(xd), bits(x1)), N
    print(f"LayerNorm, split-K input KS {KS}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("bf16", TYPES)
def test_layer_norm_dec_embedding(ctx, bf16):
    """EmbedIn: x = T(te[tok]) + pe[pos] bit for bit, then normalised; inactive
    rows carry out-of-range ids and positions, which the kernel clamps before
    it reads. (observed: f16 0.992, bf16 0.987)"""
    N, M, n_tok, n_pos = 384, er.LN_M, 50, 20
    c = er.ln_case(N, seed=2)
    rng = np.random.default_rng(12)
    te = rng.standard_normal((n_tok, N)).astype(np.float32)
    pe = rng.standard_normal((n_pos, N)).astype(np.float32)
    tok = rng.integers(0, n_tok, M).astype(np.int32)
    pos = rng.integers(0, n_pos, M).astype(np.int32)
    tok[0], pos[0], tok[1], pos[1] = 0, n_pos - 1, n_tok - 1, 0
    off = np.flatnonzero(c["active"] == 0)
    tok[off] = [2 ** 31 - 1, -5, n_tok, -2 ** 31][:len(off)] + [n_tok] * max(0, len(off) - 4)
    pos[off] = [-1, 2 ** 31 - 1, n_pos, -2 ** 31][:len(off)] + [n_pos] * max(0, len(off) - 4)
    act = c["active"].astype(bool)
    x_in = c["x"].copy()
    x_in[act] = er.round_t(te, bf16)[tok[act]] + pe[pos[act]]
    y, x1 = ctx.test_layer_norm(c["x"], c["w"], c["b"], bf16=bf16, dec=True, active=c["active"],
                                te=te, pe=pe, tok=tok, pos=pos)
    worst = ln_check(c, y, x1, bf16, x_in, "EmbedIn")
    print(f"LayerNorm, EmbedIn: worst |err| / bound = {worst:.3f}")


def test_layer_norm_refuses_wide_rows(ctx):
    """layer_norm launches nothing for N > 2048: the hook reports the shape as
    not served instead of returning unwritten rows."""
    c = er.ln_case(2056, M=2)
    for dec in (False, True):
        with pytest.raises(NotImplementedError):
            ctx.test_layer_norm(c["x"], c["w"], c["b"], bf16=False, dec=dec)
    with pytest.raises(NotImplementedError):  # the decode kernel's 32-deep tiles
        ctx.test_layer_norm(c["x"][:, :72], c["w"][:72], c["b"][:72], bf16=False, dec=True)
