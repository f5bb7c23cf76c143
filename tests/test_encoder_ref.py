"""CPU checks of tests/encoder_ref.py: the f32 / f16 emulations of the encoder
kernels' roundings stay within the derived bounds on every input set the GPU
tests use (plus a seed sweep), deliberately broken emulations exceed them, and
the chosen shapes reach the branches they are meant to. No GPU."""
import numpy as np
import pytest

import encoder_ref as er

TYPES = [pytest.param(False, id="f16"), pytest.param(True, id="bf16")]
REGIMES = ("diffuse", "sharp_first", "sharp_last")


def attn_ratio(case, bf16, pad, broken=None, n=None, b=0):
    """Worst |emulation - o64| / bound over the heads of clip b (n keys)."""
    L = case["L"]
    n = L if n is None else n
    vt = er.vt_layout(case["v"], pad)
    worst = 0.0
    for h in range(case["H"]):
        q, k, v = (case[c][b, h, :n] for c in "qkv")
        o64, bound = er.attention_ref(q, k, v, case["scale"], bf16)
        o = er.attention_emulate(q, case["k"][b, h], vt[b, h], n, case["scale"], bf16, broken)
        assert np.isfinite(o).all()
        worst = max(worst, er.worst_ratio(o, o64, bound))
    return worst


@pytest.mark.parametrize("bf16", TYPES)
def test_attention_emulation_within_bound(bf16):
    worst = {}
    for regime in REGIMES:
        for L in er.ATTN_LENS:
            seeds = (0,) if L == 1500 else (0, 1, 2)
            for seed in seeds:
                r = attn_ratio(er.attn_case(L, regime, seed), bf16, "max")
                worst[regime] = max(worst.get(regime, 0.0), r)
                assert r <= 1.0, (regime, L, seed, r)
    vl = er.vl_case()
    for b, n in enumerate(er.VL_LENS):
        r = attn_ratio(vl, bf16, 0.0, n=n, b=b)
        worst["vl"] = max(worst.get("vl", 0.0), r)
        assert r <= 1.0, (b, n, r)
    print("attention emulation, worst |err| / bound:", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("bf16", TYPES)
def test_pad_columns_do_not_reach_the_output(bf16):
    """Zero and +-65504 pad columns give the same bits (they meet p = 0)."""
    for L in (9, 65, 200, 1500):
        c = er.attn_case(L, "sharp_last")
        o = [er.attention_emulate(c["q"][0, 0], c["k"][0, 0], er.vt_layout(c["v"], p)[0, 0], L,
                                  c["scale"], bf16) for p in (0.0, "max")]
        assert np.array_equal(o[0].view(np.uint32), o[1].view(np.uint32))


@pytest.mark.parametrize("bf16", TYPES)
@pytest.mark.parametrize("broken,L,regime,pad", [
    ("drop_last", 1500, "sharp_last", 0.0),
    ("mask+1", 1500, "sharp_last", 0.0),
    ("mask+1", 200, "diffuse", "max"),
    ("no_alpha", 1500, "sharp_last", 0.0),
    ("no_alpha", 129, "sharp_last", 0.0),
    ("swap8", 1500, "sharp_first", 0.0),
    ("swap8", 9, "diffuse", 0.0),
])
def test_broken_attention_exceeds_bound(bf16, broken, L, regime, pad):
    c = er.attn_case(L, regime)
    assert attn_ratio(c, bf16, pad) <= 1.0
    r = attn_ratio(c, bf16, pad, broken)
    print(f"{broken} L {L} {regime}: |err| / bound = {r:.1f}")
    assert r > 1.0


def test_attention_shapes_cover_the_paths():
    Ls = er.ATTN_LENS
    assert any(L % 64 == 0 for L in Ls) and any(L % 64 for L in Ls)      # unmasked / masked last tile
    assert 1 in Ls and any(L < 64 for L in Ls) and any(L > 64 and L % 64 for L in Ls)
    assert any(L <= 128 for L in Ls) and any(128 < L <= 256 for L in Ls)  # one / two query blocks
    assert any(L % 8 for L in Ls) and any(L % 8 == 0 for L in Ls)        # V^T pad columns or none
    assert 1500 % 64 == 28 and 1500 % 128 == 92
    blocks = [er.attn_query_blocks(er.VL_L, n) for n in er.VL_LENS]
    assert any(z > 0 for _, z in blocks) and any(z == 0 for _, z in blocks)  # zero-filled blocks
    assert any(n % 64 == 0 and n < er.VL_L for n in er.VL_LENS)          # unmasked short clip
    assert any(n % 128 and r == 2 for (r, _), n in zip(blocks, er.VL_LENS))  # clamped rows in a block
    # 'sharp' really is: exp2 underflows f16 and the last-tile maximum moves alpha
    c = er.attn_case(1500, "sharp_last")
    s = c["q"][0, 0].astype(np.float64) @ c["k"][0, 0].astype(np.float64).T * c["scale"]
    assert np.abs(s).max() > 30 and (s.argmax(axis=1) == 1499).mean() > 0.9
    assert (np.exp(s - s.max(axis=1, keepdims=True)) < 2.0 ** -24).mean() > 0.5


# -------------------------------------------------------------------- GEMM

GEMM_GRIDS = [(260, 256), (2308, 320), (300, 192), (300, 384), (264, 384), (288, 512), (200, 128)]


def test_tile_map_is_a_bijection():
    for M, N in GEMM_GRIDS + [(4096, 2048), (1500, 1280)]:
        for group_m in (0, 8):
            for remap in (False, True):
                tiles = er.gemm_tile_map(M, N, group_m, remap)
                nbm, nbn = (M + 255) // 256, (N + 255) // 256
                assert sorted(tiles) == [(i, j) for i in range(nbm) for j in range(nbn)], (M, N)
    # the tile-map case: 20 workgroups = XCD remainder 4, a last group of 2 row
    # tiles, a 4-row tail and a 64-column tail
    nbm, nbn = (2308 + 255) // 256, (320 + 255) // 256
    assert (nbm, nbn) == (10, 2) and (nbm * nbn) % 8 == 4 and nbm % 8 == 2
    assert 2308 % 256 == 4 and 320 % 256 == 64


@pytest.mark.parametrize("bf16", TYPES)
def test_gemm_emulation_and_dropped_tile(bf16):
    worst = 0.0
    for K in (64, 128, 192, 1280):
        a, w, bias, res = er.gemm_inputs(0, 24, 64, K)
        ref, beta = er.gemm_acc_ref(a, w, bf16)
        acc = er.gemm_emulate(a, w, bf16)
        worst = max(worst, er.worst_ratio(acc, ref, beta))
        y64, by = er.res_ref(ref, beta, bias, res)
        y = (acc + bias[None]) + res
        assert y.dtype == np.float32
        worst = max(worst, er.worst_ratio(y, y64, by))
        x64, bx = er.add_bound(ref, beta, bias.astype(np.float64)[None])
        worst = max(worst, er.worst_ratio(er.f16(acc + bias[None]), x64, er.f16_store_bound(x64, bx)))
        k64, bk = er.kscale_bound(ref, beta, 0.3535)
        worst = max(worst, er.worst_ratio(er.f16(acc * np.float32(0.3535)), k64,
                                          er.f16_store_bound(k64, bk)))
        for t in range(K // 64):
            bad = (er.gemm_emulate(a, w, bf16, drop_tile=t) + bias[None]) + res
            # a dropped tile moves nearly every output by far more than the bound
            assert (np.abs(bad - y64) > by).mean() > 0.9, (K, t)
        # a dropped bias shows
        assert (np.abs((acc + res) - y64) > by).mean() > 0.9
    assert worst <= 1.0
    print(f"GEMM emulation: worst |err| / bound = {worst:.3f}")


def test_mx_codes_follow_the_block_rule():
    """mx_encode / mx_decode give np_mx_round's values, on blocks that include
    all zeros, amax on the 448 2^e edge and just past it, e4m3 subnormals, ties
    and negative values that round to zero."""
    from test_quant_format import np_mx_round
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((64, 32)) * np.exp2(rng.integers(-12, 12, (64, 1)))).astype(np.float32)
    x[0] = 0.0
    x[1, 0], x[2, 0], x[3, 0] = 448.0 * 2.0 ** 3, 448.0 * 2.0 ** -5, np.float32(448.0 * (1 + 2.0 ** -20))
    x[1, 1:] *= 0.01
    x[4] = -np.abs(x[4]) / np.abs(x[4]).max() * np.float32(2.0 ** -12)
    x[4, 0] = 300.0
    x[5, :8] = [1.0625, 1.1875, 0.001, -0.0009, 2.0 ** -10, -2.0 ** -10, 3 * 2.0 ** -10, 0.0]
    x[5, 8] = 440.0
    codes, scales = er.mx_encode(x)
    assert np.array_equal(er.mx_decode(codes, scales).reshape(-1), np_mx_round(x))
    assert scales[0, 0] == 127 and not codes[0].any()
    assert scales[1, 0] == 127 + 3 and codes[1, 0] == 0x7E and scales[3, 0] == 128
    assert (codes[4, 1:] & 0x7F == 0).all() and (codes[4, 1:] & 0x80).any()  # signed zeros


def test_vt_written_one_column_late_shows():
    """V^T [e][t] against the reference at [e][t + 1]: far outside the bound."""
    a, w, bias, _ = er.gemm_inputs(1, 16, 64, 64)
    ref, beta = er.gemm_acc_ref(a, w, False)
    x64, bx = er.add_bound(ref, beta, bias.astype(np.float64)[None])
    v = er.f16(er.gemm_emulate(a, w, False) + bias[None]).astype(np.float64)
    bound = er.f16_store_bound(x64, bx)
    assert (np.abs(v - x64) <= bound).all()
    late = np.roll(v, 1, axis=0)  # row t of the output holds t - 1
    assert (np.abs(late - x64) > bound).mean() > 0.9


@pytest.mark.parametrize("bf16", TYPES)
def test_gelu_membership_on_the_emulation(bf16):
    """The set-membership check accepts gelu_ggml of an f32 chain and rejects a
    neighbouring table entry."""
    tab = er.host_gelu_table()
    a, w, _, _ = er.gemm_inputs(2, 32, 64, 128)
    bias = np.linspace(-14, 14, 64).astype(np.float32)
    ref, beta = er.gemm_acc_ref(a, w, bf16)
    x64, bx = er.add_bound(ref, beta, bias.astype(np.float64)[None])
    x32 = er.gemm_emulate(a, w, bf16) + bias[None]
    finish = lambda g, sel=None: er.round_t(g, bf16)
    out = finish(er.gelu_emulate(x32, tab))
    assert er.gelu_candidates_ok(out, x64, bx, tab, finish).all()
    mid = (np.abs(x64) > 0.5) & (np.abs(x64) < 8)
    off = finish(er.gelu_emulate(x32 * np.float32(1.01), tab))
    assert (~er.gelu_candidates_ok(off, x64, bx, tab, finish))[mid].mean() > 0.5
    # EPI_CONV2: the stored value is f32(pe + g)
    pe = er.gemm_inputs(2, 32, 64, 128)[3]
    with_pe = lambda g, sel: pe.reshape(-1)[sel] + g
    assert er.gelu_candidates_ok(pe + er.gelu_emulate(x32, tab), x64, bx, tab, with_pe).all()
    assert not er.gelu_candidates_ok(pe + off, x64, bx, tab, with_pe)[mid].all()
    # the stand-in table (float64 rounded to f32, then to f16: one double
    # rounding at f16 ties) satisfies the table bound with under one ulp
    assert er.gelu_table_admits(tab) < 1.0
    g, bound = er.gelu_table_bound()
    t = tab[:2 * er.GELU_TAB_HALF].view(np.float16).astype(np.float64)
    assert (np.abs(t - g) <= bound).all()
    shifted = np.roll(t[:er.GELU_TAB_HALF], 1)  # every entry one f16 input late
    assert (np.abs(shifted - g[:er.GELU_TAB_HALF]) > bound[:er.GELU_TAB_HALF]).mean() > 0.5


# --------------------------------------------------------------- LayerNorm

@pytest.mark.parametrize("bf16", TYPES)
def test_layer_norm_emulation_within_bound(bf16):
    worst = 0.0
    for N in er.LN_NS:
        for seed in (0, 1, 2):
            c = er.ln_case(N, seed)
            y64, bound = er.ln_ref(c["x"], c["w"], c["b"], bf16)
            assert np.isfinite(y64).all() and np.isfinite(bound).all()
            y = er.ln_emulate(c["x"], c["w"], c["b"], bf16)
            worst = max(worst, er.worst_ratio(y, y64, bound))
            const = np.arange(er.LN_M) % 4 == 2
            assert np.array_equal(y[const], np.broadcast_to(er.round_t(c["b"], bf16), y.shape)[const])
    assert worst <= 1.0
    print(f"LayerNorm emulation: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("bf16,Ns", [(False, (64, 384, 512)), (True, (64,))])
def test_layer_norm_variance_over_n_minus_1_shows(bf16, Ns):
    """(1 / (2 N) of the normalised value against the output's half-ulp: the
    small N of the GPU shapes see it, in f16 up to 512.)"""
    for N in Ns:
        c = er.ln_case(N)
        y64, bound = er.ln_ref(c["x"], c["w"], c["b"], bf16)
        bad = er.ln_emulate(c["x"], c["w"], c["b"], bf16, ddof=1)
        assert er.worst_ratio(bad, y64, bound) > 1.0, N


def test_layer_norm_shapes_cover_the_paths():
    assert sorted({(N + 255) // 256 for N in er.LN_NS}) == [1, 2, 3, 4, 5, 8]  # NPT instantiations
    assert any(N % 256 for N in er.LN_NS) and any(N % 256 == 0 for N in er.LN_NS)
    assert all(N % 32 == 0 and N <= 2048 for N in er.LN_NS)
    act = er.ln_case(64)["active"]
    assert 0 < act.sum() < er.LN_M and {r % 4 for r in np.flatnonzero(act == 0)} == {0, 1, 2, 3}


def test_slab_fold_is_in_ks_order():
    x = er.ln_case(64)["x"][:4]
    P, pb = er.ln_slabs(x, 5)
    assert not np.array_equal(er.ln_fold(x, P, pb), er.ln_fold(x, P[::-1], pb))
