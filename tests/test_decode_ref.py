"""CPU checks of tests/decode_ref.py: the f32 / f16 emulation of the decode
kernels' roundings must stay inside the derived bounds on the very inputs the
GPU tests run (test_gpu_decode_kernels.py), so a device ratio above 1 there
points at the kernel and not at the derivation."""
import numpy as np
import pytest

import decode_ref as dr


def _ratios(rows, scale, bf16):
    worst = 0.0
    for q, K, V, *_ in rows:
        o64, bound = dr.attention_ref(q, K, V, scale, bf16)
        worst = max(worst, dr.worst_ratio(dr.attention_emulate(q, K, V, scale, bf16), o64, bound))
    return worst


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("qs", [0.02, 3.0])
def test_emulation_within_bound_self_inputs(bf16, qs):
    worst = 0.0
    for KS in (1, 2, 5, 8):
        case = dr.self_case(0, qs, KS)
        worst = max(worst, _ratios(dr.self_rows(case), case["scale"], bf16))
    print(f"self, qs {qs}, {'bf16' if bf16 else 'f16'}: worst emulation ratio {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("bf16", [False, True])
def test_emulation_within_bound_cross_inputs(bf16):
    worst = 0.0
    for i, n in enumerate(dr.CROSS_LENS):
        case = dr.cross_case(0, n, 3, 2, 1 + i % 8, 3)
        worst = max(worst, _ratios(dr.cross_rows(case), case["scale"], bf16))
    print(f"cross, {'bf16' if bf16 else 'f16'}: worst emulation ratio {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("bf16", [False, True])
def test_emulation_within_bound_seed_sweep(bf16):
    """Lengths 1 .. 1536, query scales 0.02 / 0.5 / 3.0 (one per row), 5 seeds."""
    worst = 0.0
    for seed in range(1, 6):
        for n in (1, 2, 9, 17, 129, 257, 448, 777, 1500, 1536):
            case = dr.cross_case(seed, n, 3, 1, 1, 3)
            worst = max(worst, _ratios(dr.cross_rows(case), case["scale"], bf16))
    print(f"sweep, {'bf16' if bf16 else 'f16'}: worst emulation ratio {worst:.3f}")
    assert worst <= 1.0


def test_reference_notices_a_dropped_key_and_a_swapped_pair():
    """The bound is tight enough to tell a kernel that drops the last key, or
    that swaps the weights of keys j and j + 8, from a correct one."""
    case = dr.cross_case(0, 257, 3, 2, 1, 3)
    # the diffuse row (every key weighs about 1 / n) shows a dropped key ...
    q, K, V = dr.cross_rows(case)[0]
    o64, bound = dr.attention_ref(q, K, V, case["scale"], False)
    assert dr.worst_ratio(dr.attention_emulate(q, K[:-1], V[:-1], case["scale"], False),
                          o64, bound) > 1.0
    # ... and the peaked row (unequal weights) swapped ones
    q, K, V = dr.cross_rows(case)[1]
    o64, bound = dr.attention_ref(q, K, V, case["scale"], False)
    perm = np.arange(257)
    perm[0:8], perm[8:16] = np.arange(8, 16), np.arange(0, 8)
    assert dr.worst_ratio(dr.attention_emulate(q, K, V[perm], case["scale"], False),
                          o64, bound) > 1.0


def test_slab_sum_order_and_roundings():
    """slab_sum adds in ks order in f32; q / k / v round once to f16."""
    P = np.asarray([[[1.0]], [[2.0 ** -24]], [[2.0 ** -24]]], np.float32)
    assert dr.slab_sum(P)[0, 0] == np.float32(1.0)          # (1 + e) + e, not 1 + 2e
    assert dr.slab_sum(P[::-1])[0, 0] == np.float32(1.0 + 2.0 ** -23)
    x = np.asarray([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11], np.float32)
    want = np.asarray([1.0, 1.0 + 2.0 ** -6, 1.0], np.float32)  # ties to even, both ways
    assert np.array_equal(dr.bf16_round(x), want)
    assert np.array_equal(dr.round_t(x, False),
                          np.asarray([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0], np.float32))


@pytest.mark.parametrize("bf16", [False, True])
def test_gemm_emulation_within_bound(bf16):
    worst = 0.0
    for K in (96, 128, 1280, 5120):
        a, w = dr.gemm_inputs(0, 5, 26, K)
        ref, bound = dr.gemm_ref(a, w, bf16)
        worst = max(worst, dr.worst_ratio(dr.gemm_emulate(a, w, bf16), ref, bound))
        # a dropped 32-deep k-step is far outside
        ref2, _ = dr.gemm_ref(a, w, bf16, 0, K - 32)
        assert np.max(np.abs(ref2 - ref) / bound) > 10.0
    print(f"gemm, {'bf16' if bf16 else 'f16'}: worst emulation ratio {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------- the rest of the GEMM family

FULL_KS = (96, 384, 768, 1280, 1536, 2048, 3072, 4096, 5120)  # test_gemm_decode_full_k
MODEL_WIDTHS = (384, 512, 768, 1024, 1280)


def test_k_split_rules_restate_the_launchers():
    """splitk_factor / skinny_split as the GPU tests restate them: the
    factors the existing split-K test records, every k-steps-per-wave case of
    the full-K set, and every model width served by both LayerNorm folds."""
    assert {K: dr.splitk_factor(K) for K in dr.SPLITK_KS} == dr.SPLITK_KS
    assert [dr.splitk_factor(K) for K in (96, 160, 6144 + 128)] == [0, 0, 0]
    assert sorted({dr.skinny_split(K)[1] for K in FULL_KS}) == [1, 2, 3, 4, 6, 8, 10]
    assert dr.skinny_split(48) is None and dr.skinny_split(32 * 17) is None
    for K in MODEL_WIDTHS + (2048,):
        assert dr.ln_fold_serves(K, 0) and dr.ln_fold_serves(K, 3), K
    assert not dr.ln_fold_serves(96, 0) and not dr.ln_fold_serves(96, 3)   # K % 128; 3 waves
    assert not dr.ln_fold_serves(2048 + 128, 0) and not dr.ln_fold_serves(4096, 3)


def test_probe_weights_cover_every_code_and_exponent():
    for K, nexp in ((128, 104), (512, 201)):
        codes, scales = dr.mx_probe_weights(0, 26, K)
        assert set(codes.reshape(-1)) == set(dr.FINITE_CODES) and len(dr.FINITE_CODES) == 254
        e = scales.astype(np.int64) - 127
        assert e.min() == -100 and e.max() == 100 and len(set(e.reshape(-1))) == nexp
        w = dr.mx_decode(codes, scales)
        # every value a normal bf16 (or zero): the probe's products are exact
        assert np.array_equal(dr.bf16_round(w), w)
        assert (np.abs(w[w != 0]) >= 2.0 ** -126).all() and np.isfinite(w).all()


@pytest.mark.parametrize("K", [128, 1280])
def test_w8_emulation_within_bound_and_broken_variants_rejected(K):
    """The W8 path (codes widened exactly, then the bf16 chain) holds gemm_ref's
    bound on the dequantised weights; a scale from the next k-step, from the
    neighbouring column or shared by 64 k, a lane's codes reversed and its
    first word's halves swapped each exceed it, and each fails the identity
    probe (A = I: the output is the widened weight itself)."""
    M, N = 5, 26
    codes, scales = dr.mx_dec_weights(0, N, K)
    e = scales.astype(np.int64) - 127
    assert e.min() == -30 and e.max() == 8
    a, _ = dr.gemm_inputs(0, M, N, K)
    ref, bound = dr.gemm_ref(a, dr.mx_decode(codes, scales), True)
    good = dr.worst_ratio(dr.w8_emulate(a, codes, scales), ref, bound)
    print(f"W8 K {K}: worst emulation ratio {good:.3f}")
    assert good <= 1.0
    pc, ps = dr.mx_probe_weights(0, N, min(K, 512))
    want = dr.mx_decode(pc, ps)
    assert np.array_equal(dr.w8_widen(pc, ps).view(np.uint32), want.view(np.uint32))
    for broken in dr.W8_BROKEN:
        r = dr.worst_ratio(dr.w8_emulate(a, codes, scales, broken=broken), ref, bound)
        wrong = (dr.w8_widen(pc, ps, broken).view(np.uint32) != want.view(np.uint32)).mean()
        print(f"W8 K {K} {broken}: ratio {r:.3g}, probe words wrong {wrong:.3f}")
        assert r > 1.0 and wrong > 0.25, broken


@pytest.mark.parametrize("N", [64, 96, 160])
@pytest.mark.parametrize("M", [1, 5, 17, 64, 65, 100])
def test_packed_store_check_rejects_broken_stores(M, N):
    """The packed-store check (rows < M written, pad rows untouched, the
    values at pack_index(m, n, N)) passes the store it restates and fails a
    transposed index and, above 64 rows, a store that drops rows >= 64."""
    vals = (np.arange(M * N, dtype=np.uint32) % 0xF000).astype(np.uint16).reshape(M, N)
    ok, rows = dr.packed_store_ok(dr.pack_store(vals), M, N)
    assert ok and np.array_equal(rows, vals)
    ok, rows = dr.packed_store_ok(dr.pack_store(vals, "transposed"), M, N)
    assert not (ok and np.array_equal(rows, vals))
    ok, rows = dr.packed_store_ok(dr.pack_store(vals, "drop64"), M, N)
    assert (ok and np.array_equal(rows, vals)) == (M <= 64)
