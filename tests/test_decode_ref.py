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
