"""The DTW token-timestamp restatement (tests/dtw_ref.py) against HF
transformers' _dynamic_time_warping / _median_filter, and against planted
alignments. CPU only."""
import numpy as np
import pytest

import dtw_ref as R


@pytest.fixture(scope="module")
def hf():
    import torch
    from transformers.models.whisper import generation_whisper as g

    return torch, g


DP_SHAPES = [(1, 1), (1, 9), (7, 1), (9, 5), (20, 150), (64, 257)]


@pytest.mark.parametrize("kind", ["int", "f32"])
@pytest.mark.parametrize("shape", DP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_f32_dp_equals_hf(hf, kind, shape):
    _, g = hf
    m = R.path_cost(kind, 11, *shape)
    ti, tj = R.dtw(m, np.float32)
    hi, hj = g._dynamic_time_warping(m)          # f32 in: HF's f32 table, f32 sums
    assert np.array_equal(ti, hi) and np.array_equal(tj, hj)
    # the integer matrices are exact in any precision: f64 walks the same path
    if kind == "int":
        di, dj = R.dtw(m, np.float64)
        assert np.array_equal(di, hi) and np.array_equal(dj, hj)


def test_tie_rule_is_exercised():
    """The integer matrices reach every branch: diagonal, up, left, and ties
    between each pair (the tie goes to the later candidate, finally left)."""
    m = R.path_cost("int", 11, 20, 150)
    ti, tj = R.dtw(m)
    steps = set(zip(np.diff(ti).tolist(), np.diff(tj).tolist()))
    assert steps == {(1, 1), (1, 0), (0, 1)}
    flat = np.zeros((4, 6), np.float32)          # all ties: left along the last row, then up
    ti, tj = R.dtw(flat)
    assert ti.tolist() == [0, 1, 2, 3, 3, 3, 3, 3, 3] and tj.tolist() == [0, 0, 0, 0, 1, 2, 3, 4, 5]
    assert R.frames_of_path(ti, tj, 4).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("A,N,T", [(1, 2, 1), (3, 9, 3), (3, 9, 4), (2, 24, 7), (3, 24, 300)])
def test_cost_stage_equals_hf(hf, A, N, T):
    torch, g = hf
    w = R.random_probs(5, A, N, T + 16)[..., :T].astype(np.float64)   # (cut to T, as step 2)
    wt = torch.tensor(w)[None]                                   # [batch][heads][N][T]
    std, mean = torch.std_mean(wt, dim=-2, keepdim=True, unbiased=False)
    ht = g._median_filter((wt - mean) / std, R.MEDIAN_WIDTH).mean(dim=1)
    want = -ht[0].numpy()
    got = R.cost_matrix(w, np.float64)
    assert got.shape == (N, T)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-11 * max(1.0, np.abs(want).max()))


def test_median_selects_an_element():
    z = np.random.default_rng(3).standard_normal((2, 5, 40))
    med = R.median_filter(z)
    win = z[..., R.reflect_index(40)]
    assert np.all((win == med[..., None]).any(axis=-1))
    assert R.median_filter(z[..., :3]) is not None and np.array_equal(R.median_filter(z[..., :3]),
                                                                      z[..., :3])


def test_constant_column_is_zero():
    w = R.random_probs(9, 2, 6, 12)
    w[:, :, 5] = np.float32(2.0 ** -10)
    for dt in (np.float64, np.float32):
        z, _, std = R.normalise(w, dt)
        assert np.all(std[:, 5] == 0) and np.all(z[:, :, 5] == 0) and np.all(np.isfinite(z))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_staircase_is_recovered(dtype):
    A, N, T = 3, 24, 300
    w, edge = R.planted_probs(21, A, N, T)
    fr = R.frames(R.cost_matrix(w, dtype), dtype)
    assert fr.shape == (N,)
    assert np.all(np.abs(fr - edge[:N]) <= 1), (fr, edge[:N])
    assert np.all(np.diff(fr) >= 0)


def test_f32_cost_within_its_bound():
    """The f32 restatement (the kernel's summation order) obeys the bound the
    GPU test holds the kernel to."""
    for w in (R.random_probs(2, 3, 24, 64), R.planted_probs(2, 3, 24, 64)[0]):
        c64, bound = R.cost_bound(w)
        c32 = R.cost_matrix(w, np.float32)
        assert np.all(np.abs(c32 - c64) <= bound)
        assert bound.max() < 1e-3


def test_token_times_and_columns():
    assert R.n_columns(1500, 3000) == 1500 and R.n_columns(1500, 4000) == 1500
    assert R.n_columns(1500, 999) == 500 and R.n_columns(1500, 1) == 1
    w, edge = R.planted_probs(4, 2, 10, 50)
    t = R.token_times(R.cost_matrix(w, np.float32), 3000)
    assert t.shape == (8,) and np.all(np.abs(t - (3000 + 2 * edge[1:9])) <= 2)


def test_parameter_validation():
    L, H = 2, 2
    assert R.validate_heads("n_top_most", 1, None, L, H) == [(1, 0), (1, 1)]
    assert R.validate_heads("n_top_most", 2, None, L, H) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert R.validate_heads("n_top_most", 0, None, L, H) is None
    assert R.validate_heads("n_top_most", 3, None, L, H) is None
    assert R.validate_heads("custom", -1, [(0, 1), (1, 0), (1, 1)], L, H) == [(0, 1), (1, 0), (1, 1)]
    assert R.validate_heads("custom", -1, [], L, H) is None
    assert R.validate_heads("custom", -1, [(2, 0)], L, H) is None
    assert R.validate_heads("custom", -1, [(0, 2)], L, H) is None
    assert R.validate_heads("custom", -1, [(0, -1)], L, H) is None
    assert R.validate_heads("model", -1, [(1, 1)], L, H, preset_geometry=(6, 8)) is None
    assert R.validate_heads("model", -1, [(1, 1)], L, H, preset_geometry=(2, 2)) == [(1, 1)]
    assert R.validate_heads("none", -1, None, L, H) is None


def test_mx_widening_reference():
    codes = np.array([[0x38] * 32 + [0xB9] * 32], np.uint8)     # 1.0 and -1.125
    h = R.mx_widen(codes, np.array([[127, 126]], np.uint8))
    assert h[0, 0] == np.float16(1.0) and h[0, 63] == np.float16(-0.5625)
