"""logits_bias_kernel (k_bias.hip) and the __device__ matcher transition
through mwx_test_logits_bias, against numpy float32 x + bias of the naive rule
in tests/bias_ref.py, bit for bit over the whole [R][V] array (so every entry
no match points at, and every row with active = 0 or sample = 0, must keep
its bits). V in {257, 51866}, R in {1, 5, 33}; rows in equal and in different
states; boosted ids 0 and V - 1; states whose own edge list has 0, 1, 63, 64,
65 and 257 entries (around the wave and above the 256-thread workgroup);
failure chains of the full depth; negative and zero boosts; -inf logits; the
root list of 1024 distinct first tokens; state_out against the host walk."""
import numpy as np
import pytest

import bias_ref
import mwx

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)
HEAD = {n: 10 + i for i, n in enumerate(SIZES)}  # first id of the phrases of size n
LEAF = 20  # a one-token phrase: its state has no edge of its own
RUN = 30   # [RUN] * 16: after 15 of them the failure chain has every depth


@pytest.fixture(scope="module")
def ctx(make_model):
    c = mwx.Context.open(make_model("micro"))
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def phrase_set(V):
    rng = np.random.default_rng(V)
    ph = [([LEAF], 0.75), ([RUN] * 16, 2.0), ([RUN, RUN, V - 1], -1.5), ([RUN, 0], 0.0)]
    for n in SIZES:
        # second ids 0 .. n-1 (n = 257: every id of the small vocabulary, 0 and
        # V - 1 among them); they overlap the first ids, so the state's list and
        # the root's are max-combined
        for j in range(n):
            t = j if n <= V else j % V
            ph.append(([HEAD[n], t], float(np.float32(rng.choice([-2.0, 0.5, 1.25, 3.0])))))
    ph.append(([V - 1, 0], 1.5))
    ph.append(([0, V - 1], -0.25))
    for _ in range(40):  # a small alphabet: overlaps, failure links between phrases
        ln = int(rng.integers(1, 9))
        ph.append(([int(t) for t in rng.integers(100, 103, ln)],
                   float(np.float32(rng.choice([-3.0, 0.0, 0.25, 1.0, 7.0])))))
    assert len(ph) <= bias_ref.MAX_PHRASES
    return ph


def histories(V):
    rng = np.random.default_rng(V + 1)
    hs = [[], [LEAF], [RUN] * 15, [RUN] * 40, [RUN, RUN], [5, 6, 7], [V - 1], [0], [LEAF, 0]]
    hs += [[HEAD[n]] for n in SIZES]
    hs += [[3, HEAD[257]], [HEAD[64], HEAD[65]]]
    hs += [[int(t) for t in rng.integers(100, 103, int(rng.integers(1, 30)))] for _ in range(12)]
    return hs


def expected(phrases, x, hist, active, sample):
    want = x.copy()
    for r, h in enumerate(hist):
        if active[r] and sample[r]:
            want[r] = bias_ref.apply(phrases, h, x[r])
    return want


@pytest.fixture(scope="module")
def data():
    out = {}
    for V in (257, 51866):
        ph = phrase_set(V)
        hs = histories(V)
        rng = np.random.default_rng(V + 2)
        x = (rng.standard_normal((33, V)) * 4).astype(np.float32)
        x[:, 0::7] = -np.inf          # -inf at many boosted ids (0 among them)
        x[1::2, V - 1] = -np.inf
        x[:, 3] = np.float32(-0.0)
        out[V] = (ph, hs, x)
    return out


@pytest.mark.parametrize("V", [257, 51866])
@pytest.mark.parametrize("R", [1, 5, 33])
def test_kernel_matches_reference(ctx, data, V, R):
    ph, hs, x = data[V]
    passes = (len(hs) + R - 1) // R
    seen_sizes = set()
    for k in range(passes):  # every history appears in some row of some launch
        hist = [hs[(k * R + r) % len(hs)] for r in range(R)]
        if R == 33:
            hist[31] = hist[0]  # rows in the same state
            hist[32] = hist[0]
        active = np.ones(R, np.int32)
        sample = np.ones(R, np.int32)
        if R > 1:
            active[1::4] = 0
            sample[3::4] = 0
            if k % 2:  # the rows left out move, so each history also runs live
                active[:] = 1
                sample[:] = 1
                active[2::4] = 0
                sample[0::4] = 0
        got, state = ctx.test_logits_bias(ph, x[:R], hist, active, sample)
        want = expected(ph, x[:R], hist, active, sample)
        assert (bits(got) == bits(want)).all(), (V, R, k, np.argwhere(bits(got) != bits(want))[:8])
        assert np.isneginf(got[np.isneginf(x[:R])]).all()
        for r in range(R):
            assert state[r] == mwx.bias_state(ph, hist[r]), (V, R, k, r)
            seen_sizes.add(len(bias_ref.bias_set(ph, hist[r])))
        if R == 33:
            assert state[31] == state[0] == state[32]
    assert len(seen_sizes) >= 5  # (root, +1, +63, +64, +65 / everything)


def test_own_edge_lists_have_the_sizes(data):
    """The cases above hold what the docstring says: the state after [HEAD[n]]
    adds n tokens of its own to the root's list (checked on the naive rule)."""
    for V in (257, 51866):
        ph, _, _ = data[V]
        root = bias_ref.bias_set(ph, [])
        assert 0 in root and V - 1 in root
        assert bias_ref.bias_set(ph, [LEAF]) == root  # 0 entries of its own
        for n in SIZES:
            own = {t for ids, _ in ph if len(ids) == 2 and ids[0] == HEAD[n] for t in [ids[1]]}
            assert len(own) == min(n, V), (V, n)
            assert set(bias_ref.bias_set(ph, [HEAD[n]])) == set(root) | own
        assert len(bias_ref.bias_set(ph, [HEAD[257]])) == 257 if V == 257 else True


def test_root_list_of_1024_first_tokens(ctx):
    V, R = 51866, 5
    rng = np.random.default_rng(11)
    first = rng.permutation(V)[:1024]
    first[0], first[1] = 0, V - 1
    ph = [([int(t), int(first[(i + 1) % 1024])], float(np.float32(0.5 + (i % 9) * 0.25)))
          for i, t in enumerate(first)]
    x = (rng.standard_normal((R, V)) * 3).astype(np.float32)
    hist = [[], [int(first[7])], [int(first[7]), int(first[8])], [V - 1], [1, 2, 3]]
    ones = np.ones(R, np.int32)
    got, state = ctx.test_logits_bias(ph, x, hist, ones, ones)
    want = expected(ph, x, hist, ones, ones)
    assert (bits(got) == bits(want)).all()
    assert int((bits(got[0]) != bits(x[0])).sum()) == 1024
    assert [int(s) for s in state] == [mwx.bias_state(ph, h) for h in hist]
    assert state[0] == 0 and state[4] == 0 and state[1] != 0


def test_refusals_launch_nothing(ctx):
    x = np.zeros((2, 64), np.float32)
    one = np.ones(2, np.int32)
    ok = [([1, 2], 1.0)]
    for ph in ([([1, 64], 1.0)], [([1] * 17, 1.0)], [([1], float("nan"))], [([-1], 1.0)], []):
        rc, out, state = ctx.test_logits_bias_rc(ph, x, [[], []], one, one)
        assert rc == -1, ph
        assert np.isnan(out).all() and (state == -1).all()
    rc, out, state = ctx.test_logits_bias_rc(ok, x, [[1], []], one, one)
    assert rc == 0 and out[0, 2] == 1.0 and out[0, 1] == 1.0 and out[1, 2] == 0.0
