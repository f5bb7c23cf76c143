"""The constraint tables (csrc/constraint.cpp) on the CPU,
through the context-free hook mwx_test_constraint_walk and the public host-only
queries, against tests/constraint_ref.py: choices against brute force over the
expanded strings, random DFAs' class-compressed walk against the raw table,
each refusal of mwx_constraint_from_dfa once, and the 4095-state limit hit
exactly and exceeded by one."""
import numpy as np
import pytest

import constraint_ref as cr
import mwx

CHOICES = ["yes", "no", "repeat", "Yes please", "twenty-five", "no.", " x"]
ALL = cr.FOLD_CASE | cr.LEADING_SPACE | cr.TRAILING_PUNCT


def probes(strings, rng, n):
    """Byte strings drawn from the accepted strings, their prefixes, their
    one-byte mutations and noise."""
    pool = sorted(strings)
    out = [b"", b" ", b".", b"  "]
    while len(out) < n:
        s = pool[int(rng.integers(len(pool)))]
        k = int(rng.integers(4))
        if k == 0:
            out.append(s)
        elif k == 1:
            out.append(s[:int(rng.integers(len(s) + 1))])
        elif k == 2:
            b = bytearray(s + b"?")
            b[int(rng.integers(len(b)))] = int(rng.integers(256))
            out.append(bytes(b[:int(rng.integers(1, len(b) + 1))]))
        else:
            out.append(bytes(rng.integers(0, 256, int(rng.integers(1, 6)), dtype=np.uint8)))
    return out


@pytest.mark.parametrize("flags", [0, cr.FOLD_CASE, cr.LEADING_SPACE, cr.TRAILING_PUNCT, ALL])
def test_choices_against_brute_force(flags):
    ref = cr.Choices(CHOICES, flags)
    con = mwx.Constraint.from_choices(CHOICES, flags)
    rng = np.random.default_rng(flags)
    n_viable = n_acc = 0
    for i, data in enumerate(probes(ref.strings, rng, 300)):
        s = con.walk(data)
        assert (s != 0) == ref.viable(data), data
        assert con.accepting(s) == ref.accepted(data), data
        n_viable += s != 0
        n_acc += ref.accepted(data)
        if i % 10 == 0:  # the same through the hook, which builds its own
            hs, hacc, ns, nc, nb = mwx.constraint_walk_hook(data, texts=CHOICES, flags=flags)
            assert (hs, bool(hacc), ns) == (s, con.accepting(s), con.n_states), data
            assert 1 <= nc <= 256 and nb == ns * nc * 2 + 256 + ns
    for data in probes(ref.strings, rng, 100):  # (member: expand without the set)
        assert cr.member(CHOICES, flags, data) == ref.accepted(data), data
    assert n_viable > 50 and n_acc > 20 and n_viable < 290  # (both outcomes are exercised)
    assert not con.accepting(0) and con.walk(b"yes", 0) == 0 and con.start >= 1


def random_dfa(rng, S, n_bytes):
    """Every state 1 .. S-1 accepting with probability 1/3 and state S-1
    always (and reachable from all), transitions on n_bytes distinct bytes."""
    trans = np.zeros((S, 256), np.uint16)
    used = rng.choice(256, n_bytes, replace=False)
    for s in range(1, S):
        trans[s, used] = rng.integers(0, S, n_bytes)
        trans[s, used[0]] = S - 1  # every live state reaches the accepting S-1
    acc = (rng.integers(0, 3, S) == 0).astype(np.uint8)
    acc[0], acc[S - 1] = 0, 1
    return trans, acc, used


@pytest.mark.parametrize("S,n_bytes", [(2, 1), (5, 3), (64, 17), (300, 256), (4096, 40)])
def test_compressed_walk_equals_raw(S, n_bytes):
    rng = np.random.default_rng(S)
    trans, acc, used = random_dfa(rng, S, n_bytes)
    start = int(rng.integers(1, S))
    ref = cr.Dfa(trans, acc, start)
    con = mwx.Constraint.from_dfa(trans, acc, start)
    assert con.n_states == S and con.start == start
    for s in range(0, S, max(1, S // 97)):
        assert con.accepting(s) == bool(acc[s])
    for b in range(256):  # every single byte from a few states: the class map
        for s in (start, S - 1, S // 2):
            assert con.walk(bytes([b]), s) == int(trans[s, b]), (s, b)
    for _ in range(200):
        n = int(rng.integers(0, 12))
        data = bytes(rng.choice(used if rng.integers(4) else np.arange(256), n).astype(np.uint8))
        s0 = int(rng.integers(0, S))
        assert con.walk(data, s0) == ref.next(s0, data), (s0, data)
    hs, hacc, ns, nc, nb = mwx.constraint_walk_hook(bytes(used[:3].astype(np.uint8)), trans=trans,
                                                    accepting=acc, start=start)
    want = ref.next(start, bytes(used[:3].astype(np.uint8)))
    assert (hs, bool(hacc), ns) == (want, bool(acc[want]), S)
    assert nc <= n_bytes + 1


def test_from_dfa_refusals():
    trans, acc, start = cr.accept_all_dfa()
    assert mwx.Constraint.from_dfa(trans, acc, start).n_states == 2

    def refused(t=trans, a=acc, s=start, n=None):
        with pytest.raises(ValueError):
            mwx.Constraint.from_dfa(t, a, s, n)
        return True

    assert refused(n=1)                                    # a size out of range
    big = np.zeros((cr.MAX_STATES + 1, 256), np.uint16)
    assert refused(t=big, a=np.ones(cr.MAX_STATES + 1, np.uint8))
    t = trans.copy(); t[1, 7] = 2
    assert refused(t=t)                                    # a target >= n_states
    t = trans.copy(); t[0, 9] = 1
    assert refused(t=t)                                    # state 0 not dead: an edge
    assert refused(a=np.array([1, 1], np.uint8))           # state 0 not dead: accepting
    assert refused(s=0) and refused(s=2) and refused(s=-1)  # start < 1 (or past the end)
    # a reachable state that cannot reach an accepting one: 1 -a-> 2, 2 loops
    t = np.zeros((3, 256), np.uint16)
    t[1, ord("a")] = 2
    t[2, :] = 2
    assert refused(t=t, a=np.array([0, 1, 0], np.uint8), s=1)
    # ... the same trap, unreachable, is accepted
    t2 = t.copy(); t2[1, ord("a")] = 1
    assert mwx.Constraint.from_dfa(t2, np.array([0, 1, 0], np.uint8), 1).n_states == 3
    assert mwx.constraint_walk_hook(b"a", trans=t, accepting=np.array([0, 1, 0], np.uint8),
                                    start=1)[0] == -1


def test_from_choices_refusals_and_state_limit():
    for bad in ([], [""], ["ok", ""]):
        with pytest.raises(ValueError):
            mwx.Constraint.from_choices(bad, 0)
    with pytest.raises(ValueError):
        mwx.Constraint.from_choices(["ok"], 8)
    # without flags a text of n bytes has n + 1 live states (the start and one per byte)
    con = mwx.Constraint.from_choices(["a" * 4094], 0)
    assert con.n_states == 4096  # 4095 live + the dead state
    s = con.walk(b"a" * 4094)
    assert s != 0 and con.accepting(s) and con.walk(b"a", s) == 0
    with pytest.raises(ValueError):
        mwx.Constraint.from_choices(["a" * 4095], 0)
    assert mwx.constraint_walk_hook(b"a", texts=["a" * 4095])[0] == -1
    # two texts sharing no prefix: 1 + 2047 + 2047 = 4095 live; one more byte is too many
    assert mwx.Constraint.from_choices(["a" * 2047, "b" * 2047], 0).n_states == 4096
    with pytest.raises(ValueError):
        mwx.Constraint.from_choices(["a" * 2047, "b" * 2048], 0)


def test_default_params_have_the_constraint_off():
    p = mwx.Context.default_params(mwx.SAMPLING_GREEDY)
    assert not p.constraint and p.constraint_penalty == 100.0
    p = mwx.Context.default_params(mwx.SAMPLING_BEAM_SEARCH)
    assert not p.constraint and p.constraint_penalty == 100.0


def test_mask_words_round_trip():
    rng = np.random.default_rng(3)
    for V in (1, 63, 64, 65, 257, 51865):
        rej = rng.integers(0, 2, V).astype(bool)
        w = cr.mask_words(rej)
        assert w.shape == ((V + 63) // 64,) and np.array_equal(cr.unpack(w, V), rej)
        if V % 64:
            assert int(w[-1]) >> (V % 64) == 0
