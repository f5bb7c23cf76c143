"""logits_constrain_kernel (k_constrain.hip) through mwx_test_constraint_mask
against tests/constraint_ref.py, every 64-bit word bit for bit, and the filter's
mask / penalty arguments through mwx_test_logits_process_masked against the
float64 restatement there (logits_ref.py's reference and bounds on the
penalised logits).

Mask: R in {1, 5, 33}; V = 257 with a supplied token table (single bytes, an
empty token, tokens of 5 to 40 bytes: longer than the 4-byte head) and V =
51865, the multilingual vocabulary whose last text token is empty; neither is a
multiple of 64. States: the start, mid-word, accepting without an outgoing edge
(every text token rejected, EOT not), non-accepting (EOT rejected), dead (all
zero); a choice set (brute force over strings) and a cyclic DFA (raw table).
Rows with active = 0 or sample = 0 keep their sentinel words."""
import numpy as np
import pytest

import constraint_ref as cr
import logits_ref as lr
import mwx
from test_gpu_logits_kernels import lc_struct, rows_of

pytestmark = pytest.mark.gpu

ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
FLAGS = cr.LEADING_SPACE | cr.TRAILING_PUNCT


@pytest.fixture(scope="module")
def ctx(make_model):
    with mwx.Context.open(make_model("micro-ml")) as c:
        yield c


def small_vocab():
    """256 text tokens for V = 257 (eot = 256): the bytes 0 .. 199 as single-byte
    tokens, then words: an empty token, and tokens of 2 to 40 bytes."""
    toks = [bytes([b]) for b in range(200)]
    words = [b"", b"ye", b"yes", b"yes.", b" yes", b" yes please", b"please", b"yes please?",
             b"no", b"nope", b" n", b"o!", b"repeat", b"repeat after me, slowly and clearly.",
             b"repe", b"at", b"tick", b"tock", b"ticktock", b"tickt", b"ockti", b"ticktockticktock",
             b"k", b"kt", b" ", b"  ", b".", b"?!"]
    toks += words + [bytes([65 + i % 26]) * (2 + i % 7) for i in range(56 - len(words))]
    assert len(toks) == 256 and max(len(t) for t in toks) > 2 * 4
    return toks


@pytest.fixture(scope="module")
def setups(ctx):
    """Per V: (tokens, eot, hook arguments, [(constraint, judge, [(state id,
    judge state)])])."""
    out = {}
    for V in (257, 51865):
        if V == 257:
            toks, kw = small_vocab(), dict(V=257, tokens=small_vocab())
            choices = ["yes please", "no", "repeat after me, slowly and clearly"]
            words = [b"tick", b"tock!"]
        else:
            assert ctx.hparam("n_vocab") == V
            toks, kw = cr.vocab_bytes(ctx), dict()
            assert toks[-1] == b""  # the multilingual vocabulary's empty last text token
            long_ = [t for t in toks[300:] if len(t) >= 6 and t.isalpha()][:40]
            choices = [(long_[0] + long_[1]).decode(), long_[2].decode(), "no"]
            words = [long_[3], long_[4] + b"!"]
        eot = len(toks)
        sets = []
        ch = cr.Choices(choices, FLAGS)
        con = mwx.Constraint.from_choices(choices, FLAGS)
        first = choices[0].encode()
        prefixes = [b"", first[:2], b" " + first[:7], first + b".", first, b"no", None]
        sets.append((con, ch, [(con.walk(p) if p is not None else 0, p) for p in prefixes]))
        assert con.accepting(con.walk(first + b".")) and not con.accepting(con.walk(first[:2]))
        trans, acc, start = cr.cycle_dfa(words)
        dfa = cr.Dfa(trans, acc, start)
        con2 = mwx.Constraint.from_dfa(trans, acc, start)
        ids = [start, dfa.next(start, words[0][:2]), dfa.next(start, words[1][:-1]), 0]
        sets.append((con2, dfa, [(s, s) for s in ids]))
        out[V] = (toks, eot, kw, sets)
    return out


_rej_cache = {}


def rejected(V, k, judge, jstate, toks, eot):
    key = (V, k, jstate)
    if key not in _rej_cache:
        _rej_cache[key] = cr.rejected(judge, jstate, toks, V, eot)
    return _rej_cache[key]


@pytest.mark.parametrize("V", [257, 51865])
@pytest.mark.parametrize("R", [1, 5, 33])
def test_mask_matches_reference(ctx, setups, V, R):
    toks, eot, kw, sets = setups[V]
    W = (V + 63) // 64
    for k, (con, judge, states) in enumerate(sets):
        rows = [states[(r + R) % len(states)] for r in range(R)]
        active = np.ones(R, np.int32)
        sample = np.ones(R, np.int32)
        if R > 1:
            active[1::7] = 0
            sample[3::5] = 0
        rc, mask = ctx.test_constraint_mask_rc(con, [s for s, _ in rows], active, sample, **kw)
        assert rc == 0
        assert mask.shape == (R, W)
        n_set = 0
        for r, (sid, js) in enumerate(rows):
            if not (active[r] and sample[r]):
                assert (mask[r] == ONES).all(), (k, r, "an unwritten row changed")
                continue
            rej = rejected(V, k, judge, js, toks, eot)
            want = cr.mask_words(rej)
            bad = np.nonzero(mask[r] != want)[0]
            assert bad.size == 0, (k, r, sid, int(bad[0]), hex(int(mask[r][bad[0]])),
                                   hex(int(want[bad[0]])))
            n_set += int(rej.sum())
            if sid == 0:
                assert not rej.any()
            else:
                assert rej[eot] == (not con.accepting(sid))
                assert rej[eot - 1] or toks[eot - 1] != b""  # the empty token is rejected
                assert not rej[eot + 1:].any()
        print("V", V, "R", R, "set", k, "rejected bits", n_set)


def test_states_cover_the_cases(setups):
    """What the parametrised test relies on: a state that rejects every text
    token but not EOT, states that reject EOT, tokens past the head that are
    accepted (so bytes beyond the head decide), the tail word's spare bits."""
    for V in (257, 51865):
        toks, eot, kw, sets = setups[V]
        assert V % 64 and eot < V
        con, judge, states = sets[0]
        rejs = [rejected(V, 0, judge, js, toks, eot) for _, js in states]
        assert any(r[:eot].all() and not r[eot] for r in rejs), "accepting, no outgoing edge"
        assert any(r[eot] and not r[:eot].all() for r in rejs), "non-accepting"
        long_ok = [t for r in rejs for t in np.nonzero(~r[:eot])[0] if len(toks[t]) > 4]
        assert long_ok, "no accepted token is longer than the head"
        # a token that agrees with an accepted one on the whole head and differs after it
        con2, dfa, st2 = sets[1]
        r0 = rejected(V, 1, dfa, st2[0][1], toks, eot)
        assert (~r0[:eot]).any() and r0[:eot].any()


def test_refusals_launch_nothing(ctx, setups):
    toks, eot, kw, sets = setups[257]
    con = sets[0][0]
    one = np.ones(1, np.int32)

    def rc_of(c=con, states=(con.start,), active=one, sample=one, **over):
        rc, mask = ctx.test_constraint_mask_rc(c, list(states), active, sample, **{**kw, **over})
        assert (mask == ONES).all()
        return rc

    assert rc_of(c=None) == -1
    assert rc_of(states=(con.n_states,)) == -1 and rc_of(states=(-1,)) == -1
    assert rc_of(V=255) == -1          # eot = 256 > V
    assert rc_of(V=0) == -1 and rc_of(V=lr.MAX_VOCAB + 1) == -1
    n = 257
    assert rc_of(states=[con.start] * n, active=np.ones(n, np.int32),
                 sample=np.ones(n, np.int32)) == -1
    # the context's own vocabulary with another V
    rc, mask = ctx.test_constraint_mask_rc(con, [con.start], one, one, V=51864)
    assert rc == -1 and (mask == ONES).all()


# ---- the filter with a mask and a penalty ---------------------------------------------------
def filter_case(V, lc, seed, penalty):
    rng = np.random.default_rng(seed)
    smask = np.zeros(V, np.float32)
    smask[rng.integers(0, V, V // 50)] = -np.inf
    states = [lr.STATES[0], lr.STATES[1], lr.STATES[2], lr.STATES[5], lr.STATES[4], lr.STATES[7]]
    xs, cs, rejs = [], [], []
    for k, st in enumerate(states):
        c = dict(zip(lr.CTL.names, lr.ctl_row(**st)))
        c["seek_delta"] = 14 if st["has_ts"] else 3000
        c["temperature"] = (0.0, 0.7, 0.0, 0.2)[k % 4]
        c["want_probs"] = int(k % 3 != 2)
        c["want_nosp"] = int(k % 2 == 0)
        if k == 4:
            c["sample"] = 0
        t = c["temperature"] if c["temperature"] > 0 else 1.0
        x = (rng.normal(0.0, 3.0, V) * t).astype(np.float32)
        rej = np.zeros(V, bool)
        rej[:lc.eot] = rng.integers(0, 10, lc.eot) < (9 if k % 2 else 3)
        rej[lc.eot] = bool(k & 1)
        rej[lr.LP_CHUNK - 1:lr.LP_CHUNK + 1] = [True, False]  # either side of a chunk edge
        x[int(rng.integers(0, lc.eot))] += np.float32(6 * t)
        x[int(rng.integers(lc.beg, V))] += np.float32(5 * t)
        # the raw argmax is rejected: the penalty must move the choice
        top = int(np.argmax(np.where(np.arange(V) < lc.eot, x, -np.inf)))
        rej[top] = True
        xs.append(cr.settle(x, smask, c, lc, rej, penalty))
        cs.append(tuple(c[n] for n in lr.CTL.names))
        rejs.append(rej)
    return smask, np.stack(xs), np.array(cs, lr.CTL), np.stack(rejs)


@pytest.mark.parametrize("V,penalty", [(lr.LP_CHUNK + 1, 2.5), (2 * lr.LP_CHUNK + 1, 100.0),
                                       (51865, 2.5), (51865, 100.0)])
def test_filter_with_mask_matches_reference(ctx, V, penalty):
    if V in lr.REAL:  # (beg, eot) of the real vocabulary; " " and nosp where they are there
        lc = lr.LC(V, lr.REAL[V][1], lr.REAL[V][0], 220, 1, -1, lr.REAL[V][1] + 5)
    else:
        lc = lr._layout(V)
    smask, x, ctl, rej = filter_case(V, lc, V + int(penalty), penalty)
    cmask = np.stack([cr.mask_words(r) for r in rej])
    rc, flt, probs, lps, out = ctx.test_logits_process_masked_rc(x, smask, ctl, lc_struct(lc),
                                                                 cmask, penalty)
    assert rc == 0
    flt0, probs0, lps0, out0 = ctx.test_logits_process(x, smask, ctl, lc_struct(lc))
    moved = 0
    for k, got in enumerate(rows_of(flt, probs, lps, out)):
        c = {n: ctl[k][n] for n in lr.CTL.names}
        r = cr.reference(x[k], smask, c, lc, rej[k], penalty)
        ratios = {}
        bad = lr.compare(r, got, ratios)
        print("V", V, "penalty", penalty, "row", k, {n: round(v, 3) for n, v in ratios.items()})
        assert not bad, (k, bad)
        if got is None:
            continue
        # the no-speech probability comes from the raw logits: the same bits
        assert out[k]["nosp"].view(np.uint32) == out0[k]["nosp"].view(np.uint32), k
        # ids that are not rejected keep their bits
        keep = ~rej[k]
        assert np.array_equal(lr.bits(flt[k])[keep], lr.bits(flt0[k])[keep]), k
        moved += int(out[k]["id"] != out0[k]["id"])
    assert moved >= 1, "vacuous: the penalty moved no row's choice"
    # bad penalties launch nothing
    for pen in (0.0, -1.0, float("nan"), float("inf")):
        rc, f, *_ = ctx.test_logits_process_masked_rc(x, smask, ctl, lc_struct(lc), cmask, pen)
        assert rc == -1 and np.isnan(f).all()
