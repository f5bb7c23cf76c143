"""Constrained decoding end to end on the GPU (mwx_full_params.constraint, rule
D15 of DESIGN.md) on the micro-rich geometry: greedy, best-of 3 and beam 5; the
run-ahead path, the host-driven loops and a forced fallback; the batched, pcm16,
trimmed and chunked entry points; bias_phrases together with a constraint; the
refusals; mwx_align_batch untouched.

In run-ahead every step's RowCtl the device wrote (pad[1], the constraint
state, included) is compared with the host's replay, which walks the row's
generated ids from the start state, and a difference redoes the attempt on the
host loop and counts a fallback. A run-ahead call with zero fallbacks therefore
shows that the device state equalled the host walk at every step, after every
beam hand-over too; the tests below assert that count.

test_follow: one (model seed, clip) pair was looked at, the biasing test's
(seed 1, clip 1): 17 steps, none skipped (no top-two gap inside the bound),
every step in a live state."""
import numpy as np
import pytest

import constraint_ref as cr
import logits_ref as lr
import mwx
import vad_restatement as vr
import vad_segments_restatement as sr
from test_gpu_beam_oracle import LOGITS_TOL
from test_gpu_bias import alive_ids, clip, fresh, ids_of, params, records
from test_gpu_vad_segments import SEED, _c_params, two_clip

pytestmark = pytest.mark.gpu

MODEL_SEED = 0
FOLLOW_SEED = 1
FOLLOW_CLIP = 1
ALL = cr.FOLD_CASE | cr.LEADING_SPACE | cr.TRAILING_PUNCT
BIG = 1e4  # the penalty that dominates this model's logits (the biasing tests' boost)


@pytest.fixture(scope="module")
def ctx(make_model):
    with mwx.Context.open(make_model("micro-rich", mwx.GGML_F16, MODEL_SEED)) as c:
        yield c


@pytest.fixture(scope="module")
def clips():
    return [clip(0, 30), clip(1, 12), clip(2, 21)]


def text_of(ctx, state=0):
    eot = ctx.token("eot")
    return b"".join(ctx.token_bytes([t for t in ids_of(ctx, state) if t < eot]))


def five_choices(ctx, p):
    """Five choices made of the text of tokens the static mask leaves alive."""
    ids = alive_ids(ctx, p, 12)
    tb = ctx.token_bytes(ids)
    assert all(t and t.isascii() and b"\0" not in t for t in tb), tb
    ch = [tb[0] + tb[1], tb[2], tb[3] + tb[4] + tb[5], tb[6] + tb[7], tb[8] + tb[9] + tb[10]]
    return [c.decode() for c in ch]


def own_words(ctx, pcm, p, n=2):
    """n words the model itself likes on this clip: the text of the first text
    token of its unconstrained output and of its most frequent other ones, none
    a prefix of another (so a cycle over them is deterministic)."""
    assert ctx.full_batch_states([pcm], p, [0]) == 0
    eot = ctx.token("eot")
    text = [t for t in ids_of(ctx, 0) if 256 <= t < eot]
    assert text
    order = [text[0]] + [t for t, _ in sorted(((t, -text.count(t)) for t in set(text)),
                                              key=lambda x: (x[1], x[0]))]
    words = []
    for t in order:
        w = ctx.token_bytes([t])[0]
        if w and all(not w.startswith(x) and not x.startswith(w) for x in words):
            words.append(w)
        if len(words) == n:
            return words
    raise AssertionError(("fewer distinct words than asked for", words))


def perf_count(ctx, state, cls, fn):
    import ctypes as C
    L = mwx.lib()
    s0 = ctx.state(state)
    L.mwx_perf_read(s0, None, None)
    L.mwx_perf_enable(s0, cls)
    try:
        out = fn()
        ms, n = C.c_double(), C.c_int()
        L.mwx_perf_read_class(s0, cls, C.byref(ms), C.byref(n))
    finally:
        L.mwx_perf_enable(s0, None)
    return out, n.value


# ---- 1. off is off ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "beam", "bestof"])
def test_off_is_off(ctx, clips, mode):
    """constraint = NULL launches no logits_constrain and equals, record for
    record and bit for bit, a call with an accept-everything DFA."""
    p = params(ctx, mode)
    everything = mwx.Constraint.from_dfa(*cr.accept_all_dfa())

    def run(q):
        base = fresh(ctx, 3)  # (the sampling modes draw from the states' RNGs)
        ctx.runahead_fallbacks(base)

        def go():
            assert ctx.full_batch_states(clips, q, range(base, base + 3)) == 0
        _, n = perf_count(ctx, base, b"logits_constrain", go)
        return ([records(ctx, base + i) for i in range(3)], n, ctx.runahead_fallbacks(base),
                [ctx.constraint_status(base + i) for i in range(3)])

    off, n_off, fb_off, st_off = run(p)
    on, n_on, fb_on, st_on = run(mwx.with_constraint(p, everything))
    print(mode, "tokens", [sum(len(s[2]) for s in r) for r in off], "mask launches", n_off, n_on,
          "status", st_off, st_on)
    assert n_off == 0 and n_on > 0
    assert fb_off == 0 and fb_on == 0
    assert sum(len(s[2]) for r in off for s in r) > 20
    assert off == on
    assert st_off == [-1, -1, -1] and st_on == [1, 1, 1]


# ---- 2. a closed set ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "beam", "bestof"])
def test_closed_set(ctx, clips, mode):
    p = params(ctx, mode, no_timestamps=True)
    choices = five_choices(ctx, p)
    con = mwx.Constraint.from_choices(choices, ALL)
    q = mwx.with_constraint(p, con, BIG)
    for k, pcm in enumerate(clips[1:]):  # (under 30 s: one window)
        s = fresh(ctx, 1)
        ctx.runahead_fallbacks(s)
        assert ctx.full_batch_states([pcm], q, [s]) == 0
        ids = ids_of(ctx, s)
        text = text_of(ctx, s)
        print(mode, k, text, ids)
        assert cr.member(choices, ALL, text), (text, choices)
        assert ids[-1] == ctx.token("eot")
        assert ctx.constraint_status(s) == 1
        assert ctx.runahead_fallbacks(s) == 0
    # and without the constraint the text is not one of them (or this shows nothing)
    assert ctx.full_batch_states([clips[1]], p, [0]) == 0
    assert not cr.member(choices, ALL, text_of(ctx, 0)) and ctx.constraint_status(0) == -1


def test_host_choice_match(ctx, clips, tmp_path):
    """RequestOptions::choices through the host SttEngine (the service's decode
    parameters): every result's text is one of the choices and choice_match is
    1; without choices it is -1."""
    import ctypes as C
    import json
    import os
    model = "ggml-rich.bin"
    mwx.write_synthetic_model(os.path.join(str(tmp_path), model), "micro-rich", mwx.GGML_F16,
                              MODEL_SEED)
    choices = five_choices(ctx, params(ctx, "greedy"))
    L = mwx.stt_lib()
    L.mwx_stt_new.restype = C.c_void_p
    L.mwx_stt_new.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p,
                              C.c_int, C.c_int]
    L.mwx_stt_free.argtypes = [C.c_void_p]
    fn = L.mwx_stt_transcribe_choices_f32
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_char_p),
                   C.c_int, C.c_int, C.c_float, C.c_char_p, C.c_int, C.c_float, C.c_char_p, C.c_int]
    eng = L.mwx_stt_new(str(tmp_path).encode(), model.encode(), 1, 5000, 1, b"en", 500, 0)
    assert eng
    try:
        pcm = np.ascontiguousarray(clips[1], np.float32)
        cap = 1 << 20
        buf = C.create_string_buffer(cap)

        def run(ch):
            arr = (C.c_char_p * max(1, len(ch)))(*[c.encode() for c in ch])
            r = fn(eng, pcm.ctypes.data_as(C.POINTER(C.c_float)), len(pcm), 16000, arr, len(ch),
                   -1, BIG, b"en", 1, -1.0, buf, cap)
            assert r >= 0, r
            return json.loads(buf.value.decode())

        free = run([])
        assert free["choice_match"] == -1 and free["results"]
        held = run(choices)
        print("host:", held["choice_match"], len(held["results"]))
        assert held["results"] and held["choice_match"] == 1
        for r in held["results"]:
            assert cr.member(choices, ALL, bytes.fromhex(r["text"])), r["text"]
    finally:
        L.mwx_stt_free(eng)


# ---- 3. viable prefixes, timestamps on ------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "beam"])
def test_viable_prefix_with_timestamps(ctx, clips, mode):
    p = params(ctx, mode)
    # two words the model emits on this clip by itself (so they are alive, and
    # text can win against the timestamp mass at all); at least three of them
    a, b = own_words(ctx, clips[0], params(ctx, "greedy"))
    trans, acc, start = cr.cycle_dfa([a, b], 3)
    dfa = cr.Dfa(trans, acc, start)
    con = mwx.Constraint.from_dfa(trans, acc, start)
    s = fresh(ctx, 1)
    ctx.runahead_fallbacks(s)
    assert ctx.full_batch_states([clips[0]], mwx.with_constraint(p, con, BIG), [s]) == 0
    assert ctx.runahead_fallbacks(s) == 0
    eot, beg = ctx.token("eot"), ctx.token("beg")
    n_ts = n_text = 0
    # a window's attempt starts over at the start state; segments end at timestamps
    toks = [t for sg in ctx.segments(s) for t in sg.tokens]
    st = start
    for i, t in enumerate(toks):
        if t.id == beg:
            st = start  # <|0.00|> opens a window, and only a window: a new attempt
        if t.id >= beg:
            n_ts += 1
            continue  # (a timestamp does not move the state)
        if t.id < eot:
            st = dfa.next(st, ctx.token_bytes([t.id])[0])
            n_text += 1
            assert st != 0, (i, [x.id for x in toks])
    print(mode, "text tokens", n_text, "timestamps", n_ts, "status", ctx.constraint_status(s))
    assert n_ts >= 2 and n_text >= 4
    assert ctx.constraint_status(s) in (0, 1)


# ---- 4. follow ----------------------------------------------------------------------------
def test_follow(make_model):
    """Every step's id, p and plog of a greedy constrained run against the
    reference on the engine's own teacher-forced step logits plus the
    reference's mask."""
    with mwx.Context.open(make_model("micro-rich", mwx.GGML_F16, FOLLOW_SEED)) as ctx:
        pcm = clip(FOLLOW_CLIP, 30)
        p = params(ctx, "greedy", no_timestamps=True, max_tokens=16)
        a, b, c = ctx.token_bytes(alive_ids(ctx, p, 3))
        trans, acc, start = cr.cycle_dfa([a, b + c, b + a], 8)  # (EOT only after 8 words)
        dfa = cr.Dfa(trans, acc, start)
        con = mwx.Constraint.from_dfa(trans, acc, start)
        penalty = BIG
        assert ctx.full_batch_states([pcm], mwx.with_constraint(p, con, penalty), [0]) == 0
        toks = [t for s in ctx.segments(0) for t in s.tokens]
        ids = [t.id for t in toks]
        assert len(ids) >= 8
        lcs, smask = ctx.test_logits_setup(p)
        lc = lr.LC(*(getattr(lcs, f) for f, _ in lcs._fields_))
        V = lc.n_vocab
        vocab = cr.vocab_bytes(ctx)
        seq = [ctx.token("sot")]
        if ctx.hparam("is_multilingual"):
            seq += [ctx.token("sot") + 1 + mwx.lang_id("en"), ctx.token("transcribe")]
        seq.append(ctx.token("not"))
        ctx.test_encode(pcm, cross=False)
        raw = ctx.test_decode(seq + ids)[len(seq) - 1:]
        skipped, st, n_rej_live = 0, start, 0
        for i, t in enumerate(toks):
            rej = cr.rejected(dfa, st, vocab, V, lc.eot)
            cdict = dict(zip(lr.CTL.names,
                             lr.ctl_row(**lr.ctl_of_history(ids[:i], lc.beg), want_probs=0,
                                        want_nosp=int(i == 0))))
            r = cr.reference(raw[i], smask, cdict, lc, rej, penalty)
            n_rej_live += int(st != 0)
            if t.id < lc.eot:
                st = dfa.next(st, vocab[t.id])
            if r["gap_id"] < 2 * LOGITS_TOL["micro-rich"]:
                skipped += 1
                continue
            assert t.id == r["id"], (i, t.id, r["id"], r["gap_id"])
            assert abs(float(t.p) - r["rec"]["p"]) <= r["b_rec"]["p"], (i, t.p, r["rec"]["p"])
            assert abs(float(t.plog) - r["rec"]["plog"]) <= r["b_rec"]["plog"], (i, t.plog)
        print("follow: steps", len(ids), "skipped", skipped, "steps in a live state", n_rej_live,
              "ids", ids)
        assert skipped * 10 <= len(ids)
        assert n_rej_live >= 4, "vacuous: the constraint died at once"


# ---- 5. paths agree ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "beam", "bestof"])
def test_paths_agree(ctx, clips, mode, monkeypatch):
    p0 = params(ctx, mode)
    a, b, c = own_words(ctx, clips[0], params(ctx, "greedy"), 3)
    con = mwx.Constraint.from_dfa(*cr.cycle_dfa([a, b + c, b + a], 3))
    p = mwx.with_constraint(p0, con, BIG)

    def run(q=p):
        s = fresh(ctx, 1)
        ctx.runahead_fallbacks(s)
        assert ctx.full_batch_states([clips[0]], q, [s]) == 0
        return records(ctx, s), ctx.runahead_fallbacks(s), ctx.constraint_status(s)

    ra, fb, st = run()
    assert fb == 0
    assert sum(len(s[2]) for s in ra) > 8
    monkeypatch.setenv("MWX_NO_RUNAHEAD", "1")
    host, _, st_h = run()
    monkeypatch.delenv("MWX_NO_RUNAHEAD")
    monkeypatch.setenv("MWX_NO_GRAPH", "1")
    eager, _, st_e = run()
    monkeypatch.delenv("MWX_NO_GRAPH")
    prev = mwx.set_ra_mismatch(3)
    try:
        redone, n, st_r = run()
    finally:
        mwx.set_ra_mismatch(prev)
    assert n >= 1
    assert ra == host, "run-ahead vs MWX_NO_RUNAHEAD"
    assert ra == eager, "run-ahead vs MWX_NO_GRAPH"
    assert ra == redone, "run-ahead vs a forced fallback"
    assert st == st_h == st_e == st_r
    assert run(p0)[0] != ra  # (the constraint changes something, or this shows nothing)


# ---- 6. batch invariance, the other entry points ----------------------------------------
def test_batch_invariance_and_pcm16(ctx, clips):
    p0 = params(ctx, "greedy")
    choices = five_choices(ctx, p0)
    p = mwx.with_constraint(p0, mwx.Constraint.from_choices(choices, ALL), BIG)
    assert ctx.full_batch(clips, p) == 0
    batch = [records(ctx, i) for i in range(3)]
    status = [ctx.constraint_status(i) for i in range(3)]
    assert sum(len(s[2]) for r in batch for s in r) > 3
    for i, pcm in enumerate(clips):
        assert ctx.full_batch_states([pcm], p, [5]) == 0
        assert records(ctx, 5) == batch[i], i
        assert ctx.constraint_status(5) == status[i]
    p16 = [np.round(np.asarray(c_) * 32768.0).clip(-32768, 32767).astype(np.int16) for c_ in clips]
    f16 = [mwx.pcm16_to_f32(x) for x in p16]
    assert ctx.full_batch_pcm16(p16, p) == 0
    got16 = [records(ctx, i) for i in range(3)]
    st16 = [ctx.constraint_status(i) for i in range(3)]
    assert ctx.full_batch(f16, p) == 0
    assert got16 == [records(ctx, i) for i in range(3)]
    assert st16 == [ctx.constraint_status(i) for i in range(3)] and -1 not in st16


def test_trimmed_and_chunked(ctx, tmp_path):
    path = str(tmp_path / "ggml-silero-vad.bin")
    mwx.write_synthetic_vad_model(path, SEED)
    vclips = [vr.mixed_clip(), two_clip(), vr.mixed_clip()[::-1].copy()]
    p0 = params(ctx, "greedy", no_timestamps=True)
    choices = five_choices(ctx, p0)
    p = mwx.with_constraint(p0, mwx.Constraint.from_choices(choices, ALL), BIG)
    eot = ctx.token("eot")
    with mwx.VadContext(path) as v, \
            v.trim_batch(vclips, _c_params(sr.Params(threshold=0.76)), chunk_s=1.0) as t:
        assert ctx.full_batch_trimmed([t] * 3, [0, 1, 2], p) == 0
        n_text = 0
        for i in range(3):
            if ids_of(ctx, i):
                assert cr.member(choices, ALL, text_of(ctx, i)), i
                n_text += 1
            assert ctx.constraint_status(i) == 1
        assert n_text > 0
        assert ctx.full_batch_chunked([t] * 3, [0, 1, 2], p0) == 0
        free = [records(ctx, i) for i in range(3)]
        assert [ctx.constraint_status(i) for i in range(3)] == [-1] * 3
        assert ctx.full_batch_chunked([t] * 3, [0, 1, 2], p) == 0
        got = [records(ctx, i) for i in range(3)]
        assert got != free
        for i in range(3):  # every chunk's text is one of the choices
            chunk, n_chunks = b"", 0
            for tid in ids_of(ctx, i):
                if tid == eot:
                    assert cr.member(choices, ALL, chunk), (i, chunk)
                    chunk, n_chunks = b"", n_chunks + 1
                elif tid < eot:
                    chunk += ctx.token_bytes([tid])[0]
            assert chunk == b"" and ctx.constraint_status(i) == 1
        for i in range(3):
            assert ctx.full_batch_chunked([t], [i], p, state0=4) == 0
            assert records(ctx, 4) == got[i], i


# ---- 7. with bias_phrases -----------------------------------------------------------------
def test_bias_with_constraint_stays_inside(ctx, clips):
    p0 = params(ctx, "greedy", no_timestamps=True)
    choices = five_choices(ctx, p0)
    con = mwx.Constraint.from_choices(choices, ALL)
    ids = alive_ids(ctx, p0, 14)
    phrases = [([ids[12], ids[13]], 50.0), ([ids[2]], 50.0), ([ids[11]], 80.0)]
    pb = mwx.with_bias(p0, phrases)
    assert ctx.full_batch_states([clips[1]], pb, [0]) == 0
    biased = text_of(ctx, 0)
    assert not cr.member(choices, ALL, biased)  # (the phrases alone lead outside)
    q = mwx.with_constraint(pb, con, BIG)
    assert q.n_bias_phrases == 3
    assert ctx.full_batch_states([clips[1]], q, [0]) == 0
    both = text_of(ctx, 0)
    print("bias alone", biased, "with the constraint", both)
    assert cr.member(choices, ALL, both) and ctx.constraint_status(0) == 1


# ---- 8. refusals ----------------------------------------------------------------------------
def test_refusals_leave_the_state_intact(ctx, clips):
    p = params(ctx, "greedy")
    con = mwx.Constraint.from_dfa(*cr.accept_all_dfa())
    assert ctx.full_batch_states([clips[1]], mwx.with_constraint(p, con), [0]) == 0
    before = records(ctx, 0)
    assert before and ctx.constraint_status(0) == 1
    for pen in (float("nan"), float("inf"), -float("inf"), 0.0, -1.0):
        q = mwx.with_constraint(p, con, pen)
        assert ctx.full_batch_states([clips[1]], q, [0]) == -1, pen
        assert ctx.full(clips[1], q) == -1
        p16 = np.zeros(16000, np.int16)
        assert ctx.full_batch_pcm16([p16], q) == -1
        assert records(ctx, 0) == before and ctx.constraint_status(0) == 1
    q = mwx.with_constraint(p, con)
    q.bench_fixed_steps = 4
    assert ctx.full_batch_states([clips[1]], q, [0]) == -1
    assert records(ctx, 0) == before and ctx.constraint_status(0) == 1
    # a bad penalty without a constraint is not looked at
    q = mwx.with_constraint(p, None, float("nan"))
    assert ctx.full_batch_states([clips[1]], q, [0]) == 0
    assert ctx.constraint_status(0) == -1


# ---- 9. alignment ignores it ----------------------------------------------------------------
def test_align_ignores_the_constraint(ctx, clips):
    p = params(ctx, "greedy")
    toks = alive_ids(ctx, p, 6)
    con = mwx.Constraint.from_choices(["zzzz"], 0)

    def run(q):
        assert ctx.align_batch([clips[1]], [toks], q) == 0
        return records(ctx, 0), ctx.align_rows(0).tobytes()

    plain = run(p)
    assert run(mwx.with_constraint(p, con, BIG)) == plain
    assert run(mwx.with_constraint(p, con, float("nan"))) == plain
