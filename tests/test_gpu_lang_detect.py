"""Language identification through the engine (DESIGN.md "Language
identification"): the detection pass keeps the per-language distribution
(mwx_full_lang_probs_from_state), and mwx_full_params.lang_ids gives every
batch entry a language of its own. Models micro-ml (51865 entries) and micro-v3
(51866), 1-3 s synthetic clips.

Exact: a clip's probabilities alone, inside a batch and between a
detection-only call and a full transcription; an entry's token records (and
alignment rows) with lang_ids against the same clip run alone. Bounded: the
probabilities against tests/lang_ref.py on the logits the pass fed the kernel.
"""
import numpy as np
import pytest

import lang_ref as lr
import mwx

pytestmark = pytest.mark.gpu

SECONDS = (1.0, 2.0, 3.0)


def clip(k, seconds):
    return mwx.pcm16_to_f32(mwx.synth_pcm16(k, int(seconds * 16000)))


@pytest.fixture(scope="module")
def clips():
    return [clip(20 + i, s) for i, s in enumerate(SECONDS)]


@pytest.fixture(scope="module", params=["micro-ml", "micro-v3"])
def path(request, make_model):
    return make_model(request.param)


@pytest.fixture(scope="module")
def ctx(path):
    c = mwx.Context.open(path)
    yield c
    c.close()


def params(ctx, language=b"auto", strategy=mwx.SAMPLING_GREEDY, **kw):
    p = ctx.default_params(strategy)
    p.language = language
    p.temperature_inc = 0.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def records(ctx, state=0):
    """token_records with the probability as its bit pattern."""
    return [(i, t0, t1, int(bits([p])[0])) for i, t0, t1, p in ctx.token_records(state)]


def test_detection_keeps_the_distribution(ctx, clips):
    n_lang = mwx.lang_max_id() + 1
    assert n_lang == lr.N_LANG == 100
    p = params(ctx)
    alone = []
    for c in clips:
        ctx.lang_keep(True, 0)
        assert ctx.full(c, p) == 0
        probs = ctx.lang_probs(0)
        logits = ctx.lang_last(0)
        assert probs.shape == (n_lang,) and logits.shape == (n_lang,)
        r = lr.reference(logits, 0, n_lang)
        ratios = {}
        bad = lr.compare(r, dict(p=probs, best=int(np.argmax(logits))), ratios)
        print("probs vs reference:", ratios)
        assert not bad, bad
        assert abs(float(probs.astype(np.float64).sum()) - 1.0) <= float(r["b_p"].sum()) + n_lang * lr.U
        lang = ctx.lang_id(0)
        assert 0 <= lang < n_lang and probs[lang] == probs.max()
        if r["gap"] > 0:
            assert lang == r["best"]
        alone.append(probs)
    # a fixed language: the call did not detect
    assert ctx.full(clips[0], params(ctx, b"tr")) == 0
    assert ctx.lang_probs(0).size == 0 and ctx.lang_last(0).size == 0
    assert ctx.lang_id(0) == mwx.lang_id("tr")
    # inside a batch of 3: the same bits
    assert ctx.full_batch(clips, p) == 0
    for i in range(3):
        assert (bits(ctx.lang_probs(i)) == bits(alone[i])).all(), i
    # a detection-only call: the same bits, no segments
    pd = params(ctx, detect_language=True)
    assert ctx.full_batch(clips, pd) == 0
    for i in range(3):
        assert (bits(ctx.lang_probs(i)) == bits(alone[i])).all(), i
        assert ctx.segments(i) == []
        assert ctx.lang_id(i) == int(np.argmax(alone[i]))
    ctx.lang_keep(False, 0)
    # the getter's argument check
    import ctypes as C
    fn = mwx.lib().mwx_full_lang_probs_from_state
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    buf = np.zeros(n_lang, np.float32)
    assert fn(ctx.state(0), mwx.fptr(buf), n_lang - 1) == -1
    assert fn(ctx.state(0), None, n_lang) == -1
    assert fn(None, mwx.fptr(buf), n_lang) == -1
    assert fn(ctx.state(0), mwx.fptr(buf), n_lang) == n_lang


@pytest.mark.parametrize("strategy", [mwx.SAMPLING_GREEDY, mwx.SAMPLING_BEAM_SEARCH])
def test_lang_ids_per_entry(path, clips, strategy):
    """Beam search draws its candidates with the state's own random generator,
    which persists from call to call (whisper.cpp's decoders[0].rng): the batch
    and the clips run alone each start on fresh states, entry b alone on state
    b of a second context."""
    with mwx.Context.open(path) as ctx, mwx.Context.open(path) as solo:
        _lang_ids_per_entry(ctx, solo, clips, strategy)


def _lang_ids_per_entry(ctx, solo, clips, strategy):
    def prm(language=b"auto"):
        p = params(ctx, language, strategy=strategy)
        if strategy == mwx.SAMPLING_BEAM_SEARCH:
            p.beam_search.beam_size = 5
        return p

    def state_result(i, c=ctx):
        return records(c, i), c.lang_id(i), bits(c.lang_probs(i)).tolist()

    en, tr = mwx.lang_id("en"), mwx.lang_id("tr")
    want = []
    for i, (c, lang) in enumerate(zip(clips, (b"en", b"tr", b"auto"))):
        assert solo.full(c, prm(lang), state_index=i) == 0
        want.append(state_result(i, solo))
    assert sum(len(w[0]) for w in want) > 0
    p = prm()
    assert ctx.full_batch(clips, p, lang_ids=[en, tr, -1]) == 0
    got = [state_result(i) for i in range(3)]
    assert got == want
    assert got[0][1] == en and got[1][1] == tr and got[0][2] == [] and len(got[2][2]) == 100
    # an id above the table: refused
    bad = mwx.lang_max_id() + 1
    assert ctx.full_batch(clips, p, lang_ids=[en, bad, -1]) == -3
    assert ctx.full(clips[0], p, lang_id=bad) == -3
    if strategy != mwx.SAMPLING_GREEDY:
        return
    # entries without an id follow params.language, also a fixed one
    assert ctx.full_batch(clips, prm(b"tr"), lang_ids=[en, -1, -1]) == 0
    assert records(ctx, 0) == want[0][0] and records(ctx, 1) == want[1][0]
    assert ctx.lang_id(2) == tr and ctx.lang_probs(2).size == 0
    # int16 input takes the same path
    p16 = [mwx.synth_pcm16(20 + i, int(s * 16000)) for i, s in enumerate(SECONDS)]
    assert ctx.full_batch_pcm16(p16, p, lang_ids=[en, tr, -1]) == 0
    assert [state_result(i) for i in range(3)] == want
    # mwx_full_with_state reads lang_ids[0]
    assert ctx.full(clips[1], p, lang_id=tr) == 0
    assert state_result(0) == want[1]
    # NULL, and ids below 0 only: a plain call's records
    assert ctx.full_batch(clips, p) == 0
    plain = [state_result(i) for i in range(3)]
    assert ctx.full_batch(clips, p, lang_ids=None) == 0
    assert [state_result(i) for i in range(3)] == plain
    assert ctx.full_batch(clips, p, lang_ids=[-1, -1, -5]) == 0
    assert [state_result(i) for i in range(3)] == plain


def test_lang_ids_in_align_batch(ctx, clips):
    eot = ctx.token("eot")
    toks = [[int(t) for t in np.random.default_rng([3, i]).integers(0, eot, 5 + i)]
            for i in range(3)]
    en, tr = mwx.lang_id("en"), mwx.lang_id("tr")

    def result(state):
        rows = ctx.align_rows(state)
        return (records(ctx, state), bits(rows["plog"]).tolist(), rows["top_id"].tolist(),
                bits(rows["top_plog"]).tolist(), ctx.lang_id(state))

    want = []
    for c, t, lang in zip(clips, toks, (b"en", b"tr", b"auto")):
        assert ctx.align_batch([c], [t], params(ctx, lang), state_indices=[5]) == 0
        want.append(result(5))
    assert all(len(w[1]) == len(t) + 1 for w, t in zip(want, toks))
    assert ctx.align_batch(clips, toks, params(ctx), lang_ids=[en, tr, -1]) == 0
    assert [result(i) for i in range(3)] == want
    assert len(ctx.lang_probs(2)) == 100 and ctx.lang_probs(0).size == 0
    assert ctx.align_batch(clips, toks, params(ctx), lang_ids=[en, tr, 100]) == -3


def test_english_only_model_ignores_lang_ids(make_model, clips):
    with mwx.Context.open(make_model("micro")) as ctx:
        p = params(ctx, b"en")
        assert ctx.full_batch(clips, p) == 0
        plain = [records(ctx, i) for i in range(3)]
        assert sum(len(r) for r in plain) > 0
        assert ctx.full_batch(clips, p, lang_ids=[mwx.lang_id("tr"), -1, 1000]) == 0
        assert [records(ctx, i) for i in range(3)] == plain
