"""Streaming VAD on the GPU (csrc/k_vad.hip vad_stream_stage_kernel /
vad_lstm_stream_kernel / vad_stream_scan_kernel, mwx_vad_stream_*; DESIGN.md
D11) against the one-shot calls and the plain-Python rule.

Every expected value is a bit pattern or an integer: the probabilities of a
stream are compared with mwx_vad_detect_speech of the same audio byte for
byte, the segments with the restatements over the device's own probabilities.
"""
import ctypes as C

import numpy as np
import pytest

import mwx
import vad_restatement as vr
import vad_segments_restatement as sr
import vad_stream_restatement as st

pytestmark = pytest.mark.gpu

SEED = 3  # the VAD model of test_gpu_vad.py


def _c_params(prm: sr.Params) -> mwx.VadParams:
    return mwx.vad_params(threshold=prm.threshold,
                          min_speech_duration_ms=prm.min_speech_duration_ms,
                          min_silence_duration_ms=prm.min_silence_duration_ms,
                          max_speech_duration_s=prm.max_speech_duration_s,
                          speech_pad_ms=prm.speech_pad_ms, samples_overlap=prm.samples_overlap)


def two_clip():
    """5 s + 77 samples of zeros with two noise bursts (as test_gpu_vad_segments.py)."""
    rng = np.random.default_rng(11)
    x = np.zeros(5 * 16000 + 77, np.float32)
    x[8000:30000] = (0.3 * rng.standard_normal(22000)).astype(np.float32)
    x[52000:72000] = (0.3 * rng.standard_normal(20000)).astype(np.float32)
    return x


CLIPS = {"mixed": vr.mixed_clip(), "n1": vr.noise_clip(1, seed=31), "n511": vr.noise_clip(511, seed=32),
         "n512": vr.noise_clip(512, seed=33), "n513": vr.noise_clip(513, seed=34),
         "n3721": vr.noise_clip(3721, seed=35), "two": two_clip()}
BIT_CLIPS = ["mixed", "n1", "n511", "n512", "n513", "n3721"]


def _plan(name, n):
    """Feed sizes that sum to n."""
    if name == "whole":
        return [n]
    if name == "ones":
        k = min(n, 1100)
        return [1] * k + ([n - k] if n > k else [])
    if name == "random":
        rng = np.random.default_rng(99)
        out = []
        while sum(out) < n:
            out.append(min(n - sum(out), int(rng.integers(0, 3001))))
        return out
    step = {"f511": 511, "f512": 512, "f513": 513, "cadence": 8000}[name]
    return [min(step, n - a) for a in range(0, n, step)]


PLANS = ["whole", "ones", "f511", "f512", "f513", "cadence", "random"]


class _Vad:
    def __init__(self, ctx):
        self.ctx = ctx
        self._detect = {}

    def detect(self, name, n):
        """detect(CLIPS[name][:n]), computed once per prefix and left unchanged."""
        key = (name, n)
        if key not in self._detect:
            p = self.ctx.detect(CLIPS[name][:n])
            p.setflags(write=False)
            self._detect[key] = p
        return self._detect[key]


@pytest.fixture(scope="module")
def vad(tmp_path_factory):
    d = tmp_path_factory.mktemp("vadstream")
    path = str(d / "ggml-silero-vad.bin")
    mwx.write_synthetic_vad_model(path, SEED)
    with mwx.VadContext(path) as v:
        yield _Vad(v)


def _check_stream(vad, s, name, fed):
    want = vad.detect(name, fed)
    got = s.probs()
    assert s.n_samples == fed
    assert s.n_probs == len(want) == mwx.lib().mwx_vad_n_chunks(fed)
    assert got.tobytes() == want.tobytes(), (name, fed)
    want_max = float(want.max()) if len(want) else 0.0
    assert np.float32(s.max_prob).tobytes() == np.float32(want_max).tobytes()


# ---- 1. invariant 1: the probabilities of a one-shot call, bit for bit --------------------
@pytest.mark.parametrize("plan", PLANS)
def test_probs_equal_one_shot_bitwise(vad, plan):
    n_feeds = n_partial = 0
    for name in BIT_CLIPS:
        x = CLIPS[name]
        with vad.ctx.stream() as s:
            _check_stream(vad, s, name, 0)
            fed = 0
            for k in _plan(plan, len(x)):
                s.feed(x[fed:fed + k])
                fed += k
                _check_stream(vad, s, name, fed)
                n_feeds += 1
                n_partial += fed % 512 != 0
            assert fed == len(x)
    assert n_feeds >= len(BIT_CLIPS) and n_partial > 0  # provisional chunks were compared


def test_bit_equality_has_power(vad):
    """A stream that dropped h and c at a call boundary would fail the test
    above: restarting the net at chunk 64 of `mixed` moves a later probability
    by far more than a rounding."""
    x = CLIPS["mixed"]
    whole = vad.detect("mixed", len(x))
    restarted = vad.ctx.detect(x[64 * 512:])
    assert len(restarted) == len(whole) - 64
    assert np.max(np.abs(restarted - whole[64:])) > 1e-3


# ---- 2. a batch gives the bits of the single calls ---------------------------------------
def _run_batch(vad, order):
    names = ["mixed", "n3721", "two", "n513", "mixed"]
    plans = ["cadence", "f511", "random", "ones", "f513"]
    feeds = [_plan(p, len(CLIPS[n])) for n, p in zip(names, plans)]
    feeds[1] = [0] + feeds[1]             # a 0-sample feed inside shared calls
    absent = {4: {1, 3, 4}}               # stream 4 sits these calls out
    streams = [vad.ctx.stream() for _ in names]
    try:
        pos = [0] * 5   # samples fed
        at = [0] * 5    # next entry of feeds[i]
        call = 0
        n_shared = 0
        while any(at[i] < len(feeds[i]) for i in range(5)):
            live = [i for i in order if at[i] < len(feeds[i]) and call not in absent.get(i, ())]
            call += 1
            if not live:
                continue
            pcms = []
            for i in live:
                k = feeds[i][at[i]]
                pcms.append(CLIPS[names[i]][pos[i]:pos[i] + k])
                pos[i] += k
                at[i] += 1
            mwx.VadStream.feed_batch([streams[i] for i in live], pcms)
            n_shared += len(live) > 1
            if call % 7 == 1 or call < 4:  # spot checks on the way
                for i in live:
                    _check_stream(vad, streams[i], names[i], pos[i])
        assert n_shared > 10
        for i, n in enumerate(names):
            assert pos[i] == len(CLIPS[n])
            _check_stream(vad, streams[i], n, pos[i])
        return [s.probs().tobytes() for s in streams]
    finally:
        for s in streams:
            s.free()


def test_batch_equals_single_bitwise(vad):
    a = _run_batch(vad, [0, 1, 2, 3, 4])
    b = _run_batch(vad, [4, 3, 2, 1, 0])
    assert a == b


# ---- 3. reset ----------------------------------------------------------------------------
def test_reset_equals_fresh_stream(vad):
    x, y = CLIPS["mixed"], CLIPS["two"]
    prm = _c_params(sr.Params(threshold=0.76))
    with vad.ctx.stream(prm) as s, vad.ctx.stream(prm) as fresh:
        s.feed(x[:40000])          # state, scan registers and a tail of 40000 % 512 samples
        assert s.n_probs == 79 and s.max_prob > 0.0 and s.n_samples % 512 != 0
        s.reset()
        assert (s.n_samples, s.n_probs, s.max_prob, s.segments(), s.in_speech) == (0, 0, 0.0, [], False)
        fed = 0
        for k in _plan("f513", len(y)):
            mwx.VadStream.feed_batch([s, fresh], [y[fed:fed + k]] * 2)
            fed += k
            assert s.probs().tobytes() == fresh.probs().tobytes()
            assert s.segments() == fresh.segments() and s.in_speech == fresh.in_speech
        _check_stream(vad, s, "two", len(y))
        s.finish()
        s.reset()                  # a finished stream is usable again after reset
        s.feed(y[:1000])
        _check_stream(vad, s, "two", 1000)


# ---- 4. invariant 2: segments on the network's own probabilities --------------------------
@pytest.mark.parametrize("name,thr", [("mixed", 0.76), ("two", 0.80), ("two", 0.74)])
@pytest.mark.parametrize("plan", ["cadence", "f513", "random"])
def test_segments_equal_restatement(vad, name, thr, plan):
    x = CLIPS[name]
    p = vad.detect(name, len(x))
    prm = sr.Params(threshold=thr)
    t32, n32 = np.float32(thr), sr.derived(prm)[1]
    # power: no probability is near either threshold (as test_gpu_vad_segments.py)
    assert np.min(np.abs(p - t32)) > 1e-3 and np.min(np.abs(p - n32)) > 1e-3
    scan = st.OnlineScan(prm)
    early = 0
    with vad.ctx.stream(_c_params(prm)) as s:
        fed = 0
        feeds = _plan(plan, len(x))
        for j, k in enumerate(feeds):
            s.feed(x[fed:fed + k])
            fed += k
            scan.feed(p[scan.i:fed // 512])  # the whole chunks so far
            assert s.segments() == scan.closed, (fed, s.segments(), scan.closed)
            assert s.in_speech == scan.triggered
            if j + 1 < len(feeds):
                early = len(scan.closed)
        s.finish()
        scan.finish(len(x))
        raw = s.segments()
        assert raw == scan.closed
        assert not s.in_speech
    assert early >= 1  # a segment closed before the last feed
    want = sr.segments(p, len(x), prm)
    assert st.pad(raw, len(x), prm) == want
    got_cs = vad.ctx.segments_from_samples(x, _c_params(prm))
    assert got_cs == [(np.float32(a) / np.float32(160.0), np.float32(b) / np.float32(160.0))
                      for a, b in st.pad(raw, len(x), prm)]


# ---- 5. the scan alone, on given probabilities -------------------------------------------
def _scan_case(vad, p, N, prm, splits):
    ev, state = vad.ctx.test_stream_scan(p, splits, _c_params(prm))
    scan = st.OnlineScan(prm)
    scan.feed(p)
    assert ev == scan.closed, (prm, splits, p.tolist()[:64])
    assert state == scan.state()
    tail = scan.finish(N)
    assert st.pad(ev + tail, N, prm) == sr.segments(p, N, prm)
    return len(ev)


def test_scan_hook_table_and_random(vad):
    rng = np.random.default_rng(2025)
    for name in sorted(sr.TABLE):
        rr, N, prm, _, _, _ = sr.TABLE[name]
        p = sr.runs(*rr)
        _scan_case(vad, p, N, prm, [len(p)])
        _scan_case(vad, p, N, prm, st.random_splits(rng, len(p), 7))
    n_events = n_max = 0
    for _ in range(300):
        p, N, prm = sr.random_case(rng)
        k = _scan_case(vad, p, N, prm, st.random_splits(rng, len(p)))
        n_events += k
        n_max += prm.max_speech_duration_s < 100 and k > 0
    assert n_events >= 300 and n_max >= 30


def test_scan_hook_long_stream(vad):
    """18 750 chunks (10 minutes), 16 at a time: positions pass 2^23."""
    rng = np.random.default_rng(77)
    p, N, _ = sr.random_case(rng, n_chunks=18750)
    prm = sr.Params(threshold=0.6, max_speech_duration_s=2.5)
    splits = [16] * (18750 // 16) + [18750 % 16]
    ev, state = vad.ctx.test_stream_scan(p, splits, _c_params(prm))
    scan = st.OnlineScan(prm)
    scan.feed(p)
    assert ev == scan.closed and state == scan.state()
    assert len(ev) > 50 and ev[-1][2] > 2 ** 23 and state[5] == 18750


# ---- 6. refusals -------------------------------------------------------------------------
def test_refusals(vad, tmp_path):
    L = mwx.lib()
    v = vad.ctx
    for bad in (dict(threshold=0.0), dict(threshold=1.0), dict(threshold=float("nan")),
                dict(min_speech_duration_ms=-1), dict(min_silence_duration_ms=-1),
                dict(speech_pad_ms=-1), dict(max_speech_duration_s=0.0),
                dict(max_speech_duration_s=float("nan")), dict(samples_overlap=-0.1),
                dict(samples_overlap=float("nan"))):
        assert not L.mwx_vad_stream_init(v.vctx, mwx.vad_params(**bad)), bad
    x = vr.noise_clip(480001, seed=5)

    def feed(ctx, streams, n):
        k = len(streams)
        hs = (C.c_void_p * k)(*[s.s for s in streams])
        ptrs = (C.c_void_p * k)(*[x.ctypes.data] * k)
        lens = (C.c_int * k)(*n)
        return L.mwx_vad_stream_feed_batch(ctx.vctx, hs, ptrs, lens, k)

    with v.stream() as a, v.stream() as b:
        assert feed(v, [a, b], [100, -1]) < 0
        assert feed(v, [a, b], [100, 480001]) < 0
        assert feed(v, [a, b, a], [100, 100, 100]) < 0          # a stream twice
        assert (a.n_samples, b.n_samples) == (0, 0)             # refused calls change nothing
        assert feed(v, [a, b], [100, 480000]) == 0
        assert (a.n_samples, b.n_samples, b.n_probs) == (100, 480000, 938)
        path = str(tmp_path / "other-vad.bin")
        mwx.write_synthetic_vad_model(path, SEED)
        with mwx.VadContext(path) as other:
            assert feed(other, [a], [100]) < 0                  # a stream of another context
            with other.stream() as c:
                assert feed(v, [a, c], [100, 100]) < 0
                assert feed(other, [c], [100]) == 0
        a.finish()
        assert feed(v, [a], [100]) < 0                          # finished
        assert L.mwx_vad_stream_finish(a.s) < 0
        assert feed(v, [b], [0]) == 0
        assert a.n_samples == 100
