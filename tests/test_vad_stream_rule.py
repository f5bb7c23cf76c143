"""The online form of the VAD segment rule (tests/vad_stream_restatement.py,
DESIGN.md D11) against the one-shot restatement (vad_segments_restatement.py,
D7): raw segments + finish + padding are the public segments, whatever the
split points, and a chunk closes at most one segment. No GPU."""
import numpy as np
import pytest

import vad_segments_restatement as sr
import vad_stream_restatement as st


@pytest.mark.parametrize("name", sorted(sr.TABLE))
def test_table(name):
    rr, N, prm, want_segs, _, _ = sr.TABLE[name]
    p = sr.runs(*rr)
    raw = st.raw_segments(p, N, prm)
    assert st.pad(raw, N, prm) == want_segs == sr.segments(p, N, prm)
    one_at_a_time = st.raw_segments(p, N, prm, splits=[1] * len(p))
    assert one_at_a_time == raw


def test_random_cases_equal_the_one_shot_rule():
    rng = np.random.default_rng(417)
    n_segments = n_max_speech = n_finish = n_early = 0
    for _ in range(1500):
        p, N, prm = sr.random_case(rng)
        want = sr.segments(p, N, prm)
        scan = st.OnlineScan(prm)
        per_step = [scan.step(v) for v in p]
        assert max(len(s) for s in per_step) <= 1  # at most one close per chunk
        early = list(scan.closed)
        last = scan.finish(N)
        raw = scan.closed
        assert st.pad(raw, N, prm) == want, (prm, N, p.tolist())
        # closed_at: the end of the closing chunk, never before the segment's end
        for k, closed in enumerate(per_step):
            for s, e, at in closed:
                assert at == sr.CHUNK * (k + 1) and s < e <= at - sr.CHUNK
        for s, e, at in last:
            assert (e, at) == (N, N)
        # carried across arbitrary split points
        for _ in range(2):
            splits = st.random_splits(rng, len(p))
            assert st.raw_segments(p, N, prm, splits) == raw
        n_segments += len(raw)
        n_max_speech += prm.max_speech_duration_s < 100 and len(raw) > 0
        n_finish += len(last)
        n_early += len(early)
    print(f"{n_segments} segments, {n_early} closed by a step, {n_finish} by finish, "
          f"{n_max_speech} cases with max_speech")
    assert n_segments >= 3000 and n_finish >= 100 and n_early >= 2000 and n_max_speech >= 200


def test_state_is_all_that_crosses_a_split():
    """Two scans in the same state give the same future: the registers of
    state() are the whole state."""
    rng = np.random.default_rng(5)
    for _ in range(100):
        p, N, prm = sr.random_case(rng)
        k = int(rng.integers(0, len(p) + 1))
        a = st.OnlineScan(prm)
        a.feed(p[:k])
        b = st.OnlineScan(prm)
        (b.triggered, b.start, b.temp_end, b.prev_end, b.next_start, b.i) = a.state()
        b.triggered = bool(b.triggered)
        n0 = len(a.closed)
        a.feed(p[k:])
        b.feed(p[k:])
        a.finish(N)
        b.finish(N)
        assert a.closed[n0:] == b.closed
