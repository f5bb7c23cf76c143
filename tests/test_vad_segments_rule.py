"""The numpy restatement of the VAD segment rule (tests/vad_segments_restatement.py)
reproduces the table of the rule's definition, and its outputs
keep the rule's invariants on random inputs. No GPU."""
import numpy as np
import pytest

import vad_segments_restatement as sr


@pytest.mark.parametrize("name", sorted(sr.TABLE))
def test_table(name):
    rr, N, prm, want_segs, want_len, want_pieces = sr.TABLE[name]
    p = sr.runs(*rr)
    assert len(p) == (N + sr.CHUNK - 1) // sr.CHUNK
    segs = sr.segments(p, N, prm)
    assert segs == want_segs
    pcs, total = sr.pieces(segs, prm)
    assert total == want_len
    if want_pieces is not None:
        assert pcs == want_pieces
    if name == "I":  # contiguous speech: no inserted silence
        assert all(pcs[k][2] + pcs[k][1] == pcs[k + 1][2] for k in range(len(pcs) - 1))


def test_time_map_case_m():
    rr, N, prm, _, _, _ = sr.TABLE["M"]
    pcs, _ = sr.pieces(sr.segments(sr.runs(*rr), N, prm), prm)
    for t, (as_start, as_end) in sr.M_TIME_MAP.items():
        assert sr.map_time(pcs, t, False) == as_start
        assert sr.map_time(pcs, t, True) == as_end
    assert sr.map_time(pcs, -1, False) == -1 and sr.map_time(pcs, -1, True) == -1


def test_properties_on_random_inputs():
    rng = np.random.default_rng(7)
    n_with_segments = n_multi = 0
    for _ in range(200):
        p, N, prm = sr.random_case(rng)
        segs = sr.segments(p, N, prm)
        for s, e in segs:
            assert 0 <= s < e <= N
        for (_, e0), (s1, _) in zip(segs, segs[1:]):
            assert e0 <= s1
        pcs, total = sr.pieces(segs, prm)
        assert len(pcs) == len(segs) <= len(p)
        for k, (src, ln, dst) in enumerate(pcs):
            assert ln > 0 and src + ln <= N
            if k + 1 < len(pcs):
                assert src + ln <= pcs[k + 1][0] and dst + ln <= pcs[k + 1][2]
        n_with_segments += bool(segs)
        n_multi += len(segs) > 1
        for is_end in (False, True):
            prev = 0
            for t in range(0, total // 160 + 3):
                m = sr.map_time(pcs, t, is_end)
                assert prev <= m <= N // 160
                prev = m
    assert n_with_segments >= 100 and n_multi >= 30
