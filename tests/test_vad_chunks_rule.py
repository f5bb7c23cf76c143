"""The plain-Python restatement of the chunk plan (tests/vad_chunks_restatement.py)
reproduces the table of the rule's definition, a single
full-clip chunk maps times exactly as the segment rule's map, and its outputs
keep the rule's invariants on random inputs. No GPU."""
import numpy as np
import pytest

import vad_chunks_restatement as cr
import vad_segments_restatement as sr


@pytest.mark.parametrize("name,L", sorted(cr.TABLE))
def test_table(name, L):
    assert cr.chunks(cr.table_pieces(name), L) == cr.TABLE[(name, L)]


def test_chunk_time_map_case_m():
    pcs = cr.table_pieces("M")
    ch = cr.chunks(pcs, 16000)
    for t, (as_start, as_end) in cr.M_CHUNK1_TIME_MAP.items():
        assert cr.chunk_map_time(pcs, ch[1], t, False) == as_start
        assert cr.chunk_map_time(pcs, ch[1], t, True) == as_end
    for is_end in (False, True):
        assert cr.chunk_map_time(pcs, ch[1], -1, is_end) == -1
        # chunk 0 ends with its own last piece: nothing maps into the next chunk
        assert cr.chunk_map_time(pcs, ch[0], 80, is_end) == 109
        assert cr.chunk_map_time(pcs, ch[0], 500, is_end) == 109


def test_full_clip_chunk_maps_like_the_segment_rule():
    pcs = cr.table_pieces("M")
    (ch,) = cr.chunks(pcs, 32000)
    assert ch == (0, 2, 0, 25600)
    for t in range(-2, 25600 // 160 + 40):
        for is_end in (False, True):
            assert cr.chunk_map_time(pcs, ch, t, is_end) == sr.map_time(pcs, t, is_end)


@pytest.mark.parametrize("n,m", zip(cr.ALT_N, cr.ALT_PIECES))
def test_alternating_cases(n, m):
    probs, N, prm = cr.alternating(n)
    pcs, _ = sr.pieces(sr.segments(probs, N, prm), prm)
    assert len(pcs) == m
    i = cr.ALT_N.index(n)
    for L, counts in cr.ALT_CHUNKS.items():
        assert len(cr.chunks(pcs, L)) == counts[i], L
    assert cr.chunks(pcs, 8960)[:2] == cr.ALT_8960_FIRST_TWO
    assert len(cr.chunks(pcs, 8959)) > len(cr.chunks(pcs, 8960))  # 8960 is an exact fit


def test_no_pieces_no_chunks():
    assert cr.chunks([], 16000) == []
    assert cr.cap_samples(1.0) == 16000 and cr.cap_samples(30.0) == 480000
    assert cr.cap_samples(np.float32(1.1)) == int(float(np.float32(1.1)) * 16000.0)


def test_properties_on_random_inputs():
    rng = np.random.default_rng(11)
    n_multi = n_overlong = 0
    for i in range(2000):
        p, N, prm = sr.random_case(rng)
        pcs, total = sr.pieces(sr.segments(p, N, prm), prm)
        L = (16000, 24000, 48000, 480000)[i % 4]
        ch = cr.chunks(pcs, L)
        # a partition of the pieces, in order
        nxt = 0
        for first, n, start, ln in ch:
            assert first == nxt and n >= 1
            nxt += n
            last = pcs[first + n - 1]
            assert start == pcs[first][2] and ln == last[2] + last[1] - start
            if ln > L:  # only an overlong piece exceeds the cap
                assert n == 1
                n_overlong += 1
        assert nxt == len(pcs)
        assert bool(ch) == bool(pcs)
        # the first piece of the next chunk would not have fit
        for (_, _, start, _), (f1, _, _, _) in zip(ch, ch[1:]):
            assert pcs[f1][2] + pcs[f1][1] - start > L
        if ch:
            assert ch[-1][2] + ch[-1][3] == total
        n_multi += len(ch) > 1
    assert n_multi >= 50 and n_overlong >= 20, (n_multi, n_overlong)
