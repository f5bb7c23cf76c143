"""The chunk plan (deviation D10; INTEGRATION.md, "Chunked long-form
transcription") in plain Python, on top of the segment rule's restatement.
Written from the rule's text, not from csrc/k_vad.hip; the GPU tests compare
the kernel with it as integers.

A clip's pieces are the (src, len, dst) triples of vad_segments_restatement;
L is the cap in samples. A chunk is (first piece, n pieces, start, len), start
and len in samples of the compacted clip.
"""
import vad_segments_restatement as sr


def cap_samples(chunk_s):
    """The cap of mwx_vad_trim_batch_chunked: (int64)((double)chunk_s * 16000)."""
    return int(float(chunk_s) * 16000.0)


def chunks(pieces, L):
    """a_0 = 0; a_{j+1} = the smallest b > a_j with b == m or
    dst_b + len_b - dst_{a_j} > L."""
    m = len(pieces)
    out = []
    a = 0
    while a < m:
        c = pieces[a][2]
        b = a + 1
        while b < m and pieces[b][2] + pieces[b][1] - c <= L:
            b += 1
        last = pieces[b - 1]
        out.append((a, b - a, c, last[2] + last[1] - c))
        a = b
    return out


def chunk_pieces(pieces, chunk):
    """The chunk's pieces with dst counted from the chunk's start."""
    first, n, start, _ = chunk
    return [(src, ln, dst - start) for src, ln, dst in pieces[first:first + n]]


def chunk_map_time(pieces, chunk, t, is_end):
    """Chunk-local centiseconds -> the caller's centiseconds: the time map of
    the segment rule applied to the chunk's own pieces."""
    return sr.map_time(chunk_pieces(pieces, chunk), t, is_end)


def alternating(n):
    """(probs, N, Params) of n chunks, speech and silence by turns, with
    parameters that make every speech chunk a segment of its own."""
    probs = sr.runs(*[(0.9, 1), (0.1, 1)] * (n // 2))
    prm = sr.Params(threshold=0.5, min_speech_duration_ms=0, min_silence_duration_ms=0,
                    speech_pad_ms=0, samples_overlap=0.0)
    return probs, sr.CHUNK * n, prm


def table_pieces(name):
    """The pieces of a case of the segment rule's table."""
    rn, N, prm, _, _, _ = sr.TABLE[name]
    return sr.pieces(sr.segments(sr.runs(*rn), N, prm), prm)[0]


# The table of the rule's definition: (case of sr.TABLE, L) -> chunks.
TABLE = {
    ("M", 16000): [(0, 1, 0, 12800), (1, 1, 14400, 11200)],
    ("M", 32000): [(0, 2, 0, 25600)],
    ("I", 16000): [(0, 1, 0, 15104), (1, 1, 15104, 15360), (2, 1, 30464, 15360),
                   (3, 1, 45824, 5376)],
    ("I", 32000): [(0, 2, 0, 30464), (2, 2, 30464, 20736)],
    ("I", 480000): [(0, 4, 0, 51200)],
    ("J", 16000): [(0, 1, 0, 12320), (1, 1, 12320, 15808)],
    ("J", 32000): [(0, 2, 0, 28128)],
}
# case M at L = 16000, chunk 1: t -> (start-type, end-type)
M_CHUNK1_TIME_MAP = {0: (221, 221), 35: (256, 256), 70: (291, 291), 71: (291, 291)}
# alternating(n): pieces at n = 126 / 128 / 130 / 300, and L -> chunk counts
ALT_N = (126, 128, 130, 300)
ALT_PIECES = (63, 64, 65, 150)
ALT_CHUNKS = {8960: (13, 13, 13, 30), 511: (63, 64, 65, 150), 10 ** 9: (1, 1, 1, 1)}
ALT_8960_FIRST_TWO = [(0, 5, 0, 8960), (5, 5, 10560, 8960)]
