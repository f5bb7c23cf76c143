"""One language per recording (mwx_full_params.chunk_language =
MWX_CHUNK_LANG_RECORDING; DESIGN.md, deviation D13) in plain Python. Written
from the rule's text, not from csrc/driver.inc; the GPU test compares the
engine's pooled probabilities with pool() bit for bit.

A recording's chunks have lengths len_0, len_1, ... in samples at 16 kHz, in
chunk order; chunk j's detection gives the probabilities p_j [n_lang] (f32).
"""
import numpy as np

POOL_SAMPLES = 480000  # 30 s


def counts(length):
    """The engine decodes a chunk that has at least ten mel frames (its 0.1-s
    rule: 1 + (len - 200) / 160 >= 10 in C integer arithmetic, len >= 1640
    samples); a shorter one decodes to nothing and is not looked at."""
    return length > 0 and 1 + int((length - 200) / 160) >= 10


def pooled_chunks(lengths):
    """The indices of the chunks that are detected and pooled: the chunks that
    count, in order, up to and including the one at which their summed length
    reaches POOL_SAMPLES; all of them if it never does."""
    out, total = [], 0
    for j, n in enumerate(lengths):
        if total >= POOL_SAMPLES:
            break
        if not counts(n):
            continue
        out.append(j)
        total += n
    return out


def pool(lengths, probs):
    """(P as f32 [n_lang], language id) of the pooled chunks' (length,
    probabilities): P = sum_j len_j p_j / sum_j len_j accumulated in double in
    chunk order and rounded to f32; the language is the lowest id among the
    maxima of the rounded P, so that it can be recomputed from what the state
    reports. (None, -1) without chunks."""
    if not len(lengths):
        return None, -1
    acc = np.zeros(len(probs[0]), np.float64)
    total = 0
    for n, p in zip(lengths, probs):
        acc += float(n) * np.asarray(p, np.float32).astype(np.float64)
        total += int(n)
    P = (acc / float(total)).astype(np.float32)
    return P, int(np.argmax(P))


def recording_language(lengths, probs_of):
    """The rule end to end: probs_of(j) gives chunk j's probabilities."""
    idx = pooled_chunks(lengths)
    return pool([lengths[j] for j in idx], [probs_of(j) for j in idx])


# lengths -> pooled chunk indices
TABLE_CHUNKS = [
    ([], []),
    ([1639], []),
    ([1640], [0]),
    ([100, 1639, 0], []),
    ([479999], [0]),
    ([480000], [0]),
    ([480001], [0]),
    ([479999, 16000, 16000], [0, 1]),       # 479 999 has not reached it
    ([480000, 16000, 16000], [0]),          # 480 000 has
    ([240000, 240000, 16000], [0, 1]),
    ([240000, 239999, 16000, 16000], [0, 1, 2]),
    ([240000, 240001, 16000], [0, 1]),
    ([240000, 1000, 239999, 1639, 5000, 9000], [0, 2, 4]),  # short chunks add nothing
    ([16000, 32000, 8000], [0, 1, 2]),      # never reached: all
    ([1000, 16000], [1]),
]

# (lengths, probs) -> (P, id), hand-computed
TABLE_POOL = [
    ([16000], [[0.25, 0.75]], [0.25, 0.75], 1),
    ([16000, 16000], [[1.0, 0.0], [0.0, 1.0]], [0.5, 0.5], 0),            # tie: lowest id
    ([16000, 48000], [[1.0, 0.0], [0.0, 1.0]], [0.25, 0.75], 1),          # weights
    ([48000, 16000], [[0.5, 0.5, 0.0], [0.0, 0.0, 1.0]], [0.375, 0.375, 0.25], 0),
    ([32000, 32000], [[0.5, 0.25, 0.25], [0.0, 0.75, 0.25]], [0.25, 0.5, 0.25], 1),
]
