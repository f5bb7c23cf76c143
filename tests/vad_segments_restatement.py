"""The VAD segment rule (deviation D7; INTEGRATION.md, "VAD speech
segments") in plain Python: Silero's get_speech_timestamps restated, plus this
project's compaction layout and time map. Written from the rule's text, not
from csrc/k_vad.hip; the GPU tests compare the kernels with it as integers.

All positions are Python integers in samples. Probabilities and the two
thresholds are float32 and compared as float32.
"""
from dataclasses import dataclass

import numpy as np

CHUNK = 512
SIL_AT_MAX = 1568  # samples of silence that mark a possible split point
GAP = 1600         # zero samples between two non-adjacent pieces
FLT_MAX = float(np.finfo(np.float32).max)


@dataclass
class Params:
    """mwx_vad_params (whisper_vad_params: same names, same defaults)."""
    threshold: float = 0.5
    min_speech_duration_ms: int = 250
    min_silence_duration_ms: int = 100
    max_speech_duration_s: float = FLT_MAX
    speech_pad_ms: int = 30
    samples_overlap: float = 0.1


def derived(prm):
    thr = np.float32(prm.threshold)
    neg = max(np.float32(thr - np.float32(0.15)), np.float32(0.01))
    pad = 16 * int(prm.speech_pad_ms)
    max_s = float(np.float32(prm.max_speech_duration_s))  # the struct field is a float
    max_speech = int(min(max_s * 16000.0 - 512.0 - 2.0 * pad, float(2 ** 62)))
    return (thr, np.float32(neg), 16 * int(prm.min_speech_duration_ms),
            16 * int(prm.min_silence_duration_ms), pad, max_speech)


def segments(probs, n_samples, prm=None):
    """The public (padded) segments [(s, e), ...] of one clip."""
    prm = prm or Params()
    thr, neg, min_speech, min_sil, pad, max_speech = derived(prm)
    p = np.asarray(probs, np.float32)
    N = int(n_samples)
    out = []
    trig = False
    start = temp_end = prev_end = next_start = 0
    for i in range(len(p)):
        cur = CHUNK * i
        speech = bool(p[i] >= thr)
        if speech and temp_end != 0:
            temp_end = 0
            if next_start < prev_end:
                next_start = cur
        if speech and not trig:
            trig = True
            start = cur
            continue
        if trig and cur - start > max_speech:
            if prev_end > 0:
                out.append([start, prev_end])
                if next_start < prev_end:
                    trig = False
                else:
                    start = next_start
                prev_end = next_start = temp_end = 0
            else:
                out.append([start, cur])
                prev_end = next_start = temp_end = 0
                trig = False
                continue
        if bool(p[i] < neg) and trig:
            if temp_end == 0:
                temp_end = cur
            if cur - temp_end > SIL_AT_MAX:
                prev_end = temp_end
            if cur - temp_end < min_sil:
                continue
            if temp_end - start > min_speech:
                out.append([start, temp_end])
            prev_end = next_start = temp_end = 0
            trig = False
    if trig and N - start > min_speech:
        out.append([start, N])
    m = len(out)
    for k in range(m):
        if k == 0:
            out[0][0] = max(0, out[0][0] - pad)
        if k < m - 1:
            gap = out[k + 1][0] - out[k][1]
            if gap < 2 * pad:
                out[k][1] += gap // 2
                out[k + 1][0] = max(0, out[k + 1][0] - gap // 2)
            else:
                out[k][1] = min(N, out[k][1] + pad)
                out[k + 1][0] = max(0, out[k + 1][0] - pad)
        else:
            out[k][1] = min(N, out[k][1] + pad)
    return [(s, e) for s, e in out]


def pieces(segs, prm=None):
    """([(src, len, dst), ...], compacted length) of the public segments."""
    prm = prm or Params()
    ov = int(np.float32(prm.samples_overlap) * np.float32(16000.0))
    out = []
    c = 0
    m = len(segs)
    for k, (s, e) in enumerate(segs):
        last = k == m - 1
        end = e if last else min(e + ov, segs[k + 1][0])
        out.append((s, end - s, c))
        c += end - s
        if not last and end != segs[k + 1][0]:
            c += GAP
    total = out[-1][2] + out[-1][1] if out else 0
    return out, total


def map_time(pcs, t, is_end):
    """Compacted centiseconds -> original centiseconds."""
    if t < 0 or not pcs:
        return t
    x = 160 * t
    k = 0
    for j, (_, _, dst) in enumerate(pcs):
        if dst <= x:
            k = j
    src, ln, dst = pcs[k]
    if x - dst < ln:
        orig = src + (x - dst)
    elif is_end or k == len(pcs) - 1:
        orig = src + ln
    else:
        orig = pcs[k + 1][0]
    return orig // 160


def compact(pcm, pcs, total):
    """The compacted clip of `pcm` (numpy f32) by the pieces."""
    out = np.zeros(total, np.float32)
    for src, ln, dst in pcs:
        out[dst:dst + ln] = pcm[src:src + ln]
    return out


def runs(*pairs):
    """Probabilities from (value, chunks) runs."""
    return np.concatenate([np.full(n, v, np.float32) for v, n in pairs])


# The table of the rule's definition: name -> (runs, N, Params, segments,
# compacted length, pieces or None).
TABLE = {
    "A": ([(0.1, 40)], 20480, Params(), [], 0, None),
    "B": ([(0.1, 5), (0.9, 7), (0.1, 20)], 16384, Params(), [], 0, None),
    "C": ([(0.1, 5), (0.9, 9), (0.1, 20)], 17408, Params(), [(2080, 7648)], 5568, None),
    "D": ([(0.1, 4), (0.9, 10), (0.1, 3), (0.9, 10), (0.1, 10)], 18844, Params(),
          [(1568, 14304)], 12736, None),
    "E": ([(0.1, 4), (0.9, 10), (0.4, 20), (0.1, 10)], 22528, Params(), [(1568, 17888)], 16320,
          None),
    "F": ([(0.1, 4), (0.9, 10), (0.1, 4), (0.9, 10), (0.1, 10)], 19456,
          Params(speech_pad_ms=80), [(768, 15616)], 14848, None),
    "G": ([(0.1, 3), (0.9, 20)], 11769, Params(), [(1056, 11769)], 10713, None),
    "H": ([(0.9, 12), (0.1, 12)], 12288, Params(), [(0, 6624)], 6624, None),
    "I": ([(0.9, 100)], 51200, Params(max_speech_duration_s=1.0),
          [(0, 15104), (15104, 30464), (30464, 45824), (45824, 51200)], 51200, None),
    "J": ([(0.9, 20), (0.1, 5), (0.9, 30), (0.1, 10)], 33280,
          Params(max_speech_duration_s=1.0, min_silence_duration_ms=200),
          [(0, 10720), (12320, 28128)], 28128, [(0, 12320, 0), (12320, 15808, 12320)]),
    "K": ([(0.1, 2), (0.5, 10), (0.36, 6), (0.1, 6)], 12288, Params(), [(544, 9696)], 9152, None),
    "M": ([(0.1, 10), (0.9, 20), (0.1, 40), (0.9, 20), (0.1, 10)], 51200, Params(),
          [(4640, 15840), (35360, 46560)], 25600, [(4640, 12800, 0), (35360, 11200, 14400)]),
}
# case M's time map: t -> (start-type, end-type)
M_TIME_MAP = {0: (29, 29), 79: (108, 108), 80: (221, 109), 81: (221, 109), 100: (231, 231),
              200: (291, 291)}


def random_case(rng, n_chunks=None):
    """(probs, N, Params): piecewise-constant runs over the values that sit on
    and around the thresholds, random valid parameters."""
    values = np.array([0.05, 0.2, 0.34, 0.36, 0.5, 0.7, 0.95], np.float32)
    n = int(rng.integers(1, 201)) if n_chunks is None else n_chunks
    p = np.empty(n, np.float32)
    i = 0
    while i < n:
        ln = int(rng.integers(1, 25))
        p[i:i + ln] = values[rng.integers(len(values))]
        i += ln
    N = CHUNK * n if rng.integers(2) else CHUNK * (n - 1) + int(rng.integers(1, CHUNK))
    prm = Params(
        threshold=float(rng.choice([0.3, 0.36, 0.5, 0.6, 0.7, 0.9])),
        min_speech_duration_ms=int(rng.choice([0, 32, 100, 250, 500])),
        min_silence_duration_ms=int(rng.choice([0, 32, 100, 200, 400])),
        max_speech_duration_s=float(rng.choice([FLT_MAX, FLT_MAX, 0.05, 0.5, 1.0, 2.5])),
        speech_pad_ms=int(rng.choice([0, 30, 80, 200])),
        samples_overlap=float(rng.choice([0.0, 0.05, 0.1, 0.25])),
    )
    return p, N, prm
