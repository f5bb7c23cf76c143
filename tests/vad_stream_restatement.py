"""The online form of the VAD segment rule (deviations D7 and D11;
INTEGRATION.md "Streaming VAD") in plain Python. Written from the rule's text,
not from csrc/k_vad.hip and not from vad_segments_restatement.segments: the
tests compare the three with each other as integers.

The rule reads the probabilities one chunk at a time and closes a segment the
moment it is certain: `step(p)` takes one probability and returns the raw
(unpadded) segments that this chunk closed, each as (start, end, closed_at)
with closed_at = the end of the chunk. `finish(N)` applies the tail rule for
a stream of N samples. Padding needs the next segment's start, so it is a
separate pass over the finished list: `pad(raw, N, prm)`.
"""
import numpy as np

import vad_segments_restatement as sr

CHUNK = sr.CHUNK


class OnlineScan:
    """The scan's registers and one chunk's worth of the rule."""

    def __init__(self, prm=None):
        prm = prm or sr.Params()
        (self.thr, self.neg, self.min_speech, self.min_sil, self.pad,
         self.max_speech) = sr.derived(prm)
        self.reset()

    def reset(self):
        self.i = 0            # chunks seen
        self.triggered = False
        self.start = 0        # where the open speech began
        self.temp_end = 0     # where the current silence began (0: none)
        self.prev_end = 0     # a silence long enough to split at, if the speech gets too long
        self.next_start = 0   # where speech resumed after prev_end
        self.closed = []      # every raw segment so far

    def state(self):
        return (int(self.triggered), self.start, self.temp_end, self.prev_end, self.next_start,
                self.i)

    def _close(self, s, e, at):
        self.closed.append((s, e, at))
        return (s, e, at)

    def step(self, prob):
        """One chunk. Returns the list of segments it closed."""
        p = np.float32(prob)
        cur = CHUNK * self.i
        at = cur + CHUNK
        self.i += 1
        out = []
        is_speech = bool(p >= self.thr)
        is_silence = bool(p < self.neg)
        # speech after a silence that did not end the segment: the silence is over
        if is_speech and self.temp_end != 0:
            self.temp_end = 0
            if self.next_start < self.prev_end:
                self.next_start = cur
        # speech begins
        if is_speech and not self.triggered:
            self.triggered = True
            self.start = cur
            return out
        # the open speech has become too long: cut at the last long silence if
        # there was one, else right here
        if self.triggered and cur - self.start > self.max_speech:
            if self.prev_end > 0:
                out.append(self._close(self.start, self.prev_end, at))
                if self.next_start < self.prev_end:
                    self.triggered = False
                else:
                    self.start = self.next_start
                self.prev_end = self.next_start = self.temp_end = 0
            else:
                out.append(self._close(self.start, cur, at))
                self.prev_end = self.next_start = self.temp_end = 0
                self.triggered = False
                return out
        # silence inside speech
        if is_silence and self.triggered:
            if self.temp_end == 0:
                self.temp_end = cur
            if cur - self.temp_end > sr.SIL_AT_MAX:
                self.prev_end = self.temp_end
            if cur - self.temp_end < self.min_sil:
                return out
            if self.temp_end - self.start > self.min_speech:
                out.append(self._close(self.start, self.temp_end, at))
            self.prev_end = self.next_start = self.temp_end = 0
            self.triggered = False
        return out

    def feed(self, probs):
        """Several chunks; the segments they closed."""
        out = []
        for p in probs:
            out += self.step(p)
        return out

    def finish(self, n_samples):
        """The tail rule: speech still open ends with the audio."""
        N = int(n_samples)
        out = []
        if self.triggered and N - self.start > self.min_speech:
            out.append(self._close(self.start, N, N))
        self.triggered = False
        return out


def raw_segments(probs, n_samples, prm=None, splits=None):
    """[(s, e, closed_at)] of a whole clip, optionally fed in `splits` pieces
    (a list of chunk counts that sums to len(probs))."""
    scan = OnlineScan(prm)
    p = np.asarray(probs, np.float32)
    if splits is None:
        splits = [len(p)]
    assert sum(splits) == len(p)
    at = 0
    for k in splits:
        scan.feed(p[at:at + k])
        at += k
    scan.finish(n_samples)
    return scan.closed


def pad(raw, n_samples, prm=None):
    """Rule D7's padding pass over raw segments [(s, e, ...)]: the public
    segments [(s, e)]."""
    prm = prm or sr.Params()
    padding = sr.derived(prm)[4]
    N = int(n_samples)
    seg = [[r[0], r[1]] for r in raw]
    for k in range(len(seg)):
        if k == 0:
            seg[0][0] = max(0, seg[0][0] - padding)
        if k + 1 < len(seg):
            gap = seg[k + 1][0] - seg[k][1]
            if gap < 2 * padding:
                seg[k][1] += gap // 2
                seg[k + 1][0] = max(0, seg[k + 1][0] - gap // 2)
            else:
                seg[k][1] = min(N, seg[k][1] + padding)
                seg[k + 1][0] = max(0, seg[k + 1][0] - padding)
        else:
            seg[k][1] = min(N, seg[k][1] + padding)
    return [(s, e) for s, e in seg]


def random_splits(rng, n, max_piece=40):
    """Chunk counts (zeros included) that sum to n."""
    out = []
    left = n
    while left > 0:
        k = min(left, int(rng.integers(0, max_piece + 1)))
        out.append(k)
        left -= k
    return out or [0]
