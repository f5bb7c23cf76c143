"""Contextual biasing, the rule restated naively: every phrase
and every k is tried against the history; no automaton, no tables.

A phrase is (ids, boost). For a history h (ids generated so far, oldest first)
the matches are all (p, k) with 0 <= k < len(p), k <= len(h) and h[-k:] ==
p[:k] (k = 0 always matches). bias[t] = the largest boost over the matches with
p[k] == t; a token no match points at is absent."""
import numpy as np

MAX_TOKENS = 16
MAX_PHRASES = 1024


def bias_set(phrases, hist):
    """{token: float32 bias} of the history."""
    hist = [int(t) for t in hist]
    out = {}
    for ids, boost in phrases:
        ids = [int(t) for t in ids]
        b = np.float32(boost)
        for k in range(len(ids)):
            if k > len(hist):
                break
            if k and hist[-k:] != ids[:k]:
                continue
            t = ids[k]
            if t not in out or b > out[t]:
                out[t] = b
    return out


def apply(phrases, hist, x):
    """x' = x + bias as one float32 add per boosted token; x [V] float32."""
    y = np.array(x, dtype=np.float32, copy=True)
    for t, b in bias_set(phrases, hist).items():
        y[t] = np.float32(y[t]) + np.float32(b)
    return y


def table_bound(total_tokens):
    """The table size DESIGN.md D14 states (csrc/bias.h bias_table_bound)."""
    return 32 + 20 * total_tokens


def hand_cases():
    """(name, phrases, history, expected {token: bias}) worked by hand."""
    a, b, c, d = 1, 2, 3, 4
    ov = [([a, b, a, c], 1.0), ([b, a, d], 2.0), ([a], 0.5)]
    ts = 50364  # a timestamp id: no phrase can hold it
    return [
        ("empty history", ov, [], {a: 1.0, b: 2.0}),
        ("overlap after a", ov, [a], {a: 1.0, b: 2.0}),
        ("overlap after a b", ov, [a, b], {a: 2.0, b: 2.0}),
        # a b a: phrase 0 at k = 3 (-> c), phrase 1 at k = 2 (-> d), phrase 0 at k = 1 (-> b)
        ("overlap after a b a", ov, [a, b, a], {a: 1.0, b: 2.0, c: 1.0, d: 2.0}),
        ("overlap after a b a c", ov, [a, b, a, c], {a: 1.0, b: 2.0}),
        ("a a a b: after a a", [([a, a, a, b], 3.0)], [a, a], {a: 3.0}),
        ("a a a b: after a a a", [([a, a, a, b], 3.0)], [a, a, a], {a: 3.0, b: 3.0}),
        # a fourth a keeps the k = 3 match alive (h[-3:] == a a a)
        ("a a a b: after a a a a", [([a, a, a, b], 3.0)], [a, a, a, a], {a: 3.0, b: 3.0}),
        ("duplicates, larger boost wins", [([a, b], 1.0), ([a, b], 4.0), ([a, b], 2.0)], [a],
         {a: 4.0, b: 4.0}),
        ("negative and zero boosts", [([a, b], -2.0), ([b], 0.0), ([a, c], -3.0)], [a],
         {a: -2.0, b: 0.0, c: -3.0}),
        ("negative beats more negative", [([a], -2.0), ([a, b], -5.0)], [], {a: -2.0}),
        ("history longer than any phrase", [([a, b, c], 1.5)], [d] * 20 + [a, b], {a: 1.5, c: 1.5}),
        ("a timestamp ends the match", [([a, b, c], 1.5)], [a, b, ts], {a: 1.5}),
        ("a timestamp earlier does not", [([a, b, c], 1.5)], [ts, a, b], {a: 1.5, c: 1.5}),
    ]


def random_case(rng, alphabet=4, max_phrases=12, max_len=6, max_hist=24):
    n = int(rng.integers(1, max_phrases + 1))
    phrases = []
    for _ in range(n):
        ln = int(rng.integers(1, max_len + 1))
        ids = [int(t) for t in rng.integers(0, alphabet, ln)]
        boost = float(np.float32(rng.choice([-3.0, -0.5, 0.0, 0.25, 1.0, 2.5, 7.0])))
        phrases.append((ids, boost))
    hist = [int(t) for t in rng.integers(0, alphabet + 1, int(rng.integers(0, max_hist + 1)))]
    return phrases, hist


def cases(n_random=300, seed=20240914):
    """(name, phrases, history, expected): the hand cases, then seeded random
    phrase sets over a small alphabet (so that overlaps happen), a few with
    phrases of the full MAX_TOKENS."""
    for name, ph, h, want in hand_cases():
        yield name, ph, h, {t: np.float32(b) for t, b in want.items()}
    rng = np.random.default_rng(seed)
    for i in range(n_random):
        if i % 10 == 9:
            ph, h = random_case(rng, alphabet=2, max_phrases=40, max_len=MAX_TOKENS, max_hist=40)
        else:
            ph, h = random_case(rng)
        yield f"random {i}", ph, h, bias_set(ph, h)


def worst_case():
    """MAX_PHRASES phrases of MAX_TOKENS ids, distinct first tokens and, from
    the second id on, a shared run: the root fans out MAX_PHRASES ways and
    every phrase's tail is a prefix-overlap of the others'."""
    return [([1000 + p] + [7] * (MAX_TOKENS - 2) + [p % 5], 1.0 + p % 3) for p in range(MAX_PHRASES)]
