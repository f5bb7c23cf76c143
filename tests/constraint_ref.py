"""Constrained decoding restated naively. Shared by
test_constraint_ref.py (CPU), test_gpu_constraint_kernel.py and
test_gpu_constraint.py; not a test module itself and needs no GPU.

Choices are brute force over strings, no automaton: a choice expands by the
flags into a set of byte strings (one optional ' ' before it, one optional '.',
'!' or '?' after it, each ASCII letter in either case); a prefix is viable iff
some string starts with it and accepted iff it equals one. A DFA is walked on
its raw [S][256] table.

A row's judgement of the vocabulary is a function state -> (reject(bytes),
eot_rejected): the mask of D15 is built from it token by token."""
import itertools

import numpy as np

import logits_ref as lr

FOLD_CASE, LEADING_SPACE, TRAILING_PUNCT = 1, 2, 4
MAX_STATES = 4096


def _cases(b, fold):
    c = bytes([b])
    if fold and c.isalpha() and b < 128:
        return [c.lower(), c.upper()]
    return [c]


def expand(choices, flags):
    """The set of byte strings the choices accept."""
    out = set()
    for t in choices:
        t = t if isinstance(t, bytes) else t.encode("utf-8")
        heads = [b"", b" "] if flags & LEADING_SPACE else [b""]
        tails = [b"", b".", b"!", b"?"] if flags & TRAILING_PUNCT else [b""]
        for body in itertools.product(*[_cases(b, flags & FOLD_CASE) for b in t]):
            for h in heads:
                for tl in tails:
                    out.add(h + b"".join(body) + tl)
    return out


def member(choices, flags, text):
    """text in expand(choices, flags), without building the set (a long
    choice with FOLD_CASE expands to 2^letters strings): every way of taking
    the optional ' ' and the optional mark off the text, the rest compared
    with each choice byte by byte."""
    def same(a, b):
        if len(a) != len(b):
            return False
        return all(x == y or (flags & FOLD_CASE and x < 128 and y < 128 and
                              bytes([x]).isalpha() and bytes([x]).lower() == bytes([y]).lower())
                   for x, y in zip(a, b))
    heads = [b"", b" "] if flags & LEADING_SPACE else [b""]
    tails = [b"", b".", b"!", b"?"] if flags & TRAILING_PUNCT else [b""]
    for t in choices:
        t = t if isinstance(t, bytes) else t.encode("utf-8")
        for h in heads:
            for tl in tails:
                if len(text) >= len(h) + len(tl) and text.startswith(h) and text.endswith(tl) \
                        and same(text[len(h):len(text) - len(tl)], t):
                    return True
    return False


class Choices:
    """Brute-force judgement of a choice set; a state is the prefix so far
    (None: dead)."""

    def __init__(self, choices, flags):
        self.strings = expand(choices, flags)
        self._tails = {}

    def tails(self, prefix):
        """What may follow the prefix: the rest of every string that starts
        with it (kept per prefix: a vocabulary is judged against one prefix)."""
        if prefix not in self._tails:
            self._tails[prefix] = [s[len(prefix):] for s in self.strings if s.startswith(prefix)]
        return self._tails[prefix]

    def viable(self, prefix):
        return any(s.startswith(prefix) for s in self.strings)

    def accepted(self, prefix):
        return prefix in self.strings

    def next(self, prefix, data):
        if prefix is None:
            return None
        return prefix + data if any(t.startswith(data) for t in self.tails(prefix)) else None

    def dead(self, prefix):
        return prefix is None

    def accepting(self, prefix):
        return prefix is not None and self.accepted(prefix)


class Dfa:
    """A raw table walked byte by byte; a state is its id (0: dead)."""

    def __init__(self, trans, accepting, start):
        self.trans = np.asarray(trans, np.uint16)
        self.acc = np.asarray(accepting, np.uint8)
        self.start = int(start)

    def next(self, s, data):
        for b in data:
            if s == 0:
                break
            s = int(self.trans[s, b])
        return s

    def dead(self, s):
        return s == 0

    def accepting(self, s):
        return bool(self.acc[s])


def accept_all_dfa():
    """One accepting state, every byte loops: rejects only empty tokens."""
    trans = np.zeros((2, 256), np.uint16)
    trans[1, :] = 1
    return trans, np.array([0, 1], np.uint8), 1


def cycle_dfa(words, min_words=0):
    """(word){min_words,}: the words (byte strings, none a prefix of another)
    concatenated at least min_words times. One copy of the words' trie per
    count 0 .. min_words; a whole word leads to the next copy's root (the last
    copy's to its own), and only the last copy's root is accepting."""
    trie = {0: {}}
    ends = set()
    for w in words:
        s = 0
        for i, b in enumerate(w):
            if i == len(w) - 1:
                assert b not in trie[s], "a word is a proper prefix of another"
                ends.add((s, b))
                break
            assert (s, b) not in ends, "a word is a proper prefix of another"
            if b not in trie[s]:
                trie[s][b] = len(trie)
                trie[len(trie)] = {}
            s = trie[s][b]
    n = len(trie)
    S = (min_words + 1) * n + 1
    trans = np.zeros((S, 256), np.uint16)
    for k in range(min_words + 1):
        base = 1 + k * n
        nxt = 1 + min(k + 1, min_words) * n
        for s, edges in trie.items():
            for b, t in edges.items():
                trans[base + s, b] = base + t
        for s, b in ends:
            trans[base + s, b] = nxt
    acc = np.zeros(S, np.uint8)
    acc[1 + min_words * n] = 1
    return trans, acc, 1


def vocab_bytes(ctx):
    """The byte strings of a context's ids below eot. mwx_token_to_str returns
    a C string, so the one single-byte token that is the NUL byte reads as
    empty there: it is put back (ids 0 .. 255 of the synthetic vocabularies are
    the 256 single bytes in GPT-2's order)."""
    toks = ctx.token_bytes(range(ctx.token("eot")))
    nul = [i for i in range(256) if toks[i] == b""]
    assert len(nul) == 1, nul
    toks[nul[0]] = b"\0"
    assert sorted(toks[:256]) == [bytes([b]) for b in range(256)]
    return toks


def rejected(judge, state, tokens, V, eot):
    """[V] bool: D15's rejection of every id for a row in `state`. tokens: the
    byte strings of the ids below eot."""
    rej = np.zeros(V, bool)
    if judge.dead(state):
        return rej
    for t in range(min(eot, V)):
        data = tokens[t]
        rej[t] = len(data) == 0 or judge.dead(judge.next(state, data))
    if eot < V:
        rej[eot] = not judge.accepting(state)
    return rej


def mask_words(rej):
    """[ceil(V / 64)] uint64: bit t % 64 of word t / 64 = rej[t]; zero above V."""
    V = len(rej)
    W = (V + 63) // 64
    bits = np.zeros(W * 64, np.uint64)
    bits[:V] = rej
    sh = np.arange(64, dtype=np.uint64)
    return (bits.reshape(W, 64) << sh).sum(axis=1, dtype=np.uint64)


def unpack(words, V):
    """The inverse of mask_words."""
    w = np.asarray(words, np.uint64)
    sh = np.arange(64, dtype=np.uint64)
    return ((w[:, None] >> sh) & np.uint64(1)).astype(bool).reshape(-1)[:V]


def penalised(x, c, rej, penalty):
    """The filter's y before the kill rules, float32 as the kernel forms it:
    f32(x / T) (or x), then one f32 subtraction where rejected."""
    y = np.array(lr.tempered(x, c), np.float32, copy=True)
    y[rej] = (y[rej] - np.float32(penalty)).astype(np.float32)
    return y


def reference(x, smask, c, lc, rej, penalty, depth=lr.KERNEL_DEPTH):
    """logits_ref.reference of a row whose filter subtracts the penalty from
    the rejected ids: the float64 reference and logits_ref's own bounds on the
    penalised y (which enters the stage exactly where the tempered logit does),
    and the no-speech record of the raw x, which the penalty must not reach."""
    if not (c["active"] and c["sample"]):
        return {"written": False}
    c0 = dict(c)
    c0["temperature"] = 0.0
    c0["want_nosp"] = 0
    r = lr.reference(penalised(x, c, rej, penalty), smask, c0, lc, depth)
    if c["want_nosp"]:
        raw = lr.reference(x, smask, c, lc, depth)
        r["rec"]["nosp"] = raw["rec"]["nosp"]
        r["b_rec"]["nosp"] = raw["b_rec"]["nosp"]
    return r


def settle(x, smask, c, lc, rej, penalty):
    """logits_ref._settle on the penalised row: moves the deciding raw logits
    apart until the reference alone settles every decision."""
    x = np.array(x, np.float32)
    if not (c["active"] and c["sample"]):
        return x
    c0 = dict(c, temperature=0.0, want_nosp=0)
    ts = np.arange(lc.n_vocab) >= lc.beg
    t = np.float32(c["temperature"]) if c["temperature"] > 0 else np.float32(1)
    for _ in range(16):
        r = reference(x, smask, c, lc, rej, penalty)
        try:
            lr.margins(r, penalised(x, c, rej, penalty), c0, lc)
            return x
        except AssertionError as e:
            what = e.args[0][0]
        fin = np.isfinite(r["lp"])
        step = np.float32(max(1.0, 64 * lr.MARGIN * float(r["b_lp"][fin].max()))) * t
        live = ~r["kill"]
        y = penalised(x, c, rej, penalty)
        if what.startswith("top-1"):
            x[r["id"]] += step
        elif what.startswith("timestamp best"):
            x[r["tid"]] += step
        elif what.startswith("timestamp mass"):
            tx = np.nonzero(live & ~ts)[0]
            x[tx[int(y[tx].argmax())]] += 2 * step
        else:
            tsl = np.nonzero(live & ts)[0]
            x[tsl[int(y[tsl].argmax())]] += np.float32(40) * t
    raise AssertionError("input not settled")
