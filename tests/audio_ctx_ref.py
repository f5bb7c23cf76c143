"""The reference for a short audio context (mwx_full_params.audio_ctx /
audio_ctx_fit), built from the unchanged CPU oracle.

The oracle sizes its encoder, cross K/V and decoder from the model file's
n_audio_ctx: its stem reads 2 * n_audio_ctx mel frames from the window's seek
(zeros past the clip's mel) and the positional-embedding rows 0 .. n_audio_ctx
- 1. So the stage reference for audio_ctx = K is the oracle on M', the model
file rewritten with n_audio_ctx = K and the positional embedding cut to its
first K rows; everything else of the file is copied byte for byte.

The whole pipeline keeps the original model's control flow (20-ms timestamp
tokens, max_initial_ts precision 30 / 1500, seek advance): Oracle(M)
.full_external with its encodes and logits answered by Oracle(M') per window.
"""
import os
import struct

import numpy as np

import orc

PE_NAME = b"encoder.positional_embedding"
N_SAMPLE_RATE = 16000
HOP = 160


def _pe_record(buf: bytes):
    """(offset of the first tensor record, hparams) of a ggml .bin model."""
    magic, = struct.unpack_from("<I", buf, 0)
    assert magic == 0x67676D6C, hex(magic)
    hp = list(struct.unpack_from("<11i", buf, 4))
    off = 4 + 44
    n_mels, n_fft = struct.unpack_from("<2i", buf, off)
    off += 8 + n_mels * n_fft * 4
    n_vocab, = struct.unpack_from("<i", buf, off)
    off += 4
    for _ in range(n_vocab):
        ln, = struct.unpack_from("<I", buf, off)
        off += 4 + ln
    return off, hp


def rewrite_model(src: str, dst: str, K: int) -> str:
    """Writes M' = the model at `src` with n_audio_ctx = K (1 .. its own) and
    the encoder positional embedding truncated to rows 0 .. K - 1."""
    with open(src, "rb") as f:
        buf = f.read()
    off, hp = _pe_record(buf)
    N, d = hp[1], hp[2]
    assert 1 <= K <= N, (K, N)
    nd, nlen, ttype = struct.unpack_from("<3i", buf, off)
    dims = struct.unpack_from(f"<{nd}i", buf, off + 12)
    name = buf[off + 12 + 4 * nd: off + 12 + 4 * nd + nlen]
    # the synthetic writer puts the positional embedding first, f32 [N][d]
    # (dims in ggml order: innermost first)
    assert name == PE_NAME and nd == 2 and ttype == 0 and dims == (d, N), (name, nd, ttype, dims)
    data0 = off + 12 + 4 * nd + nlen
    out = bytearray(buf[:data0])
    struct.pack_into("<i", out, 4 + 4, K)           # hparams: n_audio_ctx
    struct.pack_into("<i", out, off + 12 + 4, K)    # the record's row count
    out += buf[data0: data0 + K * d * 4]
    out += buf[data0 + N * d * 4:]
    with open(dst, "wb") as f:
        f.write(out)
    return dst


def n_len_org(n_samples: int) -> int:
    """Real mel frames of a clip (whisper_pcm_to_mel: 1 + (n + 200 - 400) / 160,
    C integer division)."""
    if n_samples <= 0:
        return 0
    return 1 + int((n_samples + 200 - 400) / HOP)


def audio_ctx_rule(N: int, n_samples: int, seek: int, audio_ctx: int, fit: bool) -> int:
    """mwx_audio_ctx_for restated (include/mwx.h)."""
    a = max(0, audio_ctx)
    if not fit:
        return min(a, N) if a > 0 else N
    rem = max(0, n_len_org(n_samples) - seek)
    floor = a if a > 0 else 64
    half = -(-rem // 2)
    want = 64 * -(-(half + 32) // 64)
    return min(N, max(floor, want))


class CtxOracles:
    """Oracle(M) and, per audio context K, Oracle(M') (made on demand in
    `workdir`); K == n_audio_ctx is M itself."""

    def __init__(self, path: str, workdir: str, mxfp8: bool = False):
        self.path, self.workdir, self.mxfp8 = path, workdir, mxfp8
        self.base = orc.Oracle(path, mxfp8=mxfp8)
        self.N = self.base.hp[1]
        self._by_k = {self.N: self.base}

    def path_for(self, K: int) -> str:
        if K == self.N:
            return self.path
        stem = os.path.splitext(os.path.basename(self.path))[0]
        dst = os.path.join(self.workdir, f"{stem}-ctx{K}.bin")
        if not os.path.exists(dst):
            rewrite_model(self.path, dst, K)
        return dst

    def at(self, K: int) -> orc.Oracle:
        if K not in self._by_k:
            self._by_k[K] = orc.Oracle(self.path_for(K), mxfp8=self.mxfp8)
        return self._by_k[K]

    def full(self, pcm: np.ndarray, opt: orc.FullOptions, audio_ctx: int = 0, fit: bool = False,
             tap=None):
        """The whole pipeline at an audio context: M's full() with every window
        encoded and decoded by the M' of that window's context. tap(seek, K,
        tokens, logits) sees every decoded row. Returns full()'s tuple and the
        list of (seek, K) windows."""
        pcm = np.ascontiguousarray(pcm, np.float32)
        mel, _ = self.base.mel(pcm)
        cur = {}
        windows = []

        def encode_fn(seek):
            K = audio_ctx_rule(self.N, len(pcm), seek, audio_ctx, fit)
            o = self.at(K)
            k, v = o.cross(o.encode(mel, seek))
            cur.update(o=o, k=k, v=v, seek=seek, K=K)
            windows.append((seek, K))

        def logits_fn(tokens):
            lg = cur["o"].decode_seq(cur["k"], cur["v"], tokens)[-1]
            if tap is not None:
                tap(cur["seek"], cur["K"], list(tokens), lg)
            return lg

        return self.base.full_external(pcm, opt, encode_fn, logits_fn), windows
