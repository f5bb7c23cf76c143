"""CPU restatement of the VAD network ("VAD model") in plain
numpy, reading the weights from a file written by mwx_write_synthetic_vad_model,
plus a pure-Python parser of that file. Shared by test_vad_format.py (CPU) and
test_gpu_vad.py; not a test module itself.

forward(model, pcm, dtype) evaluates the net in `dtype` (np.float64 or
np.float32): the front end is vectorised over chunks, the LSTM runs chunk by
chunk with h = c = 0 at the start.
"""
import struct

import numpy as np

CHUNK, PAD, NFFT, HOP, BINS, HID = 512, 64, 256, 128, 129, 128
ENC_IN = [129, 128, 64, 64]
ENC_OUT = [128, 64, 64, 128]
ENC_STRIDE = [1, 2, 2, 1]
GGML_F32, GGML_F16 = 0, 1

# name -> (shape, ggml type) in file order
TENSORS = [("_model.stft.forward_basis_buffer", (258, 256), GGML_F16)]
for _l in range(4):
    TENSORS.append((f"_model.encoder.{_l}.reparam_conv.weight", (ENC_OUT[_l], ENC_IN[_l], 3),
                    GGML_F16))
    TENSORS.append((f"_model.encoder.{_l}.reparam_conv.bias", (ENC_OUT[_l],), GGML_F32))
TENSORS += [("_model.decoder.rnn.weight_ih", (512, 128), GGML_F32),
            ("_model.decoder.rnn.weight_hh", (512, 128), GGML_F32),
            ("_model.decoder.rnn.bias_ih", (512,), GGML_F32),
            ("_model.decoder.rnn.bias_hh", (512,), GGML_F32),
            ("_model.decoder.decoder.2.weight", (1, 128, 1), GGML_F32),
            ("_model.decoder.decoder.2.bias", (1,), GGML_F32)]


def parse(path):
    """-> dict(magic, type, version, hparams, tensors=[(name, shape, ggml type, array)],
    trailing). Shapes are outermost first (the file stores ggml's order)."""
    b = open(path, "rb").read()
    pos = 0

    def i32(n=1):
        nonlocal pos
        v = struct.unpack_from(f"<{n}i", b, pos)
        pos += 4 * n
        return list(v)

    out = {"magic": b[0:4]}
    pos = 4
    (ln,) = i32()
    out["type"] = b[pos:pos + ln].decode()
    pos += ln
    out["version"] = i32(3)
    hp = {"n_encoder_layers": i32()[0]}
    n = hp["n_encoder_layers"]
    hp["encoder_in"], hp["encoder_out"], hp["kernel"] = i32(n), i32(n), i32(n)
    hp["lstm_input"], hp["lstm_hidden"], hp["final_conv_in"], hp["final_conv_out"] = i32(4)
    out["hparams"] = hp
    tensors = []
    while pos + 12 <= len(b) and len(tensors) < len(TENSORS):
        nd, nlen, ttype = i32(3)
        dims = i32(nd)
        name = b[pos:pos + nlen].decode()
        pos += nlen
        shape = tuple(reversed(dims))
        cnt = int(np.prod(shape))
        dt = np.float32 if ttype == GGML_F32 else np.float16
        arr = np.frombuffer(b, dt, cnt, pos).reshape(shape)
        pos += cnt * arr.itemsize
        tensors.append((name, shape, ttype, arr))
    out["tensors"] = tensors
    out["trailing"] = len(b) - pos
    return out


def load(path):
    """name -> float64 array (f16 widened exactly)."""
    return {name: arr.astype(np.float64) for name, _, _, arr in parse(path)["tensors"]}


def n_chunks(n):
    return (n + CHUNK - 1) // CHUNK


def _sigmoid(x, dt):
    return (dt(1) / (dt(1) + np.exp(-x))).astype(dt)


def forward(model, pcm, dtype=np.float64):
    dt = dtype
    W = {k: v.astype(dt) for k, v in model.items()}
    pcm = np.asarray(pcm, np.float32).astype(dt)
    nch = n_chunks(len(pcm))
    if nch == 0:
        return np.empty(0, dt)
    x = np.zeros(nch * CHUNK, dt)
    x[:len(pcm)] = pcm
    x = x.reshape(nch, CHUNK)
    # reflect padding, edge sample not repeated
    xp = np.concatenate([x[:, PAD:0:-1], x, x[:, CHUNK - 2:CHUNK - 2 - PAD:-1]], axis=1)
    assert xp.shape == (nch, CHUNK + 2 * PAD)
    frames = np.stack([xp[:, HOP * f:HOP * f + NFFT] for f in range(4)], axis=1)  # [n][4][256]
    raw = frames @ W["_model.stft.forward_basis_buffer"].T  # [n][4][258]
    a = np.sqrt(raw[..., :BINS] ** 2 + raw[..., BINS:] ** 2).astype(dt)  # [n][4][129]
    a = a.transpose(0, 2, 1)  # [n][channels][frames]
    for l in range(4):
        w = W[f"_model.encoder.{l}.reparam_conv.weight"]  # [out][in][3]
        bias = W[f"_model.encoder.{l}.reparam_conv.bias"]
        fin = a.shape[2]
        ap = np.zeros((nch, a.shape[1], fin + 2), dt)
        ap[:, :, 1:fin + 1] = a
        fout = (fin - 1) // ENC_STRIDE[l] + 1
        out = np.empty((nch, w.shape[0], fout), dt)
        for f in range(fout):
            win = ap[:, :, f * ENC_STRIDE[l]:f * ENC_STRIDE[l] + 3]  # [n][in][3]
            out[:, :, f] = win.reshape(nch, -1) @ w.reshape(w.shape[0], -1).T + bias
        a = np.maximum(out, dt(0)).astype(dt)
    assert a.shape == (nch, HID, 1)
    xt = a[:, :, 0]
    pre = (xt @ W["_model.decoder.rnn.weight_ih"].T + W["_model.decoder.rnn.bias_ih"]
           + W["_model.decoder.rnn.bias_hh"]).astype(dt)
    whh = W["_model.decoder.rnn.weight_hh"]
    wf = W["_model.decoder.decoder.2.weight"].reshape(HID)
    bf = W["_model.decoder.decoder.2.bias"][0]
    h = np.zeros(HID, dt)
    c = np.zeros(HID, dt)
    probs = np.empty(nch, dt)
    for n in range(nch):
        g = (pre[n] + whh @ h).astype(dt)
        i, f, gg, o = (_sigmoid(g[:HID], dt), _sigmoid(g[HID:2 * HID], dt),
                       np.tanh(g[2 * HID:3 * HID]).astype(dt), _sigmoid(g[3 * HID:], dt))
        c = (f * c + i * gg).astype(dt)
        h = (o * np.tanh(c)).astype(dt)
        probs[n] = _sigmoid(np.asarray(wf @ np.maximum(h, dt(0)) + bf, dt), dt)
    return probs


# ---- the clips the tests share ---------------------------------------------------
def mixed_clip():
    """6 s + 137 samples: 2 s zeros, 2 s of 0.3 * Gaussian noise, 2 s + 137 zeros."""
    rng = np.random.default_rng(20240)
    x = np.zeros(6 * 16000 + 137, np.float32)
    x[32000:64000] = (0.3 * rng.standard_normal(32000)).astype(np.float32)
    return x


def noise_clip(n, seed=1, amp=0.3):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def window_clip():
    """One full 30-s window (938 chunks): noise with a 5-s silent gap."""
    x = noise_clip(480000, seed=7)
    x[10 * 16000:15 * 16000] = 0.0
    return x
