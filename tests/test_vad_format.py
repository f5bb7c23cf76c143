"""The VAD model file and the CPU restatement of the network (no GPU).

The file written by mwx_write_synthetic_vad_model is read back by a
pure-Python parser (vad_restatement.parse); the numpy restatement of the
network (vad_restatement.forward, f64 and f32) must react to its input on the
seed the GPU tests use (the power condition), otherwise their parity bounds
would hold for a net that ignores the audio."""
import numpy as np
import pytest

import mwx
import vad_restatement as vr

SEED = 3  # the seed of every VAD test (chosen so that the conditions below hold)


@pytest.fixture(scope="module")
def vad_path(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("vad") / "ggml-silero-vad.bin")
    mwx.write_synthetic_vad_model(p, SEED)
    return p


def test_file_layout(vad_path):
    f = vr.parse(vad_path)
    assert int.from_bytes(f["magic"], "little") == 0x67676D6C  # "ggml"
    assert f["type"] == "silero-16k"
    assert len(f["version"]) == 3
    assert f["hparams"] == {"n_encoder_layers": 4, "encoder_in": [129, 128, 64, 64],
                            "encoder_out": [128, 64, 64, 128], "kernel": [3, 3, 3, 3],
                            "lstm_input": 128, "lstm_hidden": 128, "final_conv_in": 128,
                            "final_conv_out": 1}
    assert [(n, s, t) for n, s, t, _ in f["tensors"]] == vr.TENSORS
    assert f["trailing"] == 0
    for _, _, _, arr in f["tensors"]:
        assert np.all(np.isfinite(arr.astype(np.float64)))


def test_basis_is_the_hann_windowed_dft(vad_path):
    basis = vr.load(vad_path)["_model.stft.forward_basis_buffer"]
    n = np.arange(256)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * n / 256)
    k = np.arange(129)[:, None]
    want = np.concatenate([np.cos(2 * np.pi * k * n / 256) * win,
                           -np.sin(2 * np.pi * k * n / 256) * win])
    assert basis.shape == (258, 256)
    assert np.max(np.abs(basis - want)) <= 2.0 ** -11  # f16 rounding of values in [-1, 1]


def test_weights_are_within_the_gain_bounds(vad_path):
    m = vr.load(vad_path)
    for l in range(4):
        bound = 2.0 / np.sqrt(vr.ENC_IN[l] * 3)
        for part in ("weight", "bias"):
            a = m[f"_model.encoder.{l}.reparam_conv.{part}"]
            assert np.max(np.abs(a)) <= bound * (1 + 2.0 ** -10)
            assert np.max(np.abs(a)) > 0.5 * bound
    for name, g in (("rnn.weight_ih", 3.0), ("rnn.weight_hh", 3.0), ("rnn.bias_ih", 3.0),
                    ("rnn.bias_hh", 3.0), ("decoder.2.weight", 16.0), ("decoder.2.bias", 16.0)):
        assert np.max(np.abs(m["_model.decoder." + name])) <= g / np.sqrt(128.0)


def test_seed_determines_the_bytes(tmp_path, vad_path):
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    mwx.write_synthetic_vad_model(a, SEED)
    mwx.write_synthetic_vad_model(b, SEED + 1)
    ref = open(vad_path, "rb").read()
    assert open(a, "rb").read() == ref
    other = open(b, "rb").read()
    assert len(other) == len(ref) and other != ref


def test_power_condition_and_noise_floor(vad_path):
    """The net reacts to its input: over the mixed clip (silence, noise,
    silence) the f64 probabilities span at least 0.3. e32, the distance of the
    f32 restatement from the f64 one, is the yardstick of the GPU parity bound."""
    m = vr.load(vad_path)
    clip = vr.mixed_clip()
    assert len(clip) == 6 * 16000 + 137
    p64 = vr.forward(m, clip, np.float64)
    p32 = vr.forward(m, clip, np.float32)
    assert len(p64) == vr.n_chunks(len(clip)) == 188
    assert p32.dtype == np.float32
    span = float(p64.max() - p64.min())
    e32 = float(np.max(np.abs(p32.astype(np.float64) - p64)))
    print(f"span = {span:.4f}, e32 = {e32:.3e}")
    assert span >= 0.3
    assert 0.0 < e32 < 1e-5


def test_gate_threshold_gap(vad_path):
    """The host-gate test needs silence and noise apart: the maxima over a 2-s
    all-zero clip and a 2-s noise clip differ by at least 0.05."""
    m = vr.load(vad_path)
    silent = vr.forward(m, np.zeros(32000, np.float32)).max()
    noise = vr.forward(m, vr.noise_clip(32000)).max()
    print(f"max p: silence {silent:.4f}, noise {noise:.4f}")
    assert noise - silent >= 0.05


def test_chunk_count():
    L = mwx.lib()
    for n, want in ((0, 0), (1, 1), (511, 1), (512, 1), (513, 2), (7 * 512 + 137, 8),
                    (480000, 938)):
        assert L.mwx_vad_n_chunks(n) == want == vr.n_chunks(n)


def _open_fails(path):
    L = mwx.lib()
    v = L.mwx_vad_init_from_file_with_params(path.encode(), L.mwx_vad_default_context_params())
    if v:
        L.mwx_vad_free(v)
    return not v


def test_loader_errors(tmp_path, vad_path):
    """Bad magic, a file cut in the middle of a tensor, a wrong channel count in
    the hyper-parameters, a missing file: NULL (the reader rejects the file
    before any device work, so this needs no GPU)."""
    good = open(vad_path, "rb").read()
    hp0 = 4 + 4 + len("silero-16k") + 12  # magic, type string, version
    cases = {
        "magic": b"ggjt" + good[4:],
        "cut": good[:len(good) // 2],
        "cut-header": good[:hp0 + 10],
        "channels": good[:hp0 + 4] + (130).to_bytes(4, "little") + good[hp0 + 8:],
        "layers": good[:hp0] + (3).to_bytes(4, "little") + good[hp0 + 4:],
        "type": good[:8] + b"silero-08k" + good[18:],
        "trailing": good + b"\0" * 7,
    }
    for name, data in cases.items():
        p = str(tmp_path / f"{name}.bin")
        open(p, "wb").write(data)
        assert _open_fails(p), name
    assert _open_fails(str(tmp_path / "absent.bin"))
    assert mwx.lib().mwx_vad_default_context_params().use_gpu
