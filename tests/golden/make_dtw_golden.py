"""Generates tests/golden/dtw_golden.npz: HF transformers' eager
cross-attention probabilities (fp32, CPU) of the seeded `micro` model for a
fixed teacher-forced token list on synthetic clip 0, at the alignment heads
(0, 1), (1, 0), (1, 1), on every 4th encoder frame. The engine's DTW alignment
pass over the same tokens is pinned against it (tests/test_gpu_dtw.py).

Run from the repo root:  python tests/golden/make_dtw_golden.py
Requires libmwx.so (model writer) and oracle/liborc.so (mel), as make_golden.py.
"""
import os

import numpy as np
import torch

from make_golden import OUT, hf_model, mwx, orc, read_ggml

HEADS = [(0, 1), (1, 0), (1, 1)]
# sot | NOT, seven text tokens, EOT (the english-only vocabulary of `micro`)
TOKENS = [50257, 50362, 300, 1234, 777, 40000, 220, 1000, 2000, 50256]
POS0 = 1
FRAME_STEP = 4


def main():
    pcm = mwx.pcm16_to_f32(mwx.synth_pcm16(0))
    path = os.path.join("/tmp", "dtw_golden_micro.bin")
    mwx.write_synthetic_model(path, "micro", mwx.GGML_F16, 0)
    hp, t = read_ggml(path)
    o = orc.Oracle(path, exact=True)
    mel, _ = o.mel(pcm)
    feats = torch.from_numpy(np.ascontiguousarray(mel[:, :3000]))[None]
    orig_gelu = torch.nn.functional.gelu
    torch.nn.functional.gelu = lambda x, approximate="none": orig_gelu(x, approximate="tanh")
    try:
        m = hf_model(hp, t)
        with torch.no_grad():
            enc = m.model.encoder(feats).last_hidden_state
            dec = m.model.decoder(input_ids=torch.tensor([TOKENS]), encoder_hidden_states=enc,
                                  output_attentions=True)
    finally:
        torch.nn.functional.gelu = orig_gelu
    probs = np.stack([dec.cross_attentions[l][0, h].numpy() for l, h in HEADS])   # [A][n][1500]
    probs = probs[:, POS0:]
    assert np.allclose(probs.sum(-1), 1.0, atol=1e-5)
    idx = np.arange(0, probs.shape[-1], FRAME_STEP, dtype=np.int32)
    out = dict(heads=np.array(HEADS, np.int32), tokens=np.array(TOKENS, np.int32),
               pos0=np.int32(POS0), frames=idx, probs=probs[:, :, idx].astype(np.float32))
    np.savez_compressed(os.path.join(OUT, "dtw_golden.npz"), **out)
    o.close()
    os.remove(path)
    print("wrote dtw_golden.npz", probs.shape, "max p", probs.max())


if __name__ == "__main__":
    main()
