"""Capture the reference encoder's own forward pass on real spectrograms (build container only).

    python tests/golden/make_encoder_golden.py

Imports ``embedding_model_GE2E/s2_model_GE2E_loss_speach_embed.py`` from /root/reference, builds
``ModelGE2ELossSpeachEmbed`` at n_mels 80, hidden 128, 2 layers, embedding 64, gives its LSTM biases small non-zero values
(s2:18-22 zeroes them; the bias path would go unchecked) and runs it on four real utterances x 160 frames of the reference's
``static/spectrograms/m_ge2e/test/sv_1688.npy`` (float64 on disk, values in [0, 0.96]).

Written, data only: ``tests/golden/callers/encoder.npz`` -- the mels, the module's fp32 CPU output and the output of its
``.double()`` copy -- and ``tests/golden/callers/encoder_weights.npz`` -- the module's ``state_dict``.  Two files because the
weights alone are 0.95 MiB and no committed file may pass 1 MiB.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

from embedding_model_GE2E.s2_model_GE2E_loss_speach_embed import ModelGE2ELossSpeachEmbed  # noqa: E402
from utils.dict_to_dot import GetDictWithDotNotation  # noqa: E402


def capture(n_mels=80, hidden=128, layers=2, emb=64, utterances=4, frames=160, seed=31):
    torch.set_num_threads(1)
    hp = GetDictWithDotNotation({
        "general": {"small_err": 1e-6, "device": torch.device("cpu")},
        "audio": {"mel_n_channels": n_mels},
        "m_ge2e": {"model_hidden_size": hidden, "model_embedding_size": emb, "model_num_layers": layers},
    })
    torch.manual_seed(seed)
    model = ModelGE2ELossSpeachEmbed(hp).eval()
    with torch.no_grad():
        for name, param in model.LSTM_stack.named_parameters():
            if "bias" in name:
                torch.nn.init.normal_(param, std=0.1)
    spec = np.load(os.path.join(REF, "static", "spectrograms", "m_ge2e", "test", "sv_1688.npy"))
    mels = np.ascontiguousarray(spec[:utterances, :frames, :n_mels])          # float64, as the file holds them
    assert mels.shape == (utterances, frames, n_mels) and mels.dtype == np.float64
    with torch.no_grad():
        out32 = model(torch.from_numpy(mels)).numpy()                           # s2:28 casts to float32
        out64 = copy.deepcopy(model).double()
        # the reference's forward casts its input with .float(); its double copy is driven statement by statement
        h, _ = out64.LSTM_stack(torch.from_numpy(mels))
        y = out64.projection(h[:, h.size(1) - 1])
        out64 = (y / torch.norm(y, dim=1).unsqueeze(1)).numpy()
    callers = os.path.join(HERE, "callers")
    np.savez(os.path.join(callers, "encoder.npz"), cfg=np.array([n_mels, hidden, layers, emb, utterances, frames, seed]),
             mels=mels, out32=out32, out64=out64)
    np.savez(os.path.join(callers, "encoder_weights.npz"), **{k: v.numpy().copy() for k, v in model.state_dict().items()})
    for f in ("encoder.npz", "encoder_weights.npz"):
        print(f"{f}: {os.path.getsize(os.path.join(callers, f)) / 1024:.0f} KiB")
    print(f"fp32 against fp64: {np.linalg.norm(out32 - out64) / np.linalg.norm(out64):.2e}")


if __name__ == "__main__":
    capture()
