"""The float64 reference of the encoder tests: the LSTM equations, the projection and the norm written out in numpy
(s2:7-35; gate order i, f, g, o as torch lays the [4H] axis out).  No nn.LSTM here: tests/test_encoder_cpu.py holds this
file to torch's modules in float64.

`params` is the list the C ABI's flat buffer concatenates: per layer weight_ih [4H][I], weight_hh [4H][H], bias_ih [4H],
bias_hh [4H]; then projection.weight [D][H] and projection.bias [D]."""
import numpy as np


def sigmoid(z):
    # 1 / (1 + exp(-z)) without overflow warnings: exp of the negative magnitude on both sides
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def top_hidden(params, x):
    """h of the top layer after the last frame: x (R, T, I) float64 -> (R, H)."""
    layers = (len(params) - 2) // 4
    seq = np.asarray(x, dtype=np.float64)
    R, T, _ = seq.shape
    for l in range(layers):
        w_ih, w_hh, b_ih, b_hh = (np.asarray(p, dtype=np.float64) for p in params[4 * l:4 * l + 4])
        H = w_hh.shape[1]
        h = np.zeros((R, H))
        c = np.zeros((R, H))
        out = np.empty((R, T, H))
        for t in range(T):
            z = seq[:, t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh
            i, f, g, o = sigmoid(z[:, :H]), sigmoid(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), sigmoid(z[:, 3 * H:])
            c = f * c + i * g
            h = o * np.tanh(c)
            out[:, t] = h
        seq = out
    return seq[:, T - 1]


def encode_ref(params, x, normalize=True):
    """(R, D) float64: the projection of the last frame's top hidden state, divided by its L2 norm (no epsilon, s2:34: a
    zero row is NaN) unless normalize is False."""
    wp, bp = np.asarray(params[-2], dtype=np.float64), np.asarray(params[-1], dtype=np.float64)
    y = top_hidden(params, x) @ wp.T + bp
    if not normalize:
        return y
    with np.errstate(invalid="ignore", divide="ignore"):
        return y / np.linalg.norm(y, axis=1, keepdims=True)


def random_params(n_mels, H, L, D, seed, scale=1.0):
    """float32 parameters in pack order: xavier-normal-sized weights as s2:18-22 draws them, times `scale`, and small
    non-zero biases, so that the bias path is checked too."""
    rng = np.random.default_rng(seed)
    ps = []
    for l in range(L):
        I = n_mels if l == 0 else H
        ps.append(rng.standard_normal((4 * H, I)) * np.sqrt(2.0 / (4 * H + I)) * scale)
        ps.append(rng.standard_normal((4 * H, H)) * np.sqrt(2.0 / (5 * H)) * scale)
        ps.append(rng.standard_normal(4 * H) * 0.1 * scale)
        ps.append(rng.standard_normal(4 * H) * 0.1 * scale)
    ps.append(rng.uniform(-1, 1, (D, H)) / np.sqrt(H))
    ps.append(rng.uniform(-1, 1, D) / np.sqrt(H))
    return [p.astype(np.float32) for p in ps]


def flat(params):
    return np.concatenate([np.asarray(p, dtype=np.float32).ravel() for p in params])


def torch_modules(params, dtype):
    """nn.LSTM + nn.Linear on the CPU holding `params`, in `dtype`: the library path the gate is calibrated on."""
    import torch
    import torch.nn as nn
    L = (len(params) - 2) // 4
    H, n_mels, D = params[1].shape[1], params[0].shape[1], params[-2].shape[0]
    lstm = nn.LSTM(n_mels, H, num_layers=L, batch_first=True).to(dtype)
    proj = nn.Linear(H, D).to(dtype)
    with torch.no_grad():
        for l in range(L):
            for n, p in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), params[4 * l:4 * l + 4]):
                getattr(lstm, f"{n}_l{l}").copy_(torch.as_tensor(np.asarray(p)).to(dtype))
        proj.weight.copy_(torch.as_tensor(np.asarray(params[-2])).to(dtype))
        proj.bias.copy_(torch.as_tensor(np.asarray(params[-1])).to(dtype))
    return lstm, proj


def torch_encode(params, x, dtype, normalize=True):
    """The library path on the CPU (s2:27-35) in `dtype`, as a float64 numpy array."""
    import torch
    lstm, proj = torch_modules(params, dtype)
    with torch.no_grad():
        h, _ = lstm(torch.as_tensor(np.asarray(x)).to(dtype))
        y = proj(h[:, h.size(1) - 1])
        if normalize:
            y = y / torch.norm(y, dim=1).unsqueeze(1)
    return y.double().numpy()


def rel_err(a, ref):
    """Relative Frobenius error over the batch."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def gate(err_ref):
    """The accuracy gate of the native kernel: 4 x the error of torch's CPU fp32 path against this reference, plus two
    ulps of a unit-vector component."""
    return 4.0 * err_ref + 2.0 ** -22
