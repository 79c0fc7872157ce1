"""The float64 reference of the encoder's BACKWARD, written out in numpy beside encoder_ref.top_hidden: the LSTM equations
backwards through time, the projection's and the norm's backward (s2:7-35; gate order i, f, g, o).  No autograd here:
tests/test_encoder_grad_cpu.py holds this file to torch's float64 autograd on encoder_ref.torch_modules.  It is the
reference of tests/test_gpu_encoder_train.py and never the code under test.

`params` and the returned gradients are in pack order: per layer weight_ih, weight_hh, bias_ih, bias_hh, then
projection.weight and projection.bias."""
import numpy as np

import encoder_ref as enc


def forward_tape(params, x):
    """Everything the backward reads, float64: per layer (i, f, g, o, c, h), each (R, T, H); x (R, T, I)."""
    layers = (len(params) - 2) // 4
    seq = np.asarray(x, dtype=np.float64)
    R, T, _ = seq.shape
    tape = []
    for l in range(layers):
        w_ih, w_hh, b_ih, b_hh = (np.asarray(p, dtype=np.float64) for p in params[4 * l:4 * l + 4])
        H = w_hh.shape[1]
        h, c = np.zeros((R, H)), np.zeros((R, H))
        planes = [np.empty((R, T, H)) for _ in range(6)]
        for t in range(T):
            z = seq[:, t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh
            i, f, g, o = enc.sigmoid(z[:, :H]), enc.sigmoid(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), enc.sigmoid(z[:, 3 * H:])
            c = f * c + i * g
            h = o * np.tanh(c)
            for plane, v in zip(planes, (i, f, g, o, c, h)):
                plane[:, t] = v
        tape.append(planes)
        seq = planes[5]
    return tape


def encode_grads(params, x, d_out, normalize=True, with_dz=False):
    """The gradients of sum(out * d_out) with respect to every parameter, float64, in pack order; out = encode_ref(params,
    x, normalize).  with_dz: also the list, per layer, of dz (R, T, 4H), the gradient of the pre-activations."""
    layers = (len(params) - 2) // 4
    x = np.asarray(x, dtype=np.float64)
    R, T, _ = x.shape
    wp = np.asarray(params[-2], dtype=np.float64)
    tape = forward_tape(params, x)
    h_top = tape[-1][5][:, T - 1]
    y = h_top @ wp.T + np.asarray(params[-1], dtype=np.float64)
    g_out = np.asarray(d_out, dtype=np.float64)
    if normalize:
        with np.errstate(invalid="ignore", divide="ignore"):
            n = np.linalg.norm(y, axis=1, keepdims=True)
            e = y / n
            dy = (g_out - e * (e * g_out).sum(axis=1, keepdims=True)) / n
    else:
        dy = g_out
    grads = [None] * len(params)
    grads[-2], grads[-1] = dy.T @ h_top, dy.sum(axis=0)
    H = wp.shape[1]
    d_seq = np.zeros((R, T, H))                    # the gradient of the layer's output sequence
    d_seq[:, T - 1] = dy @ wp
    dzs = [None] * layers
    for l in reversed(range(layers)):
        w_ih, w_hh = (np.asarray(p, dtype=np.float64) for p in params[4 * l:4 * l + 2])
        i, f, g, o, c, h = tape[l]
        inp = x if l == 0 else tape[l - 1][5]
        dz = np.empty((R, T, 4 * H))
        dh_rec, dc = np.zeros((R, H)), np.zeros((R, H))
        for t in reversed(range(T)):
            dh = d_seq[:, t] + dh_rec
            tc = np.tanh(c[:, t])
            dc = dc + dh * o[:, t] * (1.0 - tc * tc)
            c_prev = c[:, t - 1] if t > 0 else np.zeros((R, H))
            dz[:, t, :H] = dc * g[:, t] * i[:, t] * (1.0 - i[:, t])
            dz[:, t, H:2 * H] = dc * c_prev * f[:, t] * (1.0 - f[:, t])
            dz[:, t, 2 * H:3 * H] = dc * i[:, t] * (1.0 - g[:, t] ** 2)
            dz[:, t, 3 * H:] = dh * tc * o[:, t] * (1.0 - o[:, t])
            dc = dc * f[:, t]
            dh_rec = dz[:, t] @ w_hh
        h_prev = np.concatenate([np.zeros((R, 1, H)), h[:, :-1]], axis=1)
        flat_dz = dz.reshape(R * T, 4 * H)
        grads[4 * l] = flat_dz.T @ inp.reshape(R * T, -1)
        grads[4 * l + 1] = flat_dz.T @ h_prev.reshape(R * T, H)
        grads[4 * l + 2] = grads[4 * l + 3] = flat_dz.sum(axis=0)
        dzs[l] = dz
        if l > 0:
            d_seq = dz @ w_ih
    return (grads, dzs) if with_dz else grads


def torch_grads(params, x, d_out, dtype, normalize=True):
    """The same from torch's CPU autograd on encoder_ref.torch_modules in `dtype` (float32: the yardstick the gate is
    calibrated on), as float64 numpy arrays in pack order."""
    import torch
    lstm, proj = enc.torch_modules(params, dtype)
    h, _ = lstm(torch.as_tensor(np.asarray(x)).to(dtype))
    y = proj(h[:, h.size(1) - 1])
    if normalize:
        y = y / torch.norm(y, dim=1).unsqueeze(1)
    (y * torch.as_tensor(np.asarray(d_out)).to(dtype)).sum().backward()
    L = (len(params) - 2) // 4
    ps = [getattr(lstm, f"{n}_l{l}") for l in range(L) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return [p.grad.double().numpy() for p in ps + [proj.weight, proj.bias]]


def split_flat(flat, params):
    """A flat gradient buffer -> the list of arrays shaped as `params`."""
    out, off = [], 0
    for p in params:
        n = int(np.prod(np.shape(p)))
        out.append(np.asarray(flat[off:off + n]).reshape(np.shape(p)))
        off += n
    assert off == len(flat)
    return out


def rel_err(a, ref):
    """Relative Frobenius error of one gradient tensor; 0.0 where both are exactly zero."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    den = np.linalg.norm(ref)
    return float(np.linalg.norm(a - ref) / den) if den > 0 else (0.0 if not np.any(a) else float("inf"))


NAMES = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def names(params):
    L = (len(params) - 2) // 4
    return [f"{n}_l{l}" for l in range(L) for n in NAMES] + ["projection.weight", "projection.bias"]
