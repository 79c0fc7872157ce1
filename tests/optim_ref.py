"""Oracles of ge2e_sgd_clip_step (include/ge2e_hip.h, OPTIMIZER STEP), numpy only: a plain helper module, no fixtures.

    step         the definition in float64: per-group norm of the scaled gradients, clip_grad_norm_'s coefficient, then
                 torch.optim.SGD (weight decay after the clip, momentum with dampening 0 and a zero-initialised buffer)
    emulate_f32  the update in float32, one rounding per operation, from GIVEN coefficients: what the kernel must store
                 bit for bit once its own coef output is taken as read
    stats_f32    norm -> coef in float32, for the non-finite patterns

Tensors are lists of arrays, `groups[i]` is tensor i's group, `hyper` a (G, 4) array of lr, max_norm, weight_decay, momentum.
"""
import numpy as np

EPS = 1e-6          # clip_grad_norm_ adds it to the norm


def norms(grads, groups, G, grad_scale=1.0):
    """float64 norm of every group's scaled gradients (0 for a group without tensors)."""
    sq = np.zeros(G, np.float64)
    for g, k in zip(grads, groups):
        sq[k] += np.sum((np.asarray(g, np.float64) * np.float64(grad_scale)) ** 2)
    return np.sqrt(sq)


def coefs(norm, max_norm):
    """clip_grad_norm_: max_norm / (norm + 1e-6) clamped from above at 1; a NaN stays (torch.clamp passes it)."""
    norm = np.asarray(norm)
    with np.errstate(all="ignore"):
        c = np.asarray(max_norm, norm.dtype) / (norm + norm.dtype.type(EPS))
        return np.where(c > 1, norm.dtype.type(1), c)


def _update(dtype, coef, params, grads, moms, groups, hyper, grad_scale, zero_grad, skip):
    f = dtype
    hyper = np.asarray(hyper, dtype)
    out_p, out_g, out_m = [], [], []
    with np.errstate(all="ignore"):
        for i, (p, g, k) in enumerate(zip(params, grads, groups)):
            lr, _, wd, mu = hyper[k]
            p, g = np.asarray(p, dtype), np.asarray(g, dtype)
            m = None if moms is None else np.asarray(moms[i], dtype)
            g1 = g * f(grad_scale)
            g2 = g1 * f(coef[k])
            g3 = g2 + wd * p if wd != 0 else g2
            m2 = mu * m + g3 if mu != 0 else g3
            p2 = p - lr * m2
            out_g.append(np.zeros_like(g2) if zero_grad else g2)
            out_p.append(p.copy() if skip else p2)
            if moms is not None:
                out_m.append(m.copy() if skip else m2)
    return out_p, out_g, (out_m if moms is not None else None)


def step(params, grads, moms, groups, hyper, grad_scale=1.0, zero_grad=False, skip_nonfinite=False):
    """One step in float64.  -> dict(params, grads, moms, norm, coef, skipped); `moms` None: no momentum buffer (every
    group's momentum must be 0 then)."""
    hyper = np.asarray(hyper, np.float64)
    G = hyper.shape[0]
    norm = norms(grads, groups, G, grad_scale)
    coef = coefs(norm, hyper[:, 1])
    skip = bool(skip_nonfinite and not np.isfinite(norm).all())
    p, g, m = _update(np.float64, coef, params, grads, moms, groups, hyper, grad_scale, zero_grad, skip)
    return dict(params=p, grads=g, moms=m, norm=norm, coef=coef, skipped=int(skip))


def emulate_f32(coef, params, grads, moms, groups, hyper, grad_scale=1.0, zero_grad=False, skip=False):
    """The update in float32 with every operation rounded on its own (numpy has no fused multiply-add), from the float32
    coefficients `coef` (G,).  -> (params, grads, moms) as float32 arrays."""
    coef = np.asarray(coef, np.float32)
    return _update(np.float32, coef, params, grads, moms, groups, np.asarray(hyper, np.float32), np.float32(grad_scale), zero_grad,
                   skip)


def stats_f32(norm, max_norm):
    """coef from a float32 norm in float32: the kernel's own two operations."""
    return coefs(np.asarray(norm, np.float32), np.asarray(max_norm, np.float32))


def chunk_counts(sizes, chunk=4096):
    return [-(-int(n) // chunk) for n in sizes]
