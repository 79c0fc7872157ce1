"""``ClipSGD``: ``clip_grad_norm_`` per parameter group and ``torch.optim.SGD`` as one call of two HIP launches.

The reference's step ends with ``clip_grad_norm_(encoder, 3.0)``, ``clip_grad_norm_(loss, 1.0)``, ``optimizer.step()``
(s4:201-203): about twenty small launches through torch's multi-tensor route, all of them host time behind ``backward()``.
``ClipSGD`` makes them ``functional.sgd_clip_step`` over one flat gradient bucket: the gradients' norm is taken per
*parameter group*, each group has its own ``max_norm``, and the learning rates live in a small device table, so that the
call has no Python float on its way and can be captured in a HIP graph.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import functional as GF

_KEYS = ("lr", "max_norm", "weight_decay", "momentum")


class ClipSGD(torch.optim.Optimizer):
    """SGD (momentum with dampening 0, no Nesterov; weight decay) behind a clip of each group's gradient norm.

    ``params``: parameters or ``param_groups`` dicts as for any torch optimizer, at most 8 groups; CUDA float32 only.
    ``max_norm``: one value, or one per group; a group's dict may carry its own, like ``lr``.  ``math.inf`` never clips.
    ``param_groups[i]["lr"]`` (``max_norm``, ``momentum``, ``weight_decay``) stay the source of truth: ``step()`` compares
    them with what it uploaded last and writes the device table again, without waiting for the device, only when one changed.
    ``flat_grad``: the caller's flat gradient bucket, in which the trainable parameters' gradients lie one behind the other
    in ``param_groups`` order (``DPTrainer.flat_grad``); without it the optimizer makes its own and points every ``.grad``
    into it.  ``grad_scale`` multiplies the gradients before the norms (1 / world size after a summing all-reduce).
    ``skip_nonfinite``: a step whose gradients hold an inf or NaN changes nothing and is counted in ``skipped``.

    After ``step()`` the gradients in the bucket are the clipped ones, as ``clip_grad_norm_`` leaves them; ``stats`` holds
    (norm before the clip, coefficient) per group on the device.  A ``.grad`` that no longer lies in the bucket (set to None
    by a foreign ``zero_grad()``, or replaced) is copied in -- None counts as zero -- and bound again.  ``zero_grad()``
    zeroes the bucket and keeps the views.  The momentum buffer is one flat tensor (``momentum_buffer``), not per-parameter
    ``state``."""

    def __init__(self, params, lr: float, max_norm=math.inf, momentum: float = 0.0, weight_decay: float = 0.0,
                 flat_grad: Optional[torch.Tensor] = None, grad_scale: float = 1.0, skip_nonfinite: bool = False):
        per_group = None
        if isinstance(max_norm, (list, tuple)):
            per_group, max_norm = [float(m) for m in max_norm], math.inf
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("lr, momentum and weight_decay must not be negative")
        super().__init__(params, dict(lr=lr, max_norm=max_norm, momentum=momentum, weight_decay=weight_decay))
        if per_group is not None:
            if len(per_group) != len(self.param_groups):
                raise ValueError(f"{len(per_group)} max_norm values for {len(self.param_groups)} parameter groups")
            for g, m in zip(self.param_groups, per_group):
                g["max_norm"] = m
        self.grad_scale, self.skip_nonfinite = float(grad_scale), bool(skip_nonfinite)
        groups = [[p for p in g["params"] if p.requires_grad] for g in self.param_groups]
        flat = [p for g in groups for p in g]
        if not flat:
            raise ValueError("nothing to train: no parameter requires grad")
        dev = flat[0].device
        for p in flat:
            if not p.is_cuda or p.dtype != torch.float32 or p.device != dev:
                raise ValueError(f"ClipSGD runs HIP kernels on float32 parameters of one GPU (got {p.dtype} on {p.device}); "
                                 "there is no other path")
        offsets, off = [], 0
        for g in groups:
            offsets.append([])
            for p in g:
                offsets[-1].append(off)
                off += p.numel()
        if flat_grad is None:
            flat_grad = torch.zeros(off, dtype=torch.float32, device=dev)
        elif flat_grad.dtype != torch.float32 or flat_grad.device != dev or not flat_grad.is_contiguous() or flat_grad.numel() != off:
            raise ValueError(f"flat_grad must be a contiguous float32 tensor of {off} elements on {dev}")
        self.flat_grad = flat_grad
        self._params = flat
        self._views = [flat_grad[o:o + p.numel()].view(p.shape) for p, o in zip(flat, (o for g in offsets for o in g))]
        self._grad_ptrs = [v.data_ptr() for v in self._views]
        self._bind()
        self.layout = GF.sgd_layout(groups, offsets)
        self.momentum_buffer = None
        self._hyper = torch.zeros(len(groups), 4, dtype=torch.float32, device=dev)
        self._uploaded = None
        self._refresh_hyper()

    def _bind(self) -> None:
        for p, v, ptr in zip(self._params, self._views, self._grad_ptrs):
            g = p.grad
            if g is None:
                v.zero_()
            elif g.data_ptr() == ptr:
                continue
            else:
                v.copy_(g)
            p.grad = v

    def _refresh_hyper(self) -> None:
        host = [[float(g[k]) for k in _KEYS] for g in self.param_groups]
        if host == self._uploaded:
            return
        if any(g[3] != 0.0 for g in host) and self.momentum_buffer is None:
            self.momentum_buffer = torch.zeros_like(self.flat_grad)
        # from pinned memory the copy is queued on the stream and the host goes on; the pinned block is the host
        # allocator's to recycle once the copy has run
        self._hyper.copy_(torch.tensor(host, dtype=torch.float32).pin_memory(), non_blocking=True)
        self._uploaded = host

    @property
    def stats(self) -> torch.Tensor:
        """(G, 2) on the device: each group's gradient norm before the clip and the coefficient of the last step."""
        return self.layout.stats

    @property
    def skipped(self) -> torch.Tensor:
        """int32 (1,) on the device: steps left out by ``skip_nonfinite`` so far."""
        return self.layout.skipped

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._bind()
        self._refresh_hyper()
        GF.sgd_clip_step(self.layout, self.flat_grad, self._hyper, self.momentum_buffer, grad_scale=self.grad_scale,
                         skip_nonfinite=self.skip_nonfinite)
        return loss

    def zero_grad(self, set_to_none: bool = False) -> None:
        """Zero the bucket.  The gradients stay views of it whatever ``set_to_none`` says: a dropped view would make
        autograd allocate a gradient of its own, which the next ``step()`` would have to copy back."""
        self.flat_grad.zero_()
        self._bind()
