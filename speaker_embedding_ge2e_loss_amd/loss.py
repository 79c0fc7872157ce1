"""Drop-in for the reference's loss module.

Mirrors ``embedding_model_GE2E/s3_loss_function_GE2E.py`` (class ``GE2ELoss``,
s3:6-127): same constructor argument (``hp`` with ``hp.general.device`` and
``hp.general.small_err``), same parameter names/initial values (``w`` = 10,
``b`` = -5, 0-dim fp32 -- s3:16-17, so ``state_dict`` round-trips and s4:35-42's
second SGD param group works), same ``forward(embeddings (N,M,D)) -> scalar`` and
the same static helpers.  The arithmetic runs in libge2e_hip.so.
"""
from __future__ import annotations

import sys

import torch
import torch.nn as nn

from . import functional as GF


class _HPGeneral:
    def __init__(self, device, small_err):
        self.device = device
        self.small_err = small_err


class _HPSection:
    pass


class HParams:
    """Smallest object with the two fields the loss reads (strings/constants.py:31,34), plus an empty ``m_ge2e``
    section for the callers that write into it (``calculate_ERR`` sets ``test_N`` / ``test_M``, s5:17-18)."""

    def __init__(self, device="cuda:0", small_err=1e-6):
        self.general = _HPGeneral(torch.device(device), small_err)
        self.m_ge2e = _HPSection()


class _GraphedLossFunction(torch.autograd.Function):
    """``graph=True``: forward = copy into the static input + one graph replay (graphed.StaticLossStep); backward (only
    reached when somebody differentiates THROUGH the loss -- a plain ``loss.backward()`` takes the shortcut below) scales
    the static gradients by the incoming one, like functional._GE2ELossFunction."""

    @staticmethod
    def forward(ctx, embeddings, w, b, step):
        step.run(embeddings)
        ctx.step, ctx.serial = step, step.serial
        return step.loss1[0].clone()             # (a copy: callers collect the losses of many steps, e.g. DPTrainer.fit)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        step = ctx.step
        if ctx.serial != step.serial:
            raise RuntimeError("GE2ELoss(graph=True): this loss belongs to an earlier forward; its static gradient buffers "
                               "have been overwritten by a later call (use graph=False to keep several losses alive)")
        n, m, d = step.shape
        o = step.out
        return GF._scale_grads(step.dE3, o.dw.data_ptr(), o.db.data_ptr(), grad_out, 1, (1, n, m, d),
                               ctx.needs_input_grad[:3], step.dw0.shape, step.db0.shape) + (None,)


def _has_hooks(t) -> bool:
    return bool(getattr(t, "_backward_hooks", None)) or bool(getattr(t, "_post_accumulate_grad_hooks", None))


def _py_refs(fns, i: int) -> int:
    return sys.getrefcount(fns[i][0])


_free_refs: list = []


def _accumulator_held(loss) -> bool:
    """Whether the Python object of an AccumulateGrad node among the loss's inputs is referenced from anywhere else.  Python
    cannot list a node's hooks, but a hook registered on a tensor's accumulator (``node.register_hook`` /
    ``register_prehook``) lives only as long as that node, and a tensor holds its accumulator weakly: whoever hooks it keeps
    the node object.  (Counted against a fresh accumulator that nobody holds, through the same call.)"""
    if not _free_refs:
        t = torch.zeros((), requires_grad=True)
        _free_refs.append(_py_refs(t.view_as(t).grad_fn.next_functions, 0))
    fns = loss.grad_fn.next_functions
    return any(type(fns[i][0]).__name__ == "AccumulateGrad" and _py_refs(fns, i) > _free_refs[0] for i in range(len(fns)))


def _distributed() -> bool:
    return torch.distributed.is_available() and torch.distributed.is_initialized()


class GE2ELoss(nn.Module):

    def __init__(self, hp, variant: str = "softmax", impl: str = "auto", graph: bool = False):
        """``graph=True`` (not in the reference): the training step of ONE fixed-shape batch per call -- s4:193-205 -- is
        served from a HIP graph over static buffers once the same (N, M, D) has come twice in a row: ``forward`` copies the
        embeddings in and replays the fused launch, and a plain ``loss.backward()`` publishes the launch's own dE / dw / db
        as the gradients without going through the autograd engine (same bits: the engine would multiply them by 1.0).
        The ``.grad`` tensors the shortcut sets are STATIC -- overwritten by the next forward (a ``.grad`` that is still attached
        then is cloned first, so accumulating over several steps stays correct); the returned loss is a copy.  The shortcut keeps
        the eager node's contract: a second ``loss.backward()`` raises unless the first one passed ``retain_graph=True``, and a
        loss that nothing requires grad for raises.  Under ``torch.distributed`` (DistributedDataParallel hooks the parameters'
        AccumulateGrad nodes from C++, where Python cannot see it), or when somebody holds an AccumulateGrad node of ``e``,
        ``w`` or ``b`` at the forward (a hook registered on it), the gradients are published through ONE
        ``torch.autograd.backward`` call on the leaves, which runs every hook.  Still the eager node: another shape, a (B, N, M, D) stack, an input that is not
        float32 (float64 embeddings run the double-precision kernel, eagerly; float16 / bfloat16 the cast route), no-grad mode, a stream
        that is capturing, tensor hooks on ``e`` / ``w`` / ``b`` / the loss, ``backward`` with a gradient / ``inputs`` /
        ``create_graph``, and any gradient that flows THROUGH the loss (``torch.autograd.grad``, ``(2 * loss).backward()``)."""
        super().__init__()
        self.device = hp.general.device  # s3:11
        self.hp = hp  # s3:12
        self.variant = variant
        self.impl = impl
        self.graph = bool(graph)
        self._steps = {}          # key (graphed.StaticLossStep.key_of) -> step; at most _MAX_STEPS, oldest dropped
        self._last_shape = None
        # s3:16-17 -- scale and shift of eq. (5), learnable
        self.w = nn.Parameter(torch.tensor(10.0).to(self.device), requires_grad=True)
        self.b = nn.Parameter(torch.tensor(-5.0).to(self.device), requires_grad=True)

    def forward(self, embeddings, counts=None, labels=None, num_speakers=None, masked=None, return_active=False,
                wide=False):
        """embeddings (N,M,D) [or (B,N,M,D)] on hp.general.device -> loss (s3:19-30).

        Like the reference, w is NOT clamped (s3:22 discards torch.clamp's result), the
        loss is a sum over all (speaker, utterance) rows (s3:126), and the gradient flows
        through both cosine norms.  Like the reference, the loss and the embeddings' gradient come back in the
        embeddings' dtype: float32 and float64 are computed natively (float64 with ``impl="auto"``; ``w.grad`` /
        ``b.grad`` stay fp32 like the parameters), float16 / bfloat16 are computed in fp32.

        ``counts`` (not in the reference, which draws the same M utterances for every speaker): the RAGGED loss.
        ``embeddings`` is then (R, D) [or (B, R, D)], the rows of speaker 0, speaker 1, ... one after the other, and
        ``counts`` their utterance counts -- (N,) or (B, N) on the host, every count >= 2, summing to R -- or a
        ``torch.int32`` device tensor of offsets, unverified (``functional.ge2e_loss_ragged``).  One kernel: ``impl`` must
        be "auto"; float64 raises NotImplementedError.  With ``graph=True`` this route is eager too (nothing is captured).

        ``labels`` (instead of ``counts``): the same loss for rows in ANY order, one speaker label per row -- (R,) or
        (B, R); arbitrary integer ids on the host (validated: at least 2 rows per speaker), or a ``torch.int32`` /
        ``torch.int64`` device tensor of dense ids in [0, ``num_speakers``), unverified, with ``num_speakers`` given
        (``functional.ge2e_loss_labeled``).  The gradient comes back in the caller's row order.  The same conditions:
        ``impl`` "auto", no float64, eager with ``graph=True``.

        ``masked=True`` (with ``labels``): the batch as it is.  ``num_speakers`` is an upper bound of the ids, rows whose
        label is outside [0, ``num_speakers``) -- on the host: negative, e.g. -1 on padding -- are ignored, a speaker left
        with fewer than 2 rows is left out, device labels may hold anything; all decided on the device.
        ``return_active=True`` returns ``(loss, active)``, active (2,) / (B, 2) int32 on the device: the numbers of
        speakers and rows that counted (``functional.ge2e_loss_labeled``).

        ``wide=True`` (with ``labels``): the masked loss -- ``masked`` is implied -- on many workgroups per batch, for few,
        large batches (``functional.loss_fwd_bwd_labeled``).
        """
        if (masked or return_active or wide) and labels is None:
            raise ValueError("masked=True / return_active=True belong to labels=...: pass one speaker label per row")
        if labels is not None:
            if counts is not None:
                raise ValueError("pass counts (rows grouped by speaker) or labels (rows in any order), not both")
            if self.impl != "auto":
                raise ValueError(f'impl="{self.impl}" names a fixed-shape kernel; the ragged loss has one kernel (impl="auto")')
            return GF.ge2e_loss_labeled(embeddings, labels, self.w, self.b, num_speakers=num_speakers,
                                        eps=self.hp.general.small_err, variant=self.variant, masked=masked,
                                        return_active=return_active, wide=wide)
        if counts is not None:
            if self.impl != "auto":
                raise ValueError(f'impl="{self.impl}" names a fixed-shape kernel; the ragged loss has one kernel (impl="auto")')
            return GF.ge2e_loss_ragged(embeddings, counts, self.w, self.b, eps=self.hp.general.small_err,
                                       variant=self.variant)
        if self.graph:
            loss = self._forward_graphed(embeddings)
            if loss is not None:
                return loss
        return GF.ge2e_loss(embeddings, self.w, self.b, eps=self.hp.general.small_err,
                            variant=self.variant, impl=self.impl)

    _MAX_STEPS = 4

    def __getstate__(self):
        # captured graphs and their static buffers belong to THIS object: a copy (copy.deepcopy, pickling, DataParallel's
        # replicate) starts without them and captures its own
        state = self.__dict__.copy()
        state["_steps"] = {}
        state["_last_shape"] = None
        return state

    def _forward_graphed(self, e):
        if (e.dim() != 3 or not e.is_cuda or e.dtype != torch.float32 or not e.is_contiguous() or e.device != self.w.device
                or not torch.is_grad_enabled() or torch.cuda.is_current_stream_capturing()):
            self._last_shape = None
            return None
        from .graphed import StaticLossStep
        key = StaticLossStep.key_of(self, e.shape)
        step = self._steps.get(key)
        if step is None:
            if self._last_shape != key:          # a shape is captured when it comes the second time in a row
                self._last_shape = key
                return None
            while len(self._steps) >= self._MAX_STEPS:
                self._steps.pop(next(iter(self._steps)))
            with torch.no_grad():
                step = self._steps[key] = StaticLossStep(self, e.shape, e.device)
        w, b = self.w, self.b
        # a .grad that still IS one of the static buffers (the caller did not set it to None): keep its value out of the replay's way
        for t in (e, w, b):
            g = t.grad if t.is_leaf else None
            if g is not None and g.data_ptr() in step.static_ptrs:
                t.grad = g.clone()
        loss = _GraphedLossFunction.apply(e, w, b, step)
        serial = step.serial
        import weakref
        wloss = weakref.ref(loss)
        consumed = [False]                       # like the eager node's saved tensors: freed by a backward without retain_graph
        # (decided here: a temporary loss -- mod(e).backward() -- is gone by the time its backward runs)
        req = loss.requires_grad
        engine = req and (_distributed() or _accumulator_held(loss))

        def backward(gradient=None, retain_graph=None, create_graph=False, inputs=None):
            lt = wloss()
            if consumed[0]:
                raise RuntimeError("Trying to backward through the graph a second time: GE2ELoss(graph=True) has already "
                                   "published this loss's gradients (pass retain_graph=True to the first backward)")
            if retain_graph is None:
                retain_graph = create_graph
            if not req:
                raise RuntimeError("element 0 of tensors does not require grad and does not have a grad_fn")
            if (gradient is not None or create_graph or inputs is not None or step.serial != serial
                    or _has_hooks(e) or _has_hooks(w) or _has_hooks(b) or (lt is not None and _has_hooks(lt))):
                torch.Tensor.backward(lt, gradient, retain_graph, create_graph, inputs)
                consumed[0] = not retain_graph
                return
            consumed[0] = not retain_graph
            pub = [(t, g) for t, g in ((w, step.dw0), (b, step.db0), (e, step.dE3)) if t.requires_grad]
            if engine:
                # somebody may have hooked an accumulator -- DistributedDataParallel's reducer does, from C++, where Python cannot
                # see it: the gradients go through the engine, which runs every hook (one call, the encoder's part included)
                torch.autograd.backward([t for t, _ in pub], [g for _, g in pub], retain_graph=retain_graph)
                return
            for t, g in pub:
                if t is e and not e.is_leaf:     # the encoder's graph continues behind the embeddings
                    torch.autograd.backward(e, g, retain_graph=retain_graph)
                elif t.grad is None:
                    t.grad = g
                elif t.grad.data_ptr() == g.data_ptr():
                    t.grad = t.grad + g          # .grad IS the static buffer (retain_graph): keep the buffer's value intact
                else:
                    t.grad.add_(g)

        loss.backward = backward                 # instance attribute: shadows Tensor.backward for this loss only
        return loss

    # eq. (1) -- s3:33-38
    @staticmethod
    def get_centroids(embeddings):
        return GF.centroids(embeddings)

    # eq. (5) cosines -- s3:41-80 (differentiable in both arguments, like the reference's)
    @staticmethod
    def get_cos_sim(embeddings, centroids, hp):
        # like the reference: `centroids` feeds every other-speaker column, the own-speaker column uses the
        # leave-one-out centroid of `embeddings` (s3:44-57, 64-78)
        return GF.cos_sim(embeddings, centroids, eps=hp.general.small_err)

    # eq. (8) -- s3:83-93, dead code in the reference (no caller); kept as an API stub
    @staticmethod
    def get_centroid(embeddings, speaker_num, utterance_num):
        spk = embeddings[speaker_num]
        return (spk.sum(dim=0) - spk[utterance_num]) / (spk.shape[0] - 1)

    # s3:95-112
    @staticmethod
    def get_utterance_centroids(embeddings):
        return GF.utterance_centroids(embeddings)

    # eq. (6) -- s3:114-127: returns (loss, per_embedding_loss (N,M))
    @staticmethod
    def calc_loss(sim_matrix, hp, variant: str = "softmax"):
        return GF.calc_loss(sim_matrix, eps=hp.general.small_err, variant=variant)
