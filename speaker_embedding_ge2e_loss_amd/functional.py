"""Tensor-level entry points over the C ABI (include/ge2e_hip.h).

torch is used for device memory, the current stream and autograd plumbing only;
all arithmetic of the hot path runs in libge2e_hip.so.  CPU tensors are rejected:
there is no CPU fallback in the product.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from itertools import accumulate
from typing import NamedTuple, Optional

import torch

from . import _lib

SMALL_ERR = 1e-6  # hp.general.small_err, strings/constants.py:31
EPS_COS = 1e-8    # F.cosine_similarity default eps (s3:57, s3:70)


def _require_cuda(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: the GE2E HIP path needs a ROCm device tensor "
            "(no CPU fallback exists in speaker_embedding_ge2e_loss_amd)")


def _as_batched(e: torch.Tensor, dtype: torch.dtype = torch.float32):
    """(N,M,D) -> view (1,N,M,D); (B,N,M,D) unchanged.  Mirrors s3:49-52: must be contiguous."""
    if e.dim() == 3:
        squeeze = True
    elif e.dim() == 4:
        squeeze = False
    else:
        raise ValueError(f"embeddings must be (N,M,D) or (B,N,M,D), got {tuple(e.shape)}")
    if not e.is_contiguous():
        # the reference calls .view() on the input (s3:49,52), which raises for non-contiguous
        raise RuntimeError("embeddings must be contiguous (the reference uses .view(), s3:49-52)")
    if e.dtype != dtype:
        raise TypeError(f"embeddings must be {str(dtype)[6:]} at this boundary, got {e.dtype}")
    return (e.unsqueeze(0) if squeeze else e), squeeze


def _as_rows(e: torch.Tensor):
    """The embeddings of the row-list entry points: (R,D) -> view (1,R,D); (B,R,D) unchanged.  Returns the batched view,
    whether the batch dimension was added, (B, R, D) and the device."""
    if e.dim() not in (2, 3):
        raise ValueError(f"embeddings must be (R,D) or (B,R,D), got {tuple(e.shape)}")
    if not e.is_contiguous():
        raise RuntimeError("embeddings must be contiguous")
    if e.dtype != torch.float32:
        raise TypeError(f"embeddings must be float32 at this boundary, got {e.dtype}")
    squeeze = e.dim() == 2
    e3 = e.unsqueeze(0) if squeeze else e
    return e3, squeeze, e3.shape, e3.device


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_ptr(t: torch.Tensor) -> int:
    """The raw hipStream_t of torch's current stream on t's device (the C call when this torch has it: 0.3 us against
    5 us for building a torch.cuda.Stream object on every launch)."""
    if _raw_stream is not None:
        idx = t.device.index
        return _raw_stream(idx if idx is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(t.device).cuda_stream


class _on_device:
    """`with torch.cuda.device(dev)` that costs nothing when dev is already current (the usual case: ~5 us of host time
    per call otherwise, on a path whose kernel takes 30 us)."""
    __slots__ = ("idx", "prev")

    def __init__(self, dev: torch.device):
        self.idx = dev.index if dev.index is not None else torch.cuda.current_device()
        self.prev = -1

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.idx:
            self.prev = cur
            torch.cuda.set_device(self.idx)
        return self

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
        return False


def _launch(name: str, dev: torch.device, *args) -> None:
    """One call into libge2e_hip.so with `dev` current: guard, call, check.  The stream is one of `args`, named at the call
    site (`_stream_ptr(t)` asks for t's own device, whichever is current)."""
    with _on_device(dev):
        code = getattr(_lib.load(), name)(*args)
    _lib.check(code, name)


class _LRU(dict):
    """A dict of at most ``cap`` entries whose order is recency: `recent` moves what it finds to the end, `put` drops from
    the front.  (Whether to look at all -- not while a stream is being captured -- is each caller's own question.)"""

    def __init__(self, cap: int):
        super().__init__()
        self.cap = cap

    def recent(self, key):
        hit = self.pop(key, None)
        if hit is not None:
            self[key] = hit
        return hit

    def put(self, key, value):
        self.pop(key, None)
        while len(self) >= self.cap:
            self.pop(next(iter(self)))
        self[key] = value
        return value


# Per-(shape, device) workspace sizes and per-(device, stream) workspace tensors of the module path.  The size depends on
# the device (its CU count), so the query runs with that device current.  A workspace is reused only by launches on the
# SAME stream, which the stream itself serialises; callers that pass `workspace=` are unaffected.
#  * While the current stream is being CAPTURED the cache is neither read nor written: the workspace comes from the
#    allocator, i.e. from the capturing graph's private pool, which lives as long as the graph.  (A cached pointer baked
#    into a graph would dangle as soon as a later, larger eager call on that stream replaced the cache entry, and two
#    graphs captured on torch's one capture stream would share -- and race on -- one workspace.)
#  * The cache holds at most _WS_CACHE_MAX (device, stream) entries, least recently used out first: a process that keeps
#    creating streams does not keep a workspace (with a large launch's fall-back slices) per dead stream forever.  A
#    dropped or outgrown workspace goes back to the caching allocator, which hands a block out again only in the order
#    of the stream it was allocated on -- the launches still using it are ahead in that very stream.
#  * The double-precision kernel, the ragged kernel, its labelled forms, the labelled evaluation call and the backward of
#    its cosines have their own entries (the key tags of _ENTRIES): their workspaces have no control block, so they are never shared with the fp32
#    kernels' workspace, need no initialisation launch, and no `workspace_override` stands in for them.
_WS_CACHE_MAX = 8
_ws_bytes_cache: dict = {}
_ws_cache = _LRU(_WS_CACHE_MAX)
_capturing = getattr(torch.cuda, "is_current_stream_capturing", None)


_ws_override: list = []      # innermost `workspace_override` first


class workspace_override:
    """``with workspace_override(ws):`` -- every loss launch inside that does not name a workspace uses ``ws`` (if it is big
    enough and on the right device).  For a caller that OWNS the lifetime question, e.g. a HIP-graph capture: the
    workspace is allocated and initialised once, outside the capture, lives as long as the object that holds the graph,
    and the captured step has no allocation / initialisation node of its own (graphed.GraphedLossStep)."""

    def __init__(self, ws: torch.Tensor):
        self.ws = ws

    def __enter__(self):
        _ws_override.insert(0, self.ws)
        return self.ws

    def __exit__(self, *exc):
        _ws_override.remove(self.ws)
        return False


class _Entry(NamedTuple):
    """An entry point that takes a cached workspace, and what the workspace cache has to know about it."""
    entry: str                  # the call
    size_query: str             # its workspace-size query: the dense shapes take (B, N, M, D, variant[, impl]), the
    #                             row-list losses (B, N, R, D, variant), the evaluation call (B, N, R, D)
    tag: tuple = ()             # what tells its workspace-cache keys from the dense fp32 loss's
    dense_f32: bool = False     # the dense fp32 loss: `impl` is an argument of both, and the workspace starts with the
    #                             team kernel's control block


# The dense losses by the dtype of the embeddings, the row-list calls by name.
_ENTRIES = {
    torch.float32: _Entry("ge2e_loss_fwd_bwd", "ge2e_workspace_bytes", dense_f32=True),
    torch.float64: _Entry("ge2e_loss_fwd_bwd_f64", "ge2e_workspace_bytes_f64", ("f64",)),
    "ragged": _Entry("ge2e_loss_fwd_bwd_ragged", "ge2e_workspace_bytes_ragged", ("ragged",)),
    "labeled": _Entry("ge2e_loss_fwd_bwd_labeled", "ge2e_workspace_bytes_labeled", ("labeled",)),
    "labeled_masked": _Entry("ge2e_loss_fwd_bwd_labeled_masked", "ge2e_workspace_bytes_labeled_masked", ("labeled_masked",)),
    "labeled_wide": _Entry("ge2e_loss_fwd_bwd_labeled_wide", "ge2e_workspace_bytes_labeled_wide", ("labeled_wide",)),
    "labeled_eval": _Entry("ge2e_cos_sim_labeled", "ge2e_cos_sim_labeled_workspace_bytes", ("labeled_eval",)),
    "labeled_cos_bwd": _Entry("ge2e_cos_sim_labeled_bwd", "ge2e_cos_sim_labeled_bwd_workspace_bytes", ("labeled_cos_bwd",)),
    "enroll": _Entry("ge2e_enroll_accumulate", "ge2e_enroll_workspace_bytes", ("enroll",)),
    "identify": _Entry("ge2e_identify", "ge2e_identify_workspace_bytes", ("identify",)),
    "cohort": _Entry("ge2e_cohort_stats", "ge2e_cohort_stats_workspace_bytes", ("cohort",)),
}


def _workspace_for(lib, dev: torch.device, stream: int, abi: _Entry, query: tuple, dev_idx: int) -> torch.Tensor:
    """The cached workspace of (device, stream) for a call of `abi` whose size query takes `query`."""
    key = query + abi.tag + (dev_idx,)
    need = _ws_bytes_cache.get(key)
    if need is None:
        need = _ws_bytes_cache[key] = int(getattr(lib, abi.size_query)(*query))
    if abi.dense_f32:
        for ws in _ws_override:
            if ws.device == dev and ws.numel() >= need:
                return ws
    if _capturing is not None and _capturing():
        return alloc_workspace(need, dev, init=abi.dense_f32)
    k = (dev_idx, stream) + abi.tag
    ws = _ws_cache.recent(k)
    if ws is None or ws.numel() < need:
        ws = _ws_cache.put(k, alloc_workspace(need, dev, init=abi.dense_f32))
    return ws


def _launch_rows(kind: str, e3: torch.Tensor, query: tuple, workspace: Optional[torch.Tensor], *args) -> None:
    """One row-list call (`kind` of _ENTRIES) into libge2e_hip.so on the current stream of e3's device: guard, stream,
    workspace -- the caller's, or the cached one for the size query's `query` -- call, check.  `args` is the entry's
    argument list up to its trailing (workspace, workspace_bytes, stream)."""
    lib = _lib.load()
    abi = _ENTRIES[kind]
    dev = e3.device
    # (the guard spans the stream read and the workspace lookup -- its size query wants `dev` current, its key wants the
    # stream -- as well as the call)
    with _on_device(dev) as guard:
        stream = _stream_ptr(e3)
        if workspace is None:
            workspace = _workspace_for(lib, dev, stream, abi, query, guard.idx)
        code = getattr(lib, abi.entry)(*args, workspace.data_ptr(), workspace.numel(), stream)
    _lib.check(code, abi.entry)


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def workspace_bytes(B: int, N: int, M: int, D: int, variant: str = "softmax", impl: str = "auto") -> int:
    return int(_lib.load().ge2e_workspace_bytes(B, N, M, D, _lib.VARIANTS[variant], _lib.IMPLS[impl]))


def resolve_impl(B: int, N: int, M: int, D: int, variant: str = "softmax", impl: str = "auto") -> str:
    code = _lib.load().ge2e_resolve_impl(B, N, M, D, _lib.VARIANTS[variant], _lib.IMPLS[impl])
    _lib.check(min(code, 0), "ge2e_resolve_impl")
    return _lib.IMPL_NAMES[code]


def alloc_workspace(nbytes: int, device, init: bool = True) -> torch.Tensor:
    """A workspace tensor with the team kernel's control block written (ge2e_workspace_init: one small launch on the
    current stream, no sync), so that the first call on it already runs the team kernel.  The block is self-cleaning
    afterwards; an uninitialised workspace would also be safe, its first call would merely take the fall-back.
    ``init=False``: the bare tensor, for the kernels whose workspace has no control block."""
    # torch's caching allocator returns >= 512-byte aligned blocks; the library wants 256
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    if init and ws.is_cuda:
        _launch("ge2e_workspace_init", ws.device, ws.data_ptr(), ws.numel(), _stream_ptr(ws))
    return ws


def _check_scalar_params(w: torch.Tensor, b: torch.Tensor, dev: torch.device, dtype: torch.dtype = torch.float32):
    """w and b cross the C ABI as raw device pointers to one fp32 (fp64 on the double-precision entry point) each:
    anything else would be a wild device read."""
    for name, t in (("w", w), ("b", b)):
        _require_cuda(t, name)
        if t.dtype != dtype or t.numel() != 1:
            raise TypeError(f"{name} must be a {str(dtype)[6:]} scalar tensor")
        if t.device != dev:
            raise RuntimeError(f"{name} is on {t.device}, embeddings on {dev}: raw pointers cross the C ABI, all on one device")


def workspace_fallback_count(workspace: torch.Tensor) -> int:
    """Diagnostic (one host sync): how many calls on this workspace were computed by the team kernel's in-call fall-back --
    no team formed, a hand-off timed out beside another stream's kernels, or the control block was not clean -- since
    `alloc_workspace` / `ge2e_workspace_init`.  (TeamCtl.fallbacks, csrc/ge2e_team.hpp: byte 1664 of the workspace.)"""
    return int(workspace[1664:1668].view(torch.int32).item())


@dataclass
class LossOutputs:
    loss: torch.Tensor                  # (B,)
    per: Optional[torch.Tensor]         # (B,N,M)
    dE: Optional[torch.Tensor]          # (B,N,M,D)
    dw: Optional[torch.Tensor]          # (B,)
    db: Optional[torch.Tensor]          # (B,)
    active: Optional[torch.Tensor] = None   # (B,2) int32, loss_fwd_bwd_labeled(masked=True) only: active speakers, active rows


def loss_fwd_bwd(embeddings: torch.Tensor, w: torch.Tensor, b: torch.Tensor, *,
                 eps: float = SMALL_ERR, eps_cos: float = EPS_COS, variant: str = "softmax",
                 impl: str = "auto", need_grad: bool = True, need_per: bool = False,
                 out: Optional[LossOutputs] = None,
                 workspace: Optional[torch.Tensor] = None) -> LossOutputs:
    """One enqueue of ge2e_loss_fwd_bwd on the current stream.  No host sync.

    ``out`` / ``workspace`` let a caller (the benchmark, a CUDA-graph capture) reuse
    buffers; otherwise they come from torch's caching allocator.

    float64 embeddings (with float64 ``w`` / ``b``) go to ge2e_loss_fwd_bwd_f64: computed in double precision, float64
    outputs.  That entry point has one kernel, so ``impl`` must be "auto".
    """
    lib = _lib.load()
    _require_cuda(embeddings, "embeddings")
    dtype = torch.float64 if embeddings.dtype == torch.float64 else torch.float32
    abi = _ENTRIES[dtype]
    if not abi.dense_f32 and impl != "auto":
        raise ValueError(f'impl="{impl}" names a float32 kernel; float64 embeddings have one kernel (impl="auto")')
    e4, _ = _as_batched(embeddings, dtype)
    B, N, M, D = e4.shape
    dev = e4.device
    _check_scalar_params(w, b, dev, dtype)
    if dtype == torch.float64:     # (float32 leaves both checks to the library: GE2E_ERR_ALIGN)
        if e4.data_ptr() % 16:     # a contiguous view at an odd storage offset
            e4 = e4.clone()
        for name, t in (vars(out).items() if out is not None else ()):
            if t is not None and (t.dtype != torch.float64 or not t.is_contiguous() or t.device != dev):
                raise TypeError(f"out.{name} must be a contiguous float64 tensor on {dev}")
    if out is None:
        out = _alloc_outputs(B, N, M, D, dtype, dev, need_grad, need_per)
    query = (B, N, M, D, _lib.VARIANTS[variant]) + ((_lib.IMPLS[impl],) if abi.dense_f32 else ())
    ptr = _ptr
    # (the host-bound hot path: _launch_rows' body inline, without its call and its argument packing; the guard also spans
    # the control-block launch of a new workspace)
    with _on_device(dev) as guard:
        stream = _stream_ptr(e4)
        if workspace is None:
            workspace = _workspace_for(lib, dev, stream, abi, query, guard.idx)
        code = getattr(lib, abi.entry)(
            e4.data_ptr(), B, N, M, D, w.data_ptr(), b.data_ptr(), eps_cos, eps, *query[4:],
            out.loss.data_ptr(), ptr(out.per), ptr(out.dE), ptr(out.dw), ptr(out.db),
            workspace.data_ptr(), workspace.numel(), stream)
    _lib.check(code, abi.entry)
    return out


def _alloc_outputs(B: int, N: int, M: int, D: int, dtype: torch.dtype, dev: torch.device, need_grad: bool,
                   need_per: bool) -> LossOutputs:
    kw = dict(dtype=dtype, device=dev)
    sc = torch.empty(3 if need_grad else 1, B, **kw)  # loss | dw | db in one allocation
    return LossOutputs(
        loss=sc[0],
        per=torch.empty(B, N, M, **kw) if need_per else None,
        dE=torch.empty(B, N, M, D, **kw) if need_grad else None,
        dw=sc[1] if need_grad else None,
        db=sc[2] if need_grad else None)


def _alloc_row_outputs(B: int, R: int, D: int, dev: torch.device, need_grad: bool, need_per: bool,
                       with_active: bool = False) -> LossOutputs:
    """`_alloc_outputs` for a row-list loss: (N, M) flattened to R, float32, and the masked loss's `active`."""
    o = _alloc_outputs(B, 1, R, D, torch.float32, dev, need_grad, need_per)
    return LossOutputs(loss=o.loss, per=o.per.view(B, R) if need_per else None, dE=o.dE.view(B, R, D) if need_grad else None,
                       dw=o.dw, db=o.db, active=torch.empty(B, 2, dtype=torch.int32, device=dev) if with_active else None)


# ---- the ragged loss: every speaker its own utterance count (ge2e_loss_fwd_bwd_ragged, csrc/ge2e_ragged.hip) ---------------

def ragged_offsets(counts, rows: int) -> torch.Tensor:
    """Utterance counts -> the row offsets ge2e_loss_fwd_bwd_ragged reads: a CPU int32 tensor (N+1,) for counts (N,), or
    (B, N+1) for (B, N), with offsets[..., 0] = 0 and offsets[..., N] = rows.  ``counts`` is a sequence or an integer CPU
    tensor.  Raises ValueError when a count is < 2 (a speaker with one utterance has no leave-one-out centroid: the
    reference divides by M - 1 = 0, s3:110-111), when a row of counts does not sum to ``rows``, or when there is no
    speaker.  Needs no GPU."""
    c = counts if torch.is_tensor(counts) else torch.as_tensor(counts)
    if c.dim() not in (1, 2) or c.shape[-1] < 1 or c.numel() < 1:
        raise ValueError(f"counts must be (N,) or (B, N) with N >= 1, got shape {tuple(c.shape)}")
    if c.is_cuda:
        raise TypeError("counts must live on the host (a device tensor is taken as offsets, and only as torch.int32)")
    if c.is_floating_point() or c.is_complex() or c.dtype == torch.bool:
        raise TypeError(f"counts must be integers, got {c.dtype}")
    c = c.to(torch.int64)
    if bool((c < 2).any()):
        raise ValueError("every speaker needs at least 2 utterances (the leave-one-out centroid divides by count - 1)")
    if bool((c.sum(dim=-1) != int(rows)).any()):
        raise ValueError(f"counts must sum to the number of rows ({int(rows)}), got {c.sum(dim=-1).tolist()}")
    if int(rows) >= 2 ** 31:
        raise ValueError("offsets are int32: fewer than 2^31 rows per batch")
    off = torch.zeros(c.shape[:-1] + (c.shape[-1] + 1,), dtype=torch.int32)
    off[..., 1:] = torch.cumsum(c, dim=-1)
    return off


# The last few offset tables uploaded from host counts, most recent last: a training loop that repeats its counts (or
# cycles through a few bucketed layouts) pays the validation and the host-to-device copy once.
_RAGGED_UPLOADS_MAX = 8
_ragged_uploads = _LRU(_RAGGED_UPLOADS_MAX)


def _ragged_offsets_on_device(spec, B: int, R: int, dev: torch.device) -> torch.Tensor:
    """(B, N+1) int32 offsets on `dev` from what the caller gave: a torch.int32 DEVICE tensor is taken as offsets, as is
    -- its contents cannot be validated without a host synchronisation, so they are the caller's word (like a tensor
    `unperm` in normalize_unperm; the kernel clamps what it reads, a broken table gives wrong numbers and no wild
    access).  Anything else is host counts: validated (ragged_offsets), uploaded, and remembered."""
    if torch.is_tensor(spec) and spec.is_cuda:
        if spec.dtype != torch.int32:
            raise TypeError(f"device offsets must be torch.int32, got {spec.dtype} (host counts may be any integer type)")
        if spec.device != dev:
            raise RuntimeError(f"offsets are on {spec.device}, embeddings on {dev}: raw pointers cross the C ABI, all on one device")
        if spec.dim() == 1:
            spec = spec.unsqueeze(0).expand(B, -1)
        if spec.dim() != 2 or spec.shape[0] != B or spec.shape[1] < 2:
            raise ValueError(f"offsets must be (N+1,) or (B, N+1) with B = {B}, got {tuple(spec.shape)}")
        return spec.contiguous()
    off = ragged_offsets(spec, R)
    if off.dim() == 1:
        off = off.unsqueeze(0).expand(B, -1)
    if off.shape[0] != B:
        raise ValueError(f"counts are for {off.shape[0]} batches, embeddings hold {B}")
    off = off.contiguous()
    if _capturing is not None and _capturing():
        return off.to(dev)              # (belongs to the capturing graph's pool: not for anybody else)
    key = (off.numpy().tobytes(), B, str(dev))
    hit = _ragged_uploads.recent(key)
    return hit if hit is not None else _ragged_uploads.put(key, off.to(dev))


def loss_fwd_bwd_ragged(embeddings: torch.Tensor, offsets_or_counts, w: torch.Tensor, b: torch.Tensor, *,
                        eps: float = SMALL_ERR, eps_cos: float = EPS_COS, variant: str = "softmax",
                        need_grad: bool = True, need_per: bool = False, out: Optional[LossOutputs] = None,
                        workspace: Optional[torch.Tensor] = None) -> LossOutputs:
    """One enqueue of ge2e_loss_fwd_bwd_ragged on the current stream.  No host sync (host counts: none after their first use).

    ``embeddings`` (R, D) or (B, R, D) float32: the rows of speaker j contiguously, speaker after speaker.
    ``offsets_or_counts``: host counts (N,) / (B, N) -- a sequence or an integer CPU tensor, validated -- or a torch.int32
    DEVICE tensor of offsets (N+1,) / (B, N+1), taken as is and NOT verified.  Outputs as `loss_fwd_bwd` with (N, M)
    flattened to R: loss (B,), per (B, R), dE (B, R, D), dw (B,), db (B,)."""
    _require_cuda(embeddings, "embeddings")
    e3, _, (B, R, D), dev = _as_rows(embeddings)
    _check_scalar_params(w, b, dev)
    with _on_device(dev):
        off = _ragged_offsets_on_device(offsets_or_counts, B, R, dev)
    N = off.shape[1] - 1
    if out is None:
        out = _alloc_row_outputs(B, R, D, dev, need_grad, need_per)
    query = (B, N, R, D, _lib.VARIANTS[variant])
    _launch_rows("ragged", e3, query, workspace,
                 e3.data_ptr(), off.data_ptr(), B, N, R, D, w.data_ptr(), b.data_ptr(), eps_cos, eps, query[4],
                 out.loss.data_ptr(), _ptr(out.per), _ptr(out.dE), _ptr(out.dw), _ptr(out.db))
    return out


# ---- the ragged loss from speaker labels: rows in any order (ge2e_loss_fwd_bwd_labeled, csrc/ge2e_labels.hip) ---------------

def dense_labels(labels, masked: bool = False):
    """Host speaker ids -> (dense ids, N): a CPU int32 tensor shaped like ``labels`` -- (R,) or (B, R) -- in which every
    batch's ids are replaced by their rank among that batch's distinct ids (ascending: the smallest id becomes 0), and the
    number of distinct speakers N.  ``labels`` is a sequence or an integer CPU tensor of ARBITRARY integers.  Raises
    ValueError for a dtype that is not an integer, a speaker with fewer than 2 rows (it has no leave-one-out centroid;
    the message names the id), and batches that do not all hold the same number of distinct speakers.  Needs no GPU.

    ``masked=True``: ids for the masked loss, which takes the batch as it is.  Negative ids mark rows to ignore and become
    -1; the non-negative ids of every batch are compacted by ascending id; N is the largest number of distinct non-negative
    ids over the batches (at least 1).  A speaker with one row is no error (the kernel leaves it out) and the batches may
    hold different numbers of speakers."""
    t = labels if torch.is_tensor(labels) else torch.as_tensor(labels)
    if t.is_cuda:
        raise TypeError("dense_labels takes host labels (device labels are taken as dense ids already)")
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"labels must be integers, got {t.dtype}")
    if t.dim() not in (1, 2) or t.shape[-1] < 1 or t.numel() < 1:
        raise ValueError(f"labels must be (R,) or (B, R) with R >= 1, got shape {tuple(t.shape)}")
    if t.shape[-1] >= 2 ** 31:
        raise ValueError("row indices are int32: fewer than 2^31 rows per batch")
    t = t.to(torch.int64)
    out = torch.empty(t.shape, dtype=torch.int32)
    if masked:
        n_max = 1
        for row, dst in zip(t.reshape(-1, t.shape[-1]), out.view(-1, t.shape[-1])):
            keep = row >= 0
            ids, inverse = torch.unique(row[keep], sorted=True, return_inverse=True)
            dst.fill_(-1)
            dst[keep] = inverse.to(torch.int32)
            n_max = max(n_max, len(ids))
        return out, int(n_max)
    n_all = None
    for bi, (row, dst) in enumerate(zip(t.reshape(-1, t.shape[-1]), out.view(-1, t.shape[-1]))):
        ids, inverse, counts = torch.unique(row, sorted=True, return_inverse=True, return_counts=True)
        if bool((counts < 2).any()):
            lone = int(ids[counts < 2][0])
            raise ValueError(f"speaker {lone}" + (f" of batch {bi}" if t.dim() == 2 else "") + " has 1 row: every speaker "
                             "needs at least 2 (the leave-one-out centroid divides by count - 1)")
        if n_all is not None and len(ids) != n_all:
            raise ValueError(f"every batch must hold the same number of distinct speakers: batch 0 has {n_all}, "
                             f"batch {bi} has {len(ids)}")
        n_all = len(ids)
        dst.copy_(inverse)
    return out, int(n_all)


# The last few label tables uploaded from the host, most recent last, like _ragged_uploads: key -> (device ids, N).
_label_uploads = _LRU(_RAGGED_UPLOADS_MAX)


def _device_labels(labels: torch.Tensor, num_speakers, masked: bool, what: str = "device labels"):
    """DEVICE labels as they cross the C ABI: (torch.int32 labels, N).  torch.int32 or torch.int64, which a torch op
    narrows -- no synchronisation.  ``masked``: the labels may hold ANY values, so torch.int64 is clamped into
    [-1, N] before it is narrowed: 2**32 + 3 is ignored and not wrapped onto speaker 3."""
    if labels.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what} must be torch.int32 or torch.int64, got {labels.dtype}")
    N = int(num_speakers)
    if N < 1:
        raise ValueError(f"num_speakers must be >= 1, got {N}")
    if masked and labels.dtype == torch.int64:
        labels = labels.clamp(-1, N)
    return labels.to(torch.int32), N


def _labels_on_device(labels, num_speakers, B: int, R: int, dev: torch.device, masked: bool = False):
    """((B, R) int32 dense ids on `dev`, N) from what the caller gave.  A DEVICE tensor (torch.int32, or torch.int64 which
    a torch op narrows -- no synchronisation) is taken as dense ids in [0, num_speakers), as is: its contents cannot be
    validated without a host synchronisation, so they are the caller's word (the index kernel clamps what it reads: broken
    labels give wrong numbers and no wild access), and ``num_speakers`` must be given.  Anything else is host labels of
    arbitrary integer ids: validated and compacted (dense_labels), uploaded, and remembered.
    ``masked``: the labels of the masked loss.  Device labels may hold ANY values and ``num_speakers`` is a bound (rows
    labelled outside [0, num_speakers) are ignored); torch.int64 is clamped into [-1, num_speakers] before it is narrowed,
    so that 2**32 + 3 is ignored and not wrapped onto speaker 3.  Host labels go through dense_labels(masked=True), and a
    ``num_speakers`` given with them is the bound to use, at least their distinct count."""
    if torch.is_tensor(labels) and labels.device.type != "cpu":
        if num_speakers is None:
            raise ValueError("device labels need num_speakers: counting the distinct ids would take a host synchronisation")
        labels, N = _device_labels(labels, num_speakers, masked)
        if labels.device != dev:
            raise RuntimeError(f"labels are on {labels.device}, embeddings on {dev}: raw pointers cross the C ABI, all on one device")
        if labels.dim() == 1:
            labels = labels.unsqueeze(0).expand(B, -1)
        if labels.dim() != 2 or tuple(labels.shape) != (B, R):
            raise ValueError(f"labels must be (R,) or (B, R) with B = {B}, R = {R}, got {tuple(labels.shape)}")
        if not masked and R < 2 * N:
            raise ValueError(f"{N} speakers need at least {2 * N} rows, got {R}")
        return labels.contiguous(), N
    raw = labels if torch.is_tensor(labels) else torch.as_tensor(labels)
    if raw.dim() not in (1, 2) or raw.shape[-1] != R or (raw.dim() == 2 and raw.shape[0] != B):
        raise ValueError(f"labels must be (R,) or (B, R) with B = {B}, R = {R}, got {tuple(raw.shape)}")
    capturing = dev.type == "cuda" and _capturing is not None and _capturing()
    integral = not (raw.is_floating_point() or raw.is_complex() or raw.dtype == torch.bool)
    # (not integral: dense_labels below refuses them, nothing is kept)
    key = (raw.to(torch.int64).contiguous().numpy().tobytes(), tuple(raw.shape), B, str(dev), masked) if integral else None
    hit = None if capturing or key is None else _label_uploads.recent(key)
    if hit is None:
        ids, N = dense_labels(raw, masked=masked)
        if ids.dim() == 1:
            ids = ids.unsqueeze(0).expand(B, -1)
        hit = (ids.contiguous().to(dev), N)
        if capturing:                   # (belongs to the capturing graph's pool: not for anybody else)
            return hit
        _label_uploads.put(key, hit)
    if masked:
        if num_speakers is not None and int(num_speakers) < hit[1]:
            raise ValueError(f"num_speakers = {int(num_speakers)} is a bound: the labels hold {hit[1]} distinct speakers")
        return hit if num_speakers is None else (hit[0], int(num_speakers))
    if num_speakers is not None and int(num_speakers) != hit[1]:
        raise ValueError(f"num_speakers = {int(num_speakers)}, the labels hold {hit[1]} distinct speakers")
    return hit


def _label_index(labels: torch.Tensor, num_speakers: int, masked: bool):
    """Both index calls: (offsets, order) and, ``masked``, (speakers, active) behind them, without the batch dimension for
    1-D labels."""
    _require_cuda(labels, "labels")
    lab, N = _device_labels(labels, num_speakers, masked, what="labels")
    if lab.dim() not in (1, 2) or lab.numel() < 1:
        raise ValueError(f"labels must be (R,) or (B, R) with R >= 1, got {tuple(lab.shape)}")
    lab = lab.contiguous()
    squeeze = lab.dim() == 1
    B, R = (1, lab.shape[0]) if squeeze else lab.shape
    dev = lab.device
    lib = _lib.load()
    entry = "ge2e_label_index_masked" if masked else "ge2e_label_index"
    res = [torch.empty(B, n, dtype=torch.int32, device=dev) for n in ((N + 1, R, N, 2) if masked else (N + 1, R))]
    with _on_device(dev):
        need = int(getattr(lib, entry + "_workspace_bytes")(B, N, R))
        ws = alloc_workspace(need, dev, init=False) if need else None
        code = getattr(lib, entry)(lab.data_ptr(), B, N, R, *(t.data_ptr() for t in res), _ptr(ws), need, _stream_ptr(lab))
    _lib.check(code, entry)
    return tuple(t[0] for t in res) if squeeze else tuple(res)


def label_index(labels: torch.Tensor, num_speakers: int):
    """ge2e_label_index on the current stream, no host sync: DEVICE labels (R,) or (B, R), torch.int32 or torch.int64,
    dense ids in [0, num_speakers) -> (offsets, order), torch.int32 on the device: offsets (N+1,) / (B, N+1) with
    offsets[j] = number of rows with a label < j, and order (R,) / (B, R), the stable argsort of the labels.  Labels
    outside [0, num_speakers) are clamped into it."""
    return _label_index(labels, num_speakers, False)


def label_index_masked(labels: torch.Tensor, num_speakers: int):
    """ge2e_label_index_masked on the current stream, no host sync: DEVICE labels (R,) or (B, R), torch.int32 or
    torch.int64, of ANY content, and ``num_speakers`` = N as a bound -> (offsets, order, speakers, active), torch.int32 on
    the device.  A row counts when 0 <= label < N and at least one more row carries its label.  order (R,) / (B, R): the
    rows that count sorted by (label, index), then all the others by index; offsets (N+1,) / (B, N+1) over the speakers
    that count, numbered by ascending label, and the number of rows that count from there on; speakers (N,) / (B, N): the
    labels of those speakers, then -1; active (2,) / (B, 2): how many speakers and rows count."""
    return _label_index(labels, num_speakers, True)


def _masked_for(masked: Optional[bool], wide: bool) -> bool:
    """``masked`` as the labelled calls use it: None is False, unless ``wide`` implies the masked semantics."""
    if wide and masked is not None and not masked:
        raise ValueError("wide=True implies the masked semantics (the wide route has no unmasked form): drop masked=False")
    return bool(wide or masked)


def loss_fwd_bwd_labeled(embeddings: torch.Tensor, labels, w: torch.Tensor, b: torch.Tensor, *,
                         num_speakers: Optional[int] = None, eps: float = SMALL_ERR, eps_cos: float = EPS_COS,
                         variant: str = "softmax", need_grad: bool = True, need_per: bool = False,
                         out: Optional[LossOutputs] = None, workspace: Optional[torch.Tensor] = None,
                         masked: Optional[bool] = None, wide: bool = False) -> LossOutputs:
    """One enqueue of ge2e_loss_fwd_bwd_labeled on the current stream (two launches: the index kernel, the loss kernel).
    No host sync (host labels: none after their first use).

    ``embeddings`` (R, D) or (B, R, D) float32, rows in ANY order; ``labels`` (R,) / (B, R) names each row's speaker:
    host labels -- a sequence or an integer CPU tensor of arbitrary ids, validated and compacted -- or a DEVICE tensor
    (torch.int32 / torch.int64) of dense ids in [0, num_speakers), taken as is and NOT verified, with ``num_speakers``
    given.  Outputs as `loss_fwd_bwd_ragged`, per (B, R) and dE (B, R, D) in the caller's row order.

    ``masked=True``: ge2e_loss_fwd_bwd_labeled_masked, which takes the batch as it is.  ``num_speakers`` is a bound, rows
    labelled outside [0, num_speakers) are ignored (host labels: negative ids), a speaker with fewer than 2 such rows is
    left out, all decided on the device.  per and dE are 0 on the rows that do not count, and ``out.active`` (B, 2) int32
    receives the numbers of speakers and rows that do (allocated here unless ``out`` is given, where it may be None).

    ``wide=True``: ge2e_loss_fwd_bwd_labeled_wide, the masked loss (``masked`` is implied; ``masked=False`` beside it is a
    ValueError) as a chain of many-workgroup kernels, seven launches with a gradient and four without: a single large
    batch spreads over the chip where the masked entry keeps it on one workgroup.  The same outputs, held to the same
    reference, with low bits of their own; its workspace grows with B (one (R, N) matrix per batch), so the masked entry
    stays the choice for many small batches.  Nothing chooses between the two."""
    masked = _masked_for(masked, wide)
    _require_cuda(embeddings, "embeddings")
    e3, _, (B, R, D), dev = _as_rows(embeddings)
    _check_scalar_params(w, b, dev)
    with _on_device(dev):
        lab, N = _labels_on_device(labels, num_speakers, B, R, dev, masked)
    if out is None:
        out = _alloc_row_outputs(B, R, D, dev, need_grad, need_per, with_active=masked)
    query = (B, N, R, D, _lib.VARIANTS[variant])
    if masked and out.active is not None and (out.active.dtype != torch.int32 or not out.active.is_contiguous()
                                              or out.active.device != dev or out.active.numel() != 2 * B):
        raise TypeError(f"out.active must be a contiguous int32 tensor of shape ({B}, 2) on {dev}")
    _launch_rows("labeled_wide" if wide else "labeled_masked" if masked else "labeled", e3, query, workspace,
                 e3.data_ptr(), lab.data_ptr(), B, N, R, D, w.data_ptr(), b.data_ptr(), eps_cos, eps, query[4],
                 out.loss.data_ptr(), _ptr(out.per), _ptr(out.dE), _ptr(out.dw), _ptr(out.db),
                 *((_ptr(out.active),) if masked else ()))
    return out


# ---- labelled evaluation: cosines and EER counts for rows in any order (ge2e_cos_sim_labeled, csrc/ge2e_labeled_eval.hip) ----

@dataclass
class LabeledCosOutputs:
    cos: Optional[torch.Tensor]         # (B, R, N) float32: column k = compact speaker k; 0 on rows / columns that do not count
    col: torch.Tensor                   # (B, R) int32: the row's own column, -1 for a row that does not count
    speakers: torch.Tensor              # (B, N) int32: the label of compact speaker k, then -1
    active: torch.Tensor                # (B, 2) int32: speakers and rows that count
    counts: Optional[torch.Tensor]      # (B, T, 2) int32: [false accepts, own accepts] per threshold


def _threshold_table(thresholds, dev: torch.device, device_ok: bool = False) -> torch.Tensor:
    """`eer_counts`'s check: 1..4096 non-decreasing values, compared in fp32.  ``device_ok``: a float32 DEVICE tensor is
    taken as it is -- reading it would take a host synchronisation, so its order is the caller's word (no upload: fit for
    a graph capture)."""
    if device_ok and torch.is_tensor(thresholds) and thresholds.device.type != "cpu":
        if thresholds.dtype != torch.float32 or thresholds.device != dev or not 1 <= thresholds.numel() <= 4096:
            raise TypeError(f"device thresholds must be 1..4096 torch.float32 values on {dev}")
        return thresholds.reshape(-1).contiguous()
    thr = torch.as_tensor(thresholds, dtype=torch.float64).to(torch.float32).reshape(-1)
    if thr.numel() < 1 or thr.numel() > 4096 or bool((thr[1:] < thr[:-1]).any()):
        raise ValueError("thresholds must be 1..4096 non-decreasing values")
    return thr.to(dev)


def _cos_sim_labeled_run(e3: torch.Tensor, lab: torch.Tensor, N: int, thr: Optional[torch.Tensor], need_cos: bool,
                         eps: float, eps_cos: float, workspace: Optional[torch.Tensor]) -> LabeledCosOutputs:
    """The enqueue of ge2e_cos_sim_labeled on a batched e3 with labels that are on the device already."""
    B, R, D = e3.shape
    dev = e3.device
    T = thr.numel() if thr is not None else 0
    i32 = dict(dtype=torch.int32, device=dev)
    out = LabeledCosOutputs(
        cos=torch.empty(B, R, N, dtype=torch.float32, device=dev) if need_cos else None,
        col=torch.empty(B, R, **i32), speakers=torch.empty(B, N, **i32), active=torch.empty(B, 2, **i32),
        counts=torch.empty(B, T, 2, **i32) if T else None)
    _launch_rows("labeled_eval", e3, (B, N, R, D), workspace,
                 e3.data_ptr(), lab.data_ptr(), B, N, R, D, eps_cos, eps, _ptr(thr), T, _ptr(out.cos), out.col.data_ptr(),
                 out.speakers.data_ptr(), out.active.data_ptr(), _ptr(out.counts))
    return out


class _CosSimLabeledFunction(torch.autograd.Function):
    """The labelled cosines with a backward: ge2e_cos_sim_labeled, then ge2e_cos_sim_labeled_bwd on the saved embeddings
    and device labels (the call is stateless: it builds its own index and centroids and recomputes the cosines)."""

    @staticmethod
    def forward(ctx, e3, lab, N, thr, eps, eps_cos, workspace):
        out = _cos_sim_labeled_run(e3, lab, N, thr, True, eps, eps_cos, workspace)
        ctx.save_for_backward(e3, lab)
        ctx.N, ctx.eps_cos = N, eps_cos
        ctx.set_materialize_grads(False)        # (no zero tensors made for the integer outputs, or for an unused cos)
        plain = tuple(t for t in (out.col, out.speakers, out.active, out.counts) if t is not None)
        ctx.mark_non_differentiable(*plain)
        return out.cos, out.col, out.speakers, out.active, out.counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        if g is None:
            return (None,) * 7
        e3, lab = ctx.saved_tensors
        B, R, D = e3.shape
        g = g.contiguous().float()
        dE = torch.empty_like(e3)
        _launch_rows("labeled_cos_bwd", e3, (B, ctx.N, R, D), None,
                     e3.data_ptr(), lab.data_ptr(), g.data_ptr(), B, ctx.N, R, D, ctx.eps_cos, dE.data_ptr(), None)
        return dE, None, None, None, None, None, None


def cos_sim_labeled(embeddings: torch.Tensor, labels, *, num_speakers: Optional[int] = None, eps: float = SMALL_ERR,
                    eps_cos: float = EPS_COS, thresholds=None, need_cos: bool = True,
                    workspace: Optional[torch.Tensor] = None, differentiable: bool = False) -> LabeledCosOutputs:
    """One enqueue of ge2e_cos_sim_labeled on the current stream (three launches: index, centroids, rows).  No host sync
    (host labels: none after their first use).  By default FORWARD ONLY: no result requires grad and nothing is recorded
    for autograd.  ``differentiable=True`` records ``cos`` for autograd: its backward is ge2e_cos_sim_labeled_bwd (six
    launches on the current stream, dL/dE through the row, the other speakers' centroids and the leave-one-out centroid),
    so a head of the caller's own can stand between these cosines and `calc_loss_labeled`, or any other torch code;
    ``col``, ``speakers``, ``active`` and ``counts`` stay plain tensors, and ``need_cos=False`` beside it is a ValueError.
    `ge2e_loss_labeled` remains the one-call route to the reference's loss.

    ``embeddings`` (R, D) or (B, R, D) float32, rows in ANY order; ``labels`` as `loss_fwd_bwd_labeled(masked=True)` takes
    them: host labels of arbitrary ids (negative: ignore the row), compacted, or a DEVICE tensor (torch.int32 /
    torch.int64) taken as it is with ``num_speakers`` = N as a bound.  The masked loss's semantics: a row counts when
    0 <= label < N and at least one more row carries its label.  Returns, for 2-D input without the batch dimension:
    ``cos`` (R, N) -- column k is the k-th counting speaker by ascending label (``speakers[k]`` names it; with every speaker
    counting a column is a label), the own column holds the leave-one-out cosine, + eps everywhere, 0 on every row and
    column that does not count (None with ``need_cos=False``: the matrix is never materialised) -- ``col`` (R,),
    ``speakers`` (N,), ``active`` (2,), and with ``thresholds`` (non-decreasing, at most 4096: a sequence, checked and
    uploaded, or a float32 DEVICE tensor taken as it is) ``counts`` (T, 2): the calculate_ERR sweep on cos itself."""
    if differentiable and not need_cos:
        raise ValueError("differentiable=True is about cos: need_cos=False beside it leaves nothing to differentiate")
    _require_cuda(embeddings, "embeddings")
    e3, squeeze, (B, R, D), dev = _as_rows(embeddings if differentiable else embeddings.detach())
    if thresholds is None and not need_cos:
        raise ValueError("nothing to compute: need_cos=False without thresholds")
    with _on_device(dev):
        lab, N = _labels_on_device(labels, num_speakers, B, R, dev, True)
        thr = _threshold_table(thresholds, dev, device_ok=True) if thresholds is not None else None
    if differentiable:
        out = LabeledCosOutputs(*_CosSimLabeledFunction.apply(e3, lab, N, thr, float(eps), float(eps_cos), workspace))
    else:
        out = _cos_sim_labeled_run(e3, lab, N, thr, need_cos, eps, eps_cos, workspace)
    if squeeze:
        out = LabeledCosOutputs(*(t[0] if t is not None else None
                                  for t in (out.cos, out.col, out.speakers, out.active, out.counts)))
    return out


def eer_counts_labeled(sim: torch.Tensor, col: torch.Tensor, active: torch.Tensor, thresholds) -> torch.Tensor:
    """ge2e_eer_counts_labeled: the calculate_ERR sweep on a caller-made ``sim`` (R, N) / (B, R, N) -- e.g. w * cos + b --
    with the ``col`` and ``active`` `cos_sim_labeled` returned -> int32 (T, 2) / (B, T, 2).  Rows with col < 0 and columns
    >= active[0] are never read.  ``thresholds``: `eer_counts`'s check (non-decreasing, else ValueError); a float32 DEVICE
    tensor is taken as it is, as in `cos_sim_labeled`."""
    _require_cuda(sim, "sim")
    squeeze = sim.dim() == 2
    s = sim.unsqueeze(0) if squeeze else sim
    if s.dim() != 3:
        raise ValueError(f"sim must be (R,N) or (B,R,N), got {tuple(sim.shape)}")
    s = s.detach().contiguous().float()
    B, R, N = s.shape
    dev = s.device
    for name, t, n in (("col", col, B * R), ("active", active, B * 2)):
        _require_cuda(t, name)
        if t.dtype != torch.int32 or t.numel() != n or t.device != dev:
            raise TypeError(f"{name} must be a torch.int32 tensor of {n} elements on {dev}")
    thr = _threshold_table(thresholds, dev, device_ok=True)
    T = thr.numel()
    counts = torch.empty(B, T, 2, dtype=torch.int32, device=dev)
    _launch("ge2e_eer_counts_labeled", dev, s.data_ptr(), col.contiguous().data_ptr(), active.contiguous().data_ptr(), B, N,
            R, thr.data_ptr(), T, counts.data_ptr(), _stream_ptr(s))
    return counts[0] if squeeze else counts


def _check_col_active(sim: torch.Tensor, col: torch.Tensor, active: torch.Tensor, B: int, R: int) -> None:
    """``col`` and ``active`` as `cos_sim_labeled` returned them: torch.int32 of B R and 2 B elements (asked first: no
    device is needed to say so), then everything on sim's ROCm device."""
    for name, t, n in (("col", col, B * R), ("active", active, B * 2)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.numel() != n:
            raise TypeError(f"{name} must be a torch.int32 tensor of {n} elements, as cos_sim_labeled returned it")
    for name, t in (("sim", sim), ("col", col), ("active", active)):
        _require_cuda(t, name)
        if t.device != sim.device:
            raise TypeError(f"{name} is on {t.device}, sim on {sim.device}")


class _CalcLossLabeledFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s3, col, active, eps, variant):
        B, R, N = s3.shape
        loss = torch.empty(B, dtype=torch.float32, device=s3.device)
        per = torch.empty(B, R, dtype=torch.float32, device=s3.device)
        _launch("ge2e_calc_loss_labeled", s3.device, s3.data_ptr(), col.data_ptr(), active.data_ptr(), B, N, R, eps,
                _lib.VARIANTS[variant], loss.data_ptr(), per.data_ptr(), _stream_ptr(s3))
        ctx.save_for_backward(s3, col, active)
        ctx.eps, ctx.variant = eps, variant
        ctx.set_materialize_grads(False)        # (an output nobody used arrives as None and crosses the ABI as NULL)
        return loss, per

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, g_per):
        if g_loss is None and g_per is None:
            return (None,) * 5
        s3, col, active = ctx.saved_tensors
        B, R, N = s3.shape
        gl = g_loss.contiguous().float() if g_loss is not None else None
        gp = g_per.contiguous().float() if g_per is not None else None
        dS = torch.empty_like(s3)
        _launch("ge2e_calc_loss_labeled_bwd", s3.device, s3.data_ptr(), col.data_ptr(), active.data_ptr(), B, N, R, ctx.eps,
                _lib.VARIANTS[ctx.variant], _ptr(gl), _ptr(gp), dS.data_ptr(), _stream_ptr(s3))
        return dS, None, None, None, None


def calc_loss_labeled(sim: torch.Tensor, col: torch.Tensor, active: torch.Tensor, *, eps: float = SMALL_ERR,
                      variant: str = "softmax"):
    """ge2e_calc_loss_labeled: calc_loss on a caller-made ``sim`` (R, N) / (B, R, N) -- e.g. w * cos + b -- with the ``col``
    and ``active`` `cos_sim_labeled` returned -> (loss () / (B,), per_row_loss (R,) / (B, R)), differentiable in ``sim``
    (ge2e_calc_loss_labeled_bwd).  A row counts when 0 <= col < active[0]; per_row_loss and the gradient are 0 on the other
    rows and on the columns >= active[0], none of which is read.  loss is the batch's sum of per_row_loss."""
    if variant not in _lib.VARIANTS:
        raise ValueError(f"variant must be one of {sorted(_lib.VARIANTS)}, got {variant!r}")
    if not torch.is_tensor(sim) or sim.dim() not in (2, 3):
        raise ValueError(f"sim must be a tensor (R,N) or (B,R,N), got {tuple(sim.shape) if torch.is_tensor(sim) else type(sim).__name__}")
    squeeze = sim.dim() == 2
    s = sim.unsqueeze(0) if squeeze else sim
    B, R, N = s.shape
    _check_col_active(s, col, active, B, R)
    loss, per = _CalcLossLabeledFunction.apply(s.contiguous().float(), col.contiguous(), active.contiguous(), float(eps),
                                               variant)
    return (loss[0], per[0]) if squeeze else (loss, per)


# ---- enrolment and verification: a speaker bank and held-out trials (csrc/ge2e_enroll.hip) --------------------------------

@dataclass
class VerifyOutputs:
    scores: Optional[torch.Tensor]      # (R, K) float32: 0 on ignored rows and on speakers that are not enrolled
    counts: Optional[torch.Tensor]      # (T, 2) int32: [impostor accepts, target accepts] per threshold
    trials: Optional[torch.Tensor]      # (2,) int32: impostor and target scores counted (the denominators of FAR and FRR)


def _bank_rows(embeddings: torch.Tensor, D: int, dev: torch.device) -> torch.Tensor:
    _require_cuda(embeddings, "embeddings")
    e = embeddings.detach()
    if e.dim() != 2 or e.shape[0] < 1 or e.shape[1] != D:
        raise ValueError(f"embeddings must be (R, {D}) with R >= 1, got {tuple(e.shape)}")
    if e.dtype != torch.float32 or not e.is_contiguous() or e.device != dev:
        raise TypeError(f"embeddings must be contiguous torch.float32 on {dev}")
    return e


def _bank_labels(labels, K: int, R: int, dev: torch.device) -> torch.Tensor:
    """(R,) int32 bank indices on `dev`.  A device tensor (torch.int32 / torch.int64) is taken as it is; a host sequence of
    ints is copied, NOT compacted: the ids are bank indices.  64-bit ids are clamped into [-1, K] before they are narrowed,
    so that 2**32 + 3 stays outside the bank."""
    if torch.is_tensor(labels) and labels.device.type != "cpu":
        if labels.device != dev:
            raise RuntimeError(f"labels are on {labels.device}, the bank on {dev}: raw pointers cross the C ABI, all on one device")
        lab, _ = _device_labels(labels, K, True, "labels")
    else:
        raw = labels if torch.is_tensor(labels) else torch.as_tensor(labels)
        if raw.is_floating_point() or raw.is_complex() or raw.dtype == torch.bool:
            raise TypeError(f"labels must be integers, got {raw.dtype}")
        lab = raw.to(torch.int64).clamp(-1, K).to(torch.int32).to(dev)
    if lab.dim() != 1 or lab.shape[0] != R:
        raise ValueError(f"labels must be ({R},), got {tuple(lab.shape)}")
    return lab.contiguous()


def _check_bank(sums: torch.Tensor, cnt: torch.Tensor):
    _require_cuda(sums, "sums")
    if sums.dim() != 2 or sums.dtype != torch.float32 or not sums.is_contiguous():
        raise TypeError("sums must be a contiguous (K, D) torch.float32 tensor")
    K, D = sums.shape
    if cnt.dtype != torch.int32 or tuple(cnt.shape) != (K,) or cnt.device != sums.device or not cnt.is_contiguous():
        raise TypeError(f"cnt must be a contiguous ({K},) torch.int32 tensor on {sums.device}")
    return K, D, sums.device


def enroll_accumulate(sums: torch.Tensor, cnt: torch.Tensor, embeddings: torch.Tensor, labels, *,
                      workspace: Optional[torch.Tensor] = None) -> None:
    """ge2e_enroll_accumulate, IN PLACE on the caller's bank ``sums`` (K, D) float32 / ``cnt`` (K,) int32 (zeroed once by
    the caller): every row of ``embeddings`` (R, D) whose label is in [0, K) is added to its speaker, rows in any order,
    every other row is ignored and never read.  One row enrols a speaker; a speaker without a row in this call is not
    touched.  Two launches on the current stream, no host sync for device labels.  ``labels``: a device torch.int32 /
    torch.int64 tensor, or a host sequence of ints (copied, not compacted: the ids are bank indices)."""
    K, D, dev = _check_bank(sums, cnt)
    e = _bank_rows(embeddings, D, dev)
    R = e.shape[0]
    with _on_device(dev):
        lab = _bank_labels(labels, K, R, dev)
    _launch_rows("enroll", e, (K, R, D), workspace, e.data_ptr(), lab.data_ptr(), K, R, D, sums.data_ptr(), cnt.data_ptr())


def enroll_finalize(sums: torch.Tensor, cnt: torch.Tensor, eps_cos: float = EPS_COS) -> torch.Tensor:
    """ge2e_enroll_finalize -> ``models`` (K, D): the unit centroid of every enrolled speaker (cnt > 0), +0 elsewhere."""
    K, D, dev = _check_bank(sums, cnt)
    models = torch.empty(K, D, dtype=torch.float32, device=dev)
    _launch("ge2e_enroll_finalize", dev, sums.data_ptr(), cnt.data_ptr(), K, D, float(eps_cos), models.data_ptr(),
            _stream_ptr(sums))
    return models


def verify_scores(embeddings: torch.Tensor, models: torch.Tensor, cnt: torch.Tensor, labels=None, thresholds=None,
                  need_scores: bool = True, eps: float = SMALL_ERR, eps_cos: float = EPS_COS) -> VerifyOutputs:
    """ge2e_verify_scores on the current stream: the trial rows ``embeddings`` (R, D) against ``models`` (K, D) of a bank
    whose ``cnt`` (K,) says who is enrolled.  No leave-one-out: a trial row is no part of a model.  Without ``labels``
    every row is scored and only ``scores`` (R, K) comes back.  With ``labels`` (as `enroll_accumulate` takes them) a row
    with a negative label is ignored (never read, its scores are 0), a row whose label is an enrolled speaker has that
    speaker as its target and every other row is an impostor against everybody; ``trials`` (2,) counts the impostor and
    target scores, and with ``thresholds`` (as `cos_sim_labeled` takes them) ``counts`` (T, 2) holds the accepts per
    threshold.  ``need_scores=False``: the matrix is never materialised."""
    return _verify(embeddings, models, cnt, None, labels, thresholds, need_scores, eps, eps_cos)


def _verify(embeddings, models, cnt, stats, labels, thresholds, need_scores, eps, eps_cos) -> VerifyOutputs:
    """`verify_scores` (``stats`` None) and `verify_scores_normed` (``stats`` = (row_stats, model_stats)): the checks, the
    labels and thresholds, the outputs and the launch."""
    _check_bank(models, cnt)
    K, D = models.shape
    dev = models.device
    e = _bank_rows(embeddings, D, dev)
    R = e.shape[0]
    if stats is not None:
        _check_stats(stats[0], R, dev, "row_stats")
        _check_stats(stats[1], K, dev, "model_stats")
    if labels is None and (thresholds is not None or not need_scores):
        raise ValueError("counts are about targets and impostors: thresholds / need_scores=False need labels")
    if thresholds is None and not need_scores:
        raise ValueError("nothing to compute: need_scores=False without thresholds")
    with _on_device(dev):
        lab = _bank_labels(labels, K, R, dev) if labels is not None else None
        thr = _threshold_table(thresholds, dev, device_ok=True) if thresholds is not None else None
    T = thr.numel() if thr is not None else 0
    i32 = dict(dtype=torch.int32, device=dev)
    out = VerifyOutputs(scores=torch.empty(R, K, dtype=torch.float32, device=dev) if need_scores else None,
                        counts=torch.empty(T, 2, **i32) if T else None,
                        trials=torch.empty(2, **i32) if lab is not None else None)
    tables = () if stats is None else (stats[0].data_ptr(), stats[1].data_ptr())
    _launch("ge2e_verify_scores" if stats is None else "ge2e_verify_scores_normed", dev, e.data_ptr(), _ptr(lab),
            models.data_ptr(), cnt.data_ptr(), K, R, D, float(eps_cos), float(eps), *tables, _ptr(thr), T, _ptr(out.scores),
            _ptr(out.counts), _ptr(out.trials), _stream_ptr(e))
    return out


# ---- identification: the best k enrolled speakers of every trial row (csrc/ge2e_identify.hip) -----------------------------

IDENTIFY_MAX_TOP = _lib.MACROS["GE2E_IDENTIFY_MAX_TOP"]


@dataclass
class IdentifyOutputs:
    indices: torch.Tensor               # (R, k) int32: the best k enrolled speakers, best first; -1 past the enrolled count
    #                                     and on ignored rows
    scores: Optional[torch.Tensor]      # (R, k) float32: their scores, -inf where indices is -1
    rank: Optional[torch.Tensor]        # (R,) int32: the target's position, k if it is outside the list, -1 without target
    hist: Optional[torch.Tensor]        # (k + 1,) int32: rows per rank; [k] = target outside the list


def identify(embeddings: torch.Tensor, models: torch.Tensor, cnt: torch.Tensor, k: int = 1, labels=None,
             need_scores: bool = True, eps: float = SMALL_ERR, eps_cos: float = EPS_COS,
             workspace: Optional[torch.Tensor] = None) -> IdentifyOutputs:
    """ge2e_identify on the current stream: for every trial row of ``embeddings`` (R, D) the best ``k`` enrolled speakers
    of the bank ``models`` (K, D) / ``cnt`` (K,), by `verify_scores`' score (the same bits), equal scores in index order,
    NaN last.  The (R, K) score matrix is never materialised and the bank axis is split over workgroups where R alone
    would not fill the chip.  With ``labels`` (as `verify_scores` takes them) a row with a negative label is ignored
    (never read, all -1), a row whose label is an enrolled speaker has that speaker as its target, and ``rank`` (R,) /
    ``hist`` (k + 1,) come back as well; without labels they are None.  ``need_scores=False``: ``scores`` is None."""
    _check_bank(models, cnt)
    K, D = models.shape
    dev = models.device
    e = _bank_rows(embeddings, D, dev)
    R = e.shape[0]
    k = int(k)
    if not 1 <= k <= IDENTIFY_MAX_TOP:
        raise ValueError(f"k must be in 1 .. {IDENTIFY_MAX_TOP}, got {k}")
    with _on_device(dev):
        lab = _bank_labels(labels, K, R, dev) if labels is not None else None
    i32 = dict(dtype=torch.int32, device=dev)
    out = IdentifyOutputs(indices=torch.empty(R, k, **i32),
                          scores=torch.empty(R, k, dtype=torch.float32, device=dev) if need_scores else None,
                          rank=torch.empty(R, **i32) if lab is not None else None,
                          hist=torch.empty(k + 1, **i32) if lab is not None else None)
    _launch_rows("identify", e, (K, R, D, k), workspace, e.data_ptr(), _ptr(lab), models.data_ptr(), cnt.data_ptr(), K, R, D, k,
                 float(eps_cos), float(eps), out.indices.data_ptr(), _ptr(out.scores), _ptr(out.rank), _ptr(out.hist))
    return out


# ---- score normalisation against a cohort, AS-norm (csrc/ge2e_snorm.hip) ---------------------------------------------------

COHORT_MAX = _lib.MACROS["GE2E_COHORT_MAX"]
EPS_STD = 1e-5


def cohort_stats(rows: torch.Tensor, cohort_models: torch.Tensor, cohort_cnt: torch.Tensor, n_top: int = 300, select=None,
                 select_min: int = 0, eps: float = SMALL_ERR, eps_cos: float = EPS_COS, eps_std: float = EPS_STD,
                 workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ge2e_cohort_stats on the current stream -> ``stats`` (R, 2) float32: for every row of ``rows`` (R, D) the mean and the
    population spread (at least ``eps_std``) of its ``n_top`` best scores against the members of the cohort
    ``cohort_models`` (C, D) / ``cohort_cnt`` (C,) -- a finalised bank; a member has cnt > 0 -- by `verify_scores`' score.
    ``select`` (R,) with ``select_min``: only the rows with select >= select_min are scored; the others are never read and
    get (0, 1), as every row does when the cohort has no member.  Trial rows pass their labels and 0, a bank's own models
    its ``cnt`` and 1.  The (R, C) matrix is never materialised: at most 32 MiB of it at a time."""
    _check_bank(cohort_models, cohort_cnt)
    C, D = cohort_models.shape
    dev = cohort_models.device
    x = _bank_rows(rows, D, dev)
    R = x.shape[0]
    n_top = int(n_top)
    if n_top < 1:
        raise ValueError(f"n_top must be at least 1, got {n_top}")
    if C > COHORT_MAX:
        raise ValueError(f"a cohort holds at most {COHORT_MAX} speakers, got {C}")
    with _on_device(dev):
        sel = _selector(select, R, dev) if select is not None else None
    stats = torch.empty(R, 2, dtype=torch.float32, device=dev)
    _launch_rows("cohort", x, (C, R, D, n_top), workspace, x.data_ptr(), _ptr(sel), int(select_min), cohort_models.data_ptr(),
                 cohort_cnt.data_ptr(), C, R, D, n_top, float(eps_cos), float(eps), float(eps_std), stats.data_ptr())
    return stats


def _selector(select, R: int, dev: torch.device) -> torch.Tensor:
    """(R,) int32 on `dev`: a device torch.int32 tensor (a bank's cnt, a label vector) is taken as it is; 64-bit and host
    integers are clamped into the int32 range before they are narrowed, so that their order against select_min stays."""
    if torch.is_tensor(select) and select.device.type != "cpu" and select.device != dev:
        raise RuntimeError(f"select is on {select.device}, the cohort on {dev}: raw pointers cross the C ABI, all on one device")
    raw = select if torch.is_tensor(select) else torch.as_tensor(select)
    if raw.is_floating_point() or raw.is_complex() or raw.dtype == torch.bool:
        raise TypeError(f"select must be integers, got {raw.dtype}")
    if raw.dim() != 1 or raw.shape[0] != R:
        raise ValueError(f"select must be ({R},), got {tuple(raw.shape)}")
    if raw.dtype != torch.int32:
        raw = raw.to(torch.int64).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32)
    return raw.to(dev).contiguous()


def _check_stats(t: torch.Tensor, n: int, dev: torch.device, name: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (n, 2) or t.device != dev or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous ({n}, 2) torch.float32 tensor on {dev}")
    return t


def verify_scores_normed(embeddings: torch.Tensor, models: torch.Tensor, cnt: torch.Tensor, row_stats: torch.Tensor,
                         model_stats: torch.Tensor, labels=None, thresholds=None, need_scores: bool = True,
                         eps: float = SMALL_ERR, eps_cos: float = EPS_COS) -> VerifyOutputs:
    """ge2e_verify_scores_normed on the current stream: `verify_scores` whose every score v of (row r, enrolled speaker k)
    becomes 0.5 ((v - mu_k) / sd_k + (v - mu_r) / sd_r) before it is stored and counted, with ``row_stats`` (R, 2) and
    ``model_stats`` (K, 2) the (mean, spread) pairs of `cohort_stats` for the trial rows and for the bank's models.  The
    same arguments, outputs and rules otherwise; with both tables (0, 1) the same bits."""
    return _verify(embeddings, models, cnt, (row_stats, model_stats), labels, thresholds, need_scores, eps, eps_cos)


# ---- the reference's static helpers (s3:33-38, 41-80, 95-112, 114-127), differentiable like the originals ----------
# Forward AND backward run in libge2e_hip.so; the autograd.Functions below only carry tensors across the C ABI.

def _cos_forward(e4: torch.Tensor, c3: Optional[torch.Tensor], eps: float, eps_cos: float) -> torch.Tensor:
    B, N, M, D = e4.shape
    dev = e4.device
    cos = torch.empty(B, N, M, N, dtype=torch.float32, device=dev)
    if c3 is not None:
        _launch("ge2e_cos_sim_centroids", dev, e4.data_ptr(), c3.data_ptr(), B, N, M, D, eps_cos, eps, cos.data_ptr(),
                _stream_ptr(e4))
    else:
        with _on_device(dev):      # the size query too runs with the tensor's device current
            ws = alloc_workspace(_lib.load().ge2e_cos_sim_workspace_bytes(B, N, M, D), dev)   # MFMA route where it exists
        _launch("ge2e_cos_sim", dev, e4.data_ptr(), B, N, M, D, eps_cos, eps, cos.data_ptr(), ws.data_ptr(), ws.numel(),
                _stream_ptr(e4))
    return cos


class _CentroidsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e4):
        B, N, M, D = e4.shape
        cent = torch.empty(B, N, D, dtype=torch.float32, device=e4.device)
        _launch("ge2e_centroids", e4.device, e4.data_ptr(), B, N, M, D, cent.data_ptr(), _stream_ptr(e4))
        ctx.shape = (B, N, M, D)
        return cent

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        B, N, M, D = ctx.shape
        g = g.contiguous().float()
        dE = torch.empty(B, N, M, D, dtype=torch.float32, device=g.device)
        _launch("ge2e_centroids_bwd", g.device, g.data_ptr(), B, N, M, D, dE.data_ptr(), _stream_ptr(g))
        return dE


class _UttCentroidsFunction(torch.autograd.Function):
    """u = (sum - e) / (M - 1): linear and symmetric, so backward is the same kernel on the gradient."""

    @staticmethod
    def _run(x):
        B, N, M, D = x.shape
        out = torch.empty_like(x)
        _launch("ge2e_utterance_centroids", x.device, x.data_ptr(), B, N, M, D, out.data_ptr(), _stream_ptr(x))
        return out

    @staticmethod
    def forward(ctx, e4):
        return _UttCentroidsFunction._run(e4)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _UttCentroidsFunction._run(g.contiguous().float())


class _CosSimFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e4, c3, eps, eps_cos, own=False):
        # own: c3 IS get_centroids(e4) (what every caller of the reference passes) -- the forward then takes ge2e_cos_sim,
        # whose contraction runs on the matrix cores for the shapes the tiled kernel accepts; c3 is kept for the backward
        cos = _cos_forward(e4, None if own else c3, eps, eps_cos)
        ctx.save_for_backward(e4, c3, cos)
        ctx.eps, ctx.eps_cos = eps, eps_cos
        return cos

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        e4, c3, cos = ctx.saved_tensors
        B, N, M, D = e4.shape
        g = g.contiguous().float()
        dE = torch.empty_like(e4)
        dC = torch.empty_like(c3)
        ws = alloc_workspace(lib.ge2e_cos_sim_bwd_workspace_bytes(B, N, M, D), e4.device)
        _launch("ge2e_cos_sim_bwd", e4.device, e4.data_ptr(), c3.data_ptr(), cos.data_ptr(), g.data_ptr(), B, N, M, D,
                ctx.eps_cos, ctx.eps, dE.data_ptr(), dC.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(e4))
        return dE, dC, None, None, None


class _CalcLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s4, eps, variant):
        B, N, M, _ = s4.shape
        loss = torch.empty(B, dtype=torch.float32, device=s4.device)
        per = torch.empty(B, N, M, dtype=torch.float32, device=s4.device)
        _launch("ge2e_calc_loss", s4.device, s4.data_ptr(), B, N, M, eps, _lib.VARIANTS[variant], loss.data_ptr(),
                per.data_ptr(), _stream_ptr(s4))
        ctx.save_for_backward(s4)
        ctx.eps, ctx.variant = eps, variant
        return loss, per

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, g_per):
        (s4,) = ctx.saved_tensors
        B, N, M, _ = s4.shape
        gl = g_loss.contiguous().float() if g_loss is not None else None
        gp = g_per.contiguous().float() if g_per is not None else None
        dS = torch.empty_like(s4)
        _launch("ge2e_calc_loss_bwd", s4.device, s4.data_ptr(), B, N, M, ctx.eps, _lib.VARIANTS[ctx.variant],
                gl.data_ptr() if gl is not None else None, gp.data_ptr() if gp is not None else None, dS.data_ptr(),
                _stream_ptr(s4))
        return dS, None, None


def cos_sim(embeddings: torch.Tensor, centroids: torch.Tensor | None = None, *, eps: float = SMALL_ERR,
            eps_cos: float = EPS_COS) -> torch.Tensor:
    """get_cos_sim (s3:42-80): (N,M,D) [, centroids (N,D)] -> (N,M,N) or batched; differentiable in both arguments.

    With ``centroids`` the other-speaker columns use them (as the reference does with its second
    argument); without, they are get_centroids(embeddings) -- what every caller in the reference passes.
    """
    _require_cuda(embeddings, "embeddings")
    e4, squeeze = _as_batched(embeddings)
    B, N, M, D = e4.shape
    own = centroids is None
    if own:
        centroids = _CentroidsFunction.apply(e4)
    _require_cuda(centroids, "centroids")
    c3 = centroids.to(torch.float32).reshape(B, -1, D).contiguous()
    if c3.shape[1] != N:
        # s3:77-78 indexes cos_diff[j, :, j] for every speaker j: the reference needs as many centroids as speakers
        raise RuntimeError(f"get_cos_sim: {c3.shape[1]} centroids for {N} speakers")
    cos = _CosSimFunction.apply(e4, c3, float(eps), float(eps_cos), own)
    return cos[0] if squeeze else cos


class _CosSimRowsFunction(torch.autograd.Function):
    """get_cos_sim on the rows of n speakers (columns j0 .. j0 + n - 1) against all N centroids (ge2e_cos_sim_rows)."""

    @staticmethod
    def forward(ctx, e3, c2, j0, eps, eps_cos):
        n, M, D = e3.shape
        N = c2.shape[0]
        cos = torch.empty(n, M, N, dtype=torch.float32, device=e3.device)
        _launch("ge2e_cos_sim_rows", e3.device, e3.data_ptr(), c2.data_ptr(), 1, n, N, j0, M, D, eps_cos, eps,
                cos.data_ptr(), _stream_ptr(e3))
        ctx.save_for_backward(e3, c2, cos)
        ctx.j0, ctx.eps, ctx.eps_cos = j0, eps, eps_cos
        return cos

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        e3, c2, cos = ctx.saved_tensors
        n, M, D = e3.shape
        N = c2.shape[0]
        g = g.contiguous().float()
        dE, dC = torch.empty_like(e3), torch.empty_like(c2)
        ws = alloc_workspace(lib.ge2e_cos_sim_rows_bwd_workspace_bytes(1, n, N, M, D), e3.device, init=False)
        _launch("ge2e_cos_sim_rows_bwd", e3.device, e3.data_ptr(), c2.data_ptr(), cos.data_ptr(), g.data_ptr(), 1, n, N,
                ctx.j0, M, D, ctx.eps_cos, ctx.eps, dE.data_ptr(), dC.data_ptr(), ws.data_ptr(), ws.numel(),
                _stream_ptr(e3))
        return dE, dC, None, None, None


class _CalcLossRowsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s3, j0, eps, variant):
        n, M, N = s3.shape
        loss = torch.empty(1, dtype=torch.float32, device=s3.device)
        per = torch.empty(n, M, dtype=torch.float32, device=s3.device)
        _launch("ge2e_calc_loss_rows", s3.device, s3.data_ptr(), 1, n, N, j0, M, eps, _lib.VARIANTS[variant],
                loss.data_ptr(), per.data_ptr(), _stream_ptr(s3))
        ctx.save_for_backward(s3)
        ctx.j0, ctx.eps, ctx.variant = j0, eps, variant
        return loss[0], per

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, g_per):
        (s3,) = ctx.saved_tensors
        n, M, N = s3.shape
        gl = g_loss.reshape(1).contiguous().float() if g_loss is not None else None
        gp = g_per.contiguous().float() if g_per is not None else None
        dS = torch.empty_like(s3)
        _launch("ge2e_calc_loss_rows_bwd", s3.device, s3.data_ptr(), 1, n, N, ctx.j0, M, ctx.eps,
                _lib.VARIANTS[ctx.variant], gl.data_ptr() if gl is not None else None,
                gp.data_ptr() if gp is not None else None, dS.data_ptr(), _stream_ptr(s3))
        return dS, None, None, None


def cos_sim_rows(embeddings: torch.Tensor, centroids: torch.Tensor, first_speaker: int, *, eps: float = SMALL_ERR,
                 eps_cos: float = EPS_COS) -> torch.Tensor:
    """get_cos_sim (s3:42-80) restricted to LOCAL ROWS: ``embeddings`` (n,M,D) are the rows of speakers ``first_speaker`` ..
    ``first_speaker + n - 1`` of a batch whose N centroids are ``centroids`` (N,D) -> (n,M,N); the own-speaker column of
    local speaker jl is ``first_speaker + jl`` and carries the cosine with the leave-one-out centroid of the local rows.
    Differentiable in both arguments (the centroid gradient is this shard's partial one).  SURVEY 8e-ii."""
    _require_cuda(embeddings, "embeddings")
    _require_cuda(centroids, "centroids")
    if embeddings.dim() != 3 or centroids.dim() != 2 or centroids.shape[1] != embeddings.shape[2]:
        raise ValueError(f"cos_sim_rows: embeddings (n,M,D) and centroids (N,D), got {tuple(embeddings.shape)}, {tuple(centroids.shape)}")
    n, N = embeddings.shape[0], centroids.shape[0]
    if first_speaker < 0 or first_speaker + n > N:
        raise ValueError(f"cos_sim_rows: speakers {first_speaker}..{first_speaker + n - 1} of {N}")
    return _CosSimRowsFunction.apply(embeddings.contiguous().float(), centroids.contiguous().float(), int(first_speaker),
                                     float(eps), float(eps_cos))


def calc_loss_rows(sim_rows: torch.Tensor, first_speaker: int, *, eps: float = SMALL_ERR, variant: str = "softmax"):
    """calc_loss (s3:114-127) on the similarity rows (n,M,N) of speakers ``first_speaker`` ..: (sum of the per-row losses,
    per-row losses (n,M)); differentiable."""
    _require_cuda(sim_rows, "sim_rows")
    if sim_rows.dim() != 3:
        raise ValueError(f"sim_rows must be (n,M,N), got {tuple(sim_rows.shape)}")
    return _CalcLossRowsFunction.apply(sim_rows.contiguous().float(), int(first_speaker), float(eps), variant)


def centroids(embeddings: torch.Tensor) -> torch.Tensor:
    """get_centroids (s3:34-38): mean over the utterance axis."""
    _require_cuda(embeddings, "embeddings")
    e4, squeeze = _as_batched(embeddings)
    cent = _CentroidsFunction.apply(e4)
    return cent[0] if squeeze else cent


def utterance_centroids(embeddings: torch.Tensor) -> torch.Tensor:
    """get_utterance_centroids (s3:95-112): leave-one-out centroid of every utterance, (N,M,D) -> (N,M,D)."""
    _require_cuda(embeddings, "embeddings")
    e4, squeeze = _as_batched(embeddings)
    u = _UttCentroidsFunction.apply(e4)
    return u[0] if squeeze else u


def calc_loss(sim_matrix: torch.Tensor, *, eps: float = SMALL_ERR, variant: str = "softmax"):
    """calc_loss (s3:115-127) on a (N,M,N) or (B,N,M,N) similarity matrix: (loss, per_embedding_loss), differentiable."""
    _require_cuda(sim_matrix, "sim_matrix")
    s = sim_matrix
    squeeze = s.dim() == 3
    if squeeze:
        s = s.unsqueeze(0)
    if s.dim() != 4 or s.shape[1] != s.shape[3]:
        raise ValueError(f"sim_matrix must be (N,M,N) or (B,N,M,N), got {tuple(sim_matrix.shape)}")
    loss, per = _CalcLossFunction.apply(s.contiguous().float(), float(eps), variant)
    return (loss[0], per[0]) if squeeze else (loss, per)


class _NormalizeUnpermFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, src, unverified):
        rows, D = y.shape
        e = torch.zeros_like(y) if unverified else torch.empty_like(y)
        ctx.unverified = unverified
        rn = torch.empty(rows, dtype=torch.float32, device=y.device)
        _launch("ge2e_normalize_unperm", y.device, y.data_ptr(), src.data_ptr() if src is not None else None, rows, D,
                e.data_ptr(), rn.data_ptr(), _stream_ptr(y))
        ctx.save_for_backward(e, rn, src)
        return e

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        e, rn, src = ctx.saved_tensors
        g = g.contiguous().float()
        rows, D = e.shape
        dy = torch.zeros_like(e) if ctx.unverified else torch.empty_like(e)
        _launch("ge2e_normalize_unperm_bwd", e.device, g.data_ptr(), e.data_ptr(), rn.data_ptr(),
                src.data_ptr() if src is not None else None, rows, D, dy.data_ptr(), _stream_ptr(e))
        return dy, None, None


def normalize_unperm(y: torch.Tensor, unperm=None, shape=None) -> torch.Tensor:
    """The encoder's tail in one kernel: ``(y / |y|)[unperm]`` -- s2:34 then s4:186 --
    optionally reshaped to ``shape`` = (N, M) -> (N,M,D) (s4:189).  ``y`` (rows, D) is the encoder's
    raw projection; ``unperm`` a permutation of range(rows) (list or int tensor), None = identity.
    Differentiable in ``y``."""
    _require_cuda(y, "y")
    if y.dim() != 2:
        raise ValueError(f"y must be (rows, D), got {tuple(y.shape)}")
    rows = y.shape[0]
    src = _unperm_index(unperm, rows, y.device)
    e = _NormalizeUnpermFunction.apply(y.contiguous().float(), src, _index_is_unverified(unperm))
    if shape is not None:
        e = e.reshape(*shape, e.shape[1])
    return e


def _unperm_index(unperm, rows: int, device) -> Optional[torch.Tensor]:
    """The reference's `unperm` (s4:183-186) as an int32 device tensor.  A list is validated on the host and travels
    through pinned memory (no host sync on the step's critical path).  A TENSOR cannot be validated without a sync, and
    the kernels write every output row exactly once only for a true permutation; so for a tensor the outputs are
    ZERO-initialised (`_index_is_unverified`) and the kernels skip entries outside range(rows): an index that is not a
    permutation yields zero rows / zero gradients where nothing was written, never uninitialised memory and never an
    out-of-range access.  `check_unperm` is the explicit (synchronising) test."""
    if unperm is None:
        return None
    if not torch.is_tensor(unperm):
        if sorted(unperm) != list(range(rows)):
            raise ValueError("unperm must be a permutation of range(rows)")
        return torch.tensor(unperm, dtype=torch.int32).pin_memory().to(device, non_blocking=True)
    if unperm.numel() != rows:
        raise ValueError("unperm must have one entry per row")
    return unperm.to(device=device, dtype=torch.int32).contiguous()


def _index_is_unverified(unperm) -> bool:
    """True for an index the host has not validated (a tensor): outputs indexed through it are zero-initialised."""
    return torch.is_tensor(unperm)


def check_unperm(unperm: torch.Tensor, rows: int) -> None:
    """Raises ValueError unless the tensor is a permutation of range(rows).  One host synchronisation."""
    src = unperm.reshape(-1).long()
    if src.numel() != rows or bool((src < 0).any()) or bool((src >= rows).any()) \
            or bool((torch.bincount(src.clamp(0, rows - 1), minlength=rows) != 1).any()):
        raise ValueError("unperm (tensor) is not a permutation of range(rows)")


def encode_supported(n_mels: int, hidden: int, layers: int, dim: int) -> bool:
    """Encoder shapes ge2e_encode runs: hidden 128 or 256, 1..4 layers, up to 256 mel channels and 256 dimensions."""
    return _lib.load().ge2e_encoder_packed_bytes(int(n_mels), int(hidden), int(layers), int(dim)) > 0


def encoder_flat_numel(n_mels: int, hidden: int, layers: int, dim: int) -> int:
    """Elements of the flat parameter buffer ``encoder_pack`` takes."""
    return 4 * hidden * (n_mels + hidden + 2) + (layers - 1) * 4 * hidden * (2 * hidden + 2) + dim * hidden + dim


def encoder_pack(flat_params: torch.Tensor, n_mels: int, hidden: int, layers: int, dim: int) -> torch.Tensor:
    """ge2e_encoder_pack -> the packed weights ``encode`` streams from.  ``flat_params``: one float32 device vector, per
    layer weight_ih, weight_hh, bias_ih, bias_hh in torch's layout (gate order i, f, g, o), then projection.weight and
    projection.bias.  One launch on the current stream; run it once per set of weights."""
    _require_cuda(flat_params, "flat_params")
    nbytes = _lib.load().ge2e_encoder_packed_bytes(int(n_mels), int(hidden), int(layers), int(dim))
    if nbytes == 0:
        raise ValueError(f"encoder shape (n_mels {n_mels}, hidden {hidden}, layers {layers}, dim {dim}) has no native kernel")
    f = flat_params.detach()
    if f.dim() != 1 or f.dtype != torch.float32 or not f.is_contiguous() or \
            f.numel() != encoder_flat_numel(n_mels, hidden, layers, dim):
        raise ValueError(f"flat_params must be a contiguous float32 vector of "
                         f"{encoder_flat_numel(n_mels, hidden, layers, dim)} elements, got {tuple(f.shape)} {f.dtype}")
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=f.device)
    _launch("ge2e_encoder_pack", f.device, f.data_ptr(), int(n_mels), int(hidden), int(layers), int(dim), packed.data_ptr(),
            _stream_ptr(f))
    return packed


def _encoder_rows(mel: torch.Tensor, T: Optional[int], row_start: Optional[torch.Tensor]):
    """The mel argument of ``encode`` / ``encode_train`` -> (contiguous float32 mels, row_start or None, R, T, n_mels)."""
    _require_cuda(mel, "mel")
    dev = mel.device
    m = mel.detach()
    if m.dtype == torch.float64:
        m = m.float()
    if m.dtype != torch.float32:
        raise TypeError(f"mel must be float32 or float64, got {mel.dtype}")
    m = m.contiguous()
    if row_start is None:
        if m.dim() != 3 or m.shape[0] < 1 or m.shape[1] < 1 or (T is not None and T != m.shape[1]):
            raise ValueError(f"mel must be (R, T, n_mels) with R, T >= 1 (or flat with row_start and T), got {tuple(m.shape)}")
        return m, None, m.shape[0], m.shape[1], m.shape[2]
    if m.dim() != 2 or T is None or T < 1 or m.shape[0] < T:
        raise ValueError("with row_start, mel must be flat (frames, n_mels) with frames >= T, and T given")
    if row_start.dtype != torch.int64 or row_start.dim() != 1 or row_start.device != dev or row_start.numel() < 1:
        raise TypeError(f"row_start must be a (R,) torch.int64 tensor on {dev}")
    return m, row_start.contiguous(), row_start.numel(), int(T), m.shape[1]


def encode(packed: torch.Tensor, mel: torch.Tensor, *, T: Optional[int] = None, row_start: Optional[torch.Tensor] = None,
           hidden: int, layers: int, dim: int, normalize: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ge2e_encode: mel windows to d-vectors (R, dim) float32 in one launch on the current stream, no workspace.
    ``mel``: (R, T, n_mels); or flat (frames, n_mels) with ``row_start`` (R,) int64 on the device -- the first frame of
    every window, windows may overlap -- and ``T``, the window length.  float64 mels are cast to float32 (s2:28).
    ``normalize=False`` returns the raw projection (``SpeakerEncoder.raw``'s contract).  ``out``: a contiguous (R, dim)
    float32 tensor to write into (static buffers of a captured graph)."""
    m, row_start, R, T, n_mels = _encoder_rows(mel, T, row_start)
    dev = m.device
    rs_ptr = None if row_start is None else row_start.data_ptr()
    if packed.device != dev or packed.dtype != torch.float32 or not packed.is_contiguous() or \
            packed.numel() * 4 != _lib.load().ge2e_encoder_packed_bytes(n_mels, int(hidden), int(layers), int(dim)):
        raise ValueError(f"packed is not encoder_pack's buffer for (n_mels {n_mels}, hidden {hidden}, layers {layers}, "
                         f"dim {dim}) on {dev}")
    if out is None:
        out = torch.empty(R, dim, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (R, dim) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise TypeError(f"out must be a contiguous ({R}, {dim}) torch.float32 tensor on {dev}")
    _launch("ge2e_encode", dev, packed.data_ptr(), m.data_ptr(), rs_ptr, R, int(T), n_mels, int(hidden), int(layers), int(dim),
            int(bool(normalize)), out.data_ptr(), _stream_ptr(m))
    return out


def encode_train_tape_bytes(R: int, T: int, n_mels: int, hidden: int, layers: int, dim: int) -> int:
    """Bytes of the tape ``encode_train`` keeps between its forward and its backward: 4 (6 layers T R hidden + R dim) --
    2.9 MB a window for 80 -> 3 x 256 -> 256 at T = 160.  0 for a shape without a kernel."""
    return _lib.load().ge2e_encode_train_tape_bytes(int(R), int(T), int(n_mels), int(hidden), int(layers), int(dim))


def encode_bwd_workspace_bytes(R: int, T: int, n_mels: int, hidden: int, layers: int, dim: int) -> int:
    """Bytes of the workspace ``encode_train``'s backward allocates: the dZ planes (4 layers T R 4 hidden), dy and the
    K-slice partials of the weight gradients.  0 for a shape without a kernel."""
    return _lib.load().ge2e_encode_bwd_workspace_bytes(int(R), int(T), int(n_mels), int(hidden), int(layers), int(dim))


class _EncodeTrainFunction(torch.autograd.Function):
    """ge2e_encode_train / ge2e_encode_bwd as one autograd node over the parameter tensors in pack order."""

    @staticmethod
    def forward(ctx, m, row_start, shape, normalize, *params):
        R, T, n_mels, H, L, D = shape
        lib, dev, stream = _lib.load(), m.device, _stream_ptr(m)
        flat = torch.cat([p.detach().reshape(-1) for p in params])
        packed = encoder_pack(flat, n_mels, H, L, D)
        packed_bwd = torch.empty(lib.ge2e_encoder_packed_bwd_bytes(n_mels, H, L, D) // 4, dtype=torch.float32, device=dev)
        _launch("ge2e_encoder_pack_bwd", dev, flat.data_ptr(), n_mels, H, L, D, packed_bwd.data_ptr(), stream)
        tape = torch.empty(lib.ge2e_encode_train_tape_bytes(*shape) // 4, dtype=torch.float32, device=dev)
        out = torch.empty(R, D, dtype=torch.float32, device=dev)
        rs_ptr = None if row_start is None else row_start.data_ptr()
        _launch("ge2e_encode_train", dev, packed.data_ptr(), m.data_ptr(), rs_ptr, R, T, n_mels, H, L, D, int(normalize),
                out.data_ptr(), tape.data_ptr(), stream)
        ctx.save_for_backward(m, packed_bwd, tape, *([] if row_start is None else [row_start]))
        ctx.cfg = (shape, normalize, [tuple(p.shape) for p in params])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        shape, normalize, shapes = ctx.cfg
        R, T, n_mels, H, L, D = shape
        m, packed_bwd, tape, *rest = ctx.saved_tensors
        lib, dev = _lib.load(), m.device
        g = g.detach().to(torch.float32).contiguous()
        d_flat = torch.empty(encoder_flat_numel(n_mels, H, L, D), dtype=torch.float32, device=dev)
        ws = torch.empty(lib.ge2e_encode_bwd_workspace_bytes(*shape) // 4, dtype=torch.float32, device=dev)
        _launch("ge2e_encode_bwd", dev, packed_bwd.data_ptr(), m.data_ptr(), rest[0].data_ptr() if rest else None, R, T, n_mels,
                H, L, D, int(normalize), tape.data_ptr(), g.data_ptr(), d_flat.data_ptr(), ws.data_ptr(), _stream_ptr(m))
        grads, off = [], 0
        for s in shapes:                                  # the views of the flat buffer, one per parameter
            n = 1
            for d in s:
                n *= d
            grads.append(d_flat[off:off + n].view(s))
            off += n
        return (None, None, None, None, *grads)


def encode_train(params, mel: torch.Tensor, *, T: Optional[int] = None, row_start: Optional[torch.Tensor] = None,
                 hidden: int, layers: int, dim: int, normalize: bool = True) -> torch.Tensor:
    """The encoder's forward WITH gradients, native both ways: ge2e_encode_train keeps a tape, and ``backward()`` runs
    ge2e_encode_bwd -- the LSTM backward through time, the projection's and the norm's backward in hand-written HIP --
    and hands every parameter its gradient as a view of one flat buffer.  ``params``: the float32 parameter tensors in
    pack order (per layer weight_ih, weight_hh, bias_ih, bias_hh; then projection.weight, projection.bias) on ``mel``'s
    device; they are concatenated and packed on every call.  ``mel``, ``T`` and ``row_start`` as ``encode``; the output
    (R, dim) has ``encode``'s bits.  No gradient goes to the mels: a ``mel`` that requires grad raises.  The tape takes
    ``encode_train_tape_bytes`` between forward and backward, the backward ``encode_bwd_workspace_bytes`` more.  Raises
    where the shape has no kernel: there is no fallback here."""
    if mel.requires_grad:
        raise ValueError("encode_train produces no gradient with respect to the mels: mel must not require grad")
    params = list(params)
    m, row_start, R, T, n_mels = _encoder_rows(mel, T, row_start)
    shape = (int(R), int(T), int(n_mels), int(hidden), int(layers), int(dim))
    if not encode_supported(*shape[2:]):
        raise ValueError(f"encoder shape (n_mels {n_mels}, hidden {hidden}, layers {layers}, dim {dim}) has no native kernel")
    want = [(4 * hidden, n_mels if l == 0 else hidden) if k == 0 else (4 * hidden, hidden) if k == 1 else (4 * hidden,)
            for l in range(layers) for k in range(4)] + [(dim, hidden), (dim,)]
    if [tuple(p.shape) for p in params] != want or any(p.dtype != torch.float32 or p.device != m.device for p in params):
        raise ValueError(f"params must be the {len(want)} float32 tensors of the encoder in pack order on {m.device}: {want}")
    return _EncodeTrainFunction.apply(m, row_start, shape, bool(normalize), *params)


def melspec_supported(n_fft: int, n_mels: int) -> bool:
    """Front-end shapes ge2e_melspec runs: n_fft 256, 512, 1024 or 2048 and up to 128 mel channels."""
    return _lib.load().ge2e_melspec_packed_bytes(int(n_fft), int(n_mels)) > 0


# ---- what the audio stages (melspec, resample, volume_gain, vad_*, trim_silences) share: the layout and the call prologue ----
def _resolve_device(device=None) -> torch.device:
    """``device`` as a torch.device; None, and "cuda" without an index, are the current device."""
    dev = torch.device("cuda" if device is None else device)
    return torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev


def _int_list(values) -> list:
    return [int(v) for v in (values.tolist() if isinstance(values, torch.Tensor) else values)]


def _utterance_tables(ls: list, counts: list, device, *extra):
    """The tables of an audio layout.  ``ls``: the utterances' sample counts, back to back in the flat buffer; ``counts``:
    how many units (frames, output samples, windows) each has; ``extra``: further per-utterance rows.  Returns ``(unit_start,
    rows)``: the running starts of the units as a Python list of U + 1 entries, the last one the total, and int64 views of
    ONE upload to ``device``: the utterances' starts, their lengths, every extra row, then the U + 1 unit starts.
    ``counts=None``: no units -- ``unit_start`` is None and the rows are the starts and the lengths alone.  Python ints
    until the upload: a length past 2^32 stays exact."""
    if len(ls) < 1 or min(ls) < 0:
        raise ValueError("there must be at least one utterance, none of a negative length")
    starts = list(accumulate(ls, initial=0))
    unit_start = None if counts is None else list(accumulate(counts, initial=0))
    rows = [starts[:-1], ls, *extra] + ([] if counts is None else [unit_start])
    d = torch.tensor(sum(rows, []), dtype=torch.int64).to(_resolve_device(device))
    return unit_start, d.split([len(row) for row in rows])


def _utterances(layout):
    """``(starts, lengths, ls)`` of a MelLayout, ResampleLayout or VadLayout: where its utterances lie in the flat buffer,
    int64 on the device, and the lengths as the Python list.  Every layout type has the two tensors as its first fields."""
    if not isinstance(layout, (MelLayout, ResampleLayout, VadLayout)):
        raise TypeError("layout must be a melspec_layout, a resample_layout or a vad_layout")
    return layout[0], layout[1], layout.lengths


def _flat_wav(wav: torch.Tensor) -> torch.Tensor:
    w = wav.detach()
    if w.dim() != 1 or w.dtype != torch.float32 or not w.is_contiguous():
        raise TypeError(f"wav must be a flat contiguous float32 tensor, got {tuple(w.shape)} {w.dtype}")
    return w


def _check_fits(starts: torch.Tensor, ls: list, w: torch.Tensor) -> None:
    """Utterances of ``ls`` samples, their starts in ``starts``, lie inside ``w`` on w's device."""
    if starts.device != w.device or sum(ls) > w.numel():
        raise ValueError(f"the utterances add up to {sum(ls)} samples with their starts on {starts.device}; wav has "
                         f"{w.numel()} on {w.device}")


def _check_gain(gain: Optional[torch.Tensor], U: int, dev) -> Optional[torch.Tensor]:
    if gain is None:
        return None
    if gain.dtype != torch.float32 or gain.device != dev or tuple(gain.shape) != (U,) or not gain.is_contiguous():
        raise TypeError(f"gain must be a contiguous ({U},) torch.float32 tensor on {dev}")
    return gain.detach()


def _out_tensor(out: Optional[torch.Tensor], shape: tuple, dev) -> torch.Tensor:
    """``out`` where it is the contiguous float32 tensor of ``shape`` on ``dev``, a new one where it is None."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    if tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise TypeError(f"out must be a contiguous {shape} torch.float32 tensor on {dev}")
    return out


def _use_native(native: Optional[bool], supported: bool, name: str, what, default: Optional[bool] = None) -> bool:
    """The route of an audio entry: ``native=None`` takes ``default`` (the kernel wherever there is one, where None),
    ``native=True`` raises where there is none; ``what()`` names the parameters without a kernel."""
    use = (supported if default is None else default) if native is None else bool(native)
    if use and not supported:
        raise RuntimeError(f"{name}(native=True): no HIP kernel for {what()}")
    return use


def _utterance_views(w: torch.Tensor, layout) -> list:
    """The utterances of the flat buffer as views, in the layout's order (the torch routes)."""
    return [w[a:a + n] for a, n in zip(accumulate(layout.lengths, initial=0), layout.lengths)]


class MelTables(NamedTuple):
    """What ``melspec_pack`` returns: the window (n_fft,) and basis (n_fft/2 + 1, n_mels) as given (float32, the torch
    route reads them) and ``packed``, ge2e_melspec_pack's buffer, or None where the shape has no native kernel."""
    packed: Optional[torch.Tensor]
    window: torch.Tensor
    basis: torch.Tensor

    @property
    def n_fft(self) -> int:
        return self.window.numel()

    @property
    def n_mels(self) -> int:
        return self.basis.shape[1]


class MelLayout(NamedTuple):
    """Where the utterances of a flat waveform buffer lie and where their frames go: int64 device tensors for the kernel,
    ``frame_start`` also as a Python list (U + 1 entries, the last one the frame total).  Pure arithmetic on lengths."""
    utt_start: torch.Tensor
    utt_len: torch.Tensor
    utt_padded_len: torch.Tensor
    frame_start_dev: torch.Tensor
    frame_start: list
    lengths: list
    padded_lengths: list
    hop: int


def melspec_pack(window: torch.Tensor, basis: torch.Tensor) -> MelTables:
    """ge2e_melspec_pack -> the tables ``melspec`` reads.  ``window`` (n_fft,) and ``basis`` (n_fft/2 + 1, n_mels) on the
    device, any values (``audio.hann_window`` / ``audio.mel_filterbank`` make the reference's); cast to float32.  One
    launch on the current stream; run it once per (window, basis).  For a shape without a kernel ``packed`` is None and
    ``melspec`` takes its torch route."""
    _require_cuda(window, "window")
    w = window.detach().to(torch.float32).contiguous()
    b = basis.detach().to(device=w.device, dtype=torch.float32).contiguous()
    if w.dim() != 1 or b.dim() != 2 or w.numel() % 2 or b.shape[0] != w.numel() // 2 + 1 or b.shape[1] < 1:
        raise ValueError(f"window must be (n_fft,) with n_fft even and basis (n_fft/2 + 1, n_mels), got {tuple(w.shape)} "
                         f"and {tuple(b.shape)}")
    n_fft, n_mels = w.numel(), b.shape[1]
    nbytes = _lib.load().ge2e_melspec_packed_bytes(n_fft, n_mels)
    if nbytes == 0:
        return MelTables(None, w, b)
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
    _launch("ge2e_melspec_pack", w.device, w.data_ptr(), b.data_ptr(), n_fft, n_mels, packed.data_ptr(), _stream_ptr(w))
    return MelTables(packed, w, b)


def melspec_layout(lengths, *, hop: int, n_fft: int, padded_lengths=None, device=None) -> MelLayout:
    """The index tables of a ``melspec`` call: utterance u is ``lengths[u]`` samples from the sum of the lengths before
    it, extended with zeros to ``padded_lengths[u]`` (its own length where None), and has ``padded // hop + 1`` frames.
    ``lengths`` / ``padded_lengths``: Python lists or CPU tensors.  Build it once for a captured graph and pass it as
    ``melspec(layout=...)``: building it uploads four small tensors."""
    ls = _int_list(lengths)
    ps = list(ls) if padded_lengths is None else _int_list(padded_lengths)
    if hop < 1 or len(ls) < 1 or len(ps) != len(ls):
        raise ValueError("melspec needs hop >= 1, at least one utterance and one padded length per utterance")
    for n, p in zip(ls, ps):
        if n < 0 or p < n or p <= n_fft // 2:
            raise ValueError(f"an utterance of {n} samples padded to {p}: the padded length must be at least the length "
                             f"and more than n_fft / 2 = {n_fft // 2} (the reflection)")
    frame_start, rows = _utterance_tables(ls, [p // hop + 1 for p in ps], device, ps)
    return MelLayout(*rows, frame_start, ls, ps, int(hop))


def _melspec_torch(t: MelTables, wav, lay: MelLayout, gain, mode, min_level_db, ref_level_db, out):
    """The same frames with torch's ops on wav's device: pad, ``unfold``, ``torch.fft.rfft``, ``matmul``."""
    n_fft = t.n_fft
    for u, x in enumerate(_utterance_views(wav, lay)):
        if gain is not None:
            x = x * gain[u]
        x = torch.nn.functional.pad(x, (0, lay.padded_lengths[u] - lay.lengths[u]))
        x = torch.nn.functional.pad(x[None, None], (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
        m = torch.fft.rfft(x.unfold(0, n_fft, lay.hop) * t.window, dim=1).abs().matmul(t.basis)
        if mode == "db":
            level = torch.full((), 10.0 ** (min_level_db / 20.0), dtype=m.dtype, device=m.device)
            m = ((20.0 * torch.log10(torch.maximum(level, m)) - ref_level_db - min_level_db) / -min_level_db).clamp(0.0, 1.0)
        out[lay.frame_start[u]:lay.frame_start[u + 1]] = m
    return out


def melspec(packed, wav: torch.Tensor, lengths=None, *, hop: int, n_fft: Optional[int] = None, n_mels: Optional[int] = None,
            padded_lengths=None, gain: Optional[torch.Tensor] = None, mode: str = "db", min_level_db: float = -100.0,
            ref_level_db: float = 16.0, out: Optional[torch.Tensor] = None, native: Optional[bool] = None,
            layout: Optional[MelLayout] = None):
    """ge2e_melspec: waveforms to mel frames in one launch on the current stream, no workspace -> ``(frames,
    frame_start)``: ``frames`` (total_frames, n_mels) float32, the layout ``encode(..., row_start=)`` reads, and
    ``frame_start`` a Python list of U + 1 first rows (host arithmetic on the lengths: nothing is read back).
    ``packed``: ``melspec_pack``'s MelTables (or its raw ``packed`` tensor, with ``n_fft`` and ``n_mels``).  ``wav``: a flat
    float32 device tensor holding the utterances back to back, ``lengths`` their sample counts (a list or CPU tensor; None:
    ``wav`` is one utterance); ``padded_lengths``: the length each utterance is zero-extended to, without a copy;
    ``gain`` (U,) float32 on the device: a scale per utterance (``audio.volume_gain``).  ``mode`` "db" (the reference's
    normalised log-mel in [0, 1]) or "linear".  ``layout``: a ``melspec_layout`` built beforehand (a captured graph).
    ``native=None`` takes the kernel where the shape has one and the torch route otherwise; ``native=True`` raises where
    it has none; ``native=False`` is the torch route."""
    _require_cuda(wav, "wav")
    dev = wav.device
    w = _flat_wav(wav)
    if mode not in ("db", "linear"):
        raise ValueError(f"mode must be 'db' or 'linear', got {mode!r}")
    if not min_level_db < 0:
        raise ValueError("min_level_db must be below 0")
    tables = packed if isinstance(packed, MelTables) else None
    if tables is not None:
        if (n_fft is not None and n_fft != tables.n_fft) or (n_mels is not None and n_mels != tables.n_mels):
            raise ValueError(f"the tables are for n_fft {tables.n_fft}, n_mels {tables.n_mels}, not {n_fft}, {n_mels}")
        n_fft, n_mels, pk = tables.n_fft, tables.n_mels, tables.packed
    else:
        pk = packed
        if n_fft is None or n_mels is None:
            raise ValueError("a raw packed tensor needs n_fft and n_mels")
    # (native=False does not ask the library whether the shape has a kernel)
    supported = (native is None or bool(native)) and pk is not None and melspec_supported(n_fft, n_mels)
    use_native = _use_native(native, supported, "melspec", lambda: f"n_fft {n_fft}, n_mels {n_mels}")
    if not use_native and tables is None:
        raise ValueError("the torch route needs melspec_pack's MelTables (window and basis), not a raw packed tensor")
    if layout is None:
        layout = melspec_layout([w.numel()] if lengths is None else lengths, hop=hop, n_fft=n_fft,
                                padded_lengths=padded_lengths, device=dev)
    elif layout.hop != hop or layout.utt_start.device != dev:
        raise ValueError(f"layout was built for hop {layout.hop} on {layout.utt_start.device}")
    _check_fits(layout.utt_start, layout.lengths, w)
    U, total = len(layout.lengths), layout.frame_start[-1]
    gain = _check_gain(gain, U, dev)
    out = _out_tensor(out, (total, n_mels), dev)
    if not use_native:
        return _melspec_torch(tables, w, layout, gain, mode, min_level_db, ref_level_db, out), layout.frame_start
    if pk.device != dev or pk.dtype != torch.float32 or not pk.is_contiguous() or \
            pk.numel() * 4 != _lib.load().ge2e_melspec_packed_bytes(n_fft, n_mels):
        raise ValueError(f"packed is not melspec_pack's buffer for n_fft {n_fft}, n_mels {n_mels} on {dev}")
    _launch("ge2e_melspec", dev, pk.data_ptr(), w.data_ptr(), layout.utt_start.data_ptr(), layout.utt_len.data_ptr(),
            layout.utt_padded_len.data_ptr(), None if gain is None else gain.data_ptr(), layout.frame_start_dev.data_ptr(),
            U, total, n_fft, int(hop), n_mels, int(mode == "db"), float(min_level_db), float(ref_level_db), out.data_ptr(),
            _stream_ptr(w))
    return out, layout.frame_start


def resample_supported(up: int, down: int, width: int) -> bool:
    """Banks ge2e_resample runs: up and down in 1 .. 640 and an odd width (taps a phase) of at most 1025."""
    return _lib.load().ge2e_resample_packed_bytes(int(up), int(down), int(width)) > 0


class ResampleTables(NamedTuple):
    """What ``resample_pack`` returns: the bank (up, 2 lead + 1) as given (float32, the torch route reads it), the ratio and
    ``packed``, ge2e_resample_pack's buffer, or None where the shape has no native kernel."""
    packed: Optional[torch.Tensor]
    taps: torch.Tensor
    up: int
    down: int
    lead: int
    weight: torch.Tensor     # the torch route's conv1d weight (up, 1, width + (up - 1) down // up)

    @property
    def width(self) -> int:
        return self.taps.shape[1]


class ResampleLayout(NamedTuple):
    """Where the utterances of a flat waveform buffer lie and where their resampled samples go: int64 device tensors for the
    kernel, ``out_start`` also as a Python list (U + 1 entries, the last one the total).  Pure arithmetic on lengths."""
    in_start: torch.Tensor
    in_len: torch.Tensor
    out_start_dev: torch.Tensor
    out_start: list
    lengths: list
    out_lengths: list
    up: int
    down: int


def _resample_conv_weight(taps: torch.Tensor, up: int, down: int) -> torch.Tensor:
    """The torch route's conv1d weight (up, 1, width + (up - 1) down // up): channel c = n mod up has phase (c down) mod up
    and starts (c down) div up samples further on; conv1d correlates, so the taps are reversed."""
    c = torch.arange(up, device=taps.device)
    width = taps.shape[1]
    weight = taps.new_zeros(up, width + (up - 1) * down // up)
    weight.scatter_(1, ((c * down) // up)[:, None] + torch.arange(width, device=taps.device)[None, :],
                    taps[(c * down) % up].flip(1))
    return weight[:, None, :]


def resample_pack(taps: torch.Tensor, up: int, down: int, lead: int) -> ResampleTables:
    """ge2e_resample_pack -> the tables ``resample`` reads.  ``taps`` (up, 2 lead + 1) on the device, any values
    (``audio.resample_bank`` makes the project's Kaiser-windowed sinc); cast to float32.  One launch on the current stream;
    run it once per bank.  For a shape without a kernel ``packed`` is None and ``resample`` takes its torch route."""
    _require_cuda(taps, "taps")
    t = taps.detach().to(torch.float32).contiguous()
    up, down, lead = int(up), int(down), int(lead)
    if up < 1 or down < 1 or lead < 0 or tuple(t.shape) != (up, 2 * lead + 1):
        raise ValueError(f"taps must be (up, 2 lead + 1) = ({up}, {2 * lead + 1}) with up, down >= 1 and lead >= 0, got "
                         f"{tuple(t.shape)}")
    width, weight = 2 * lead + 1, _resample_conv_weight(t, up, down)
    nbytes = _lib.load().ge2e_resample_packed_bytes(up, down, width)
    if nbytes == 0:
        return ResampleTables(None, t, up, down, lead, weight)
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=t.device)
    _launch("ge2e_resample_pack", t.device, t.data_ptr(), up, down, lead, packed.data_ptr(), _stream_ptr(t))
    return ResampleTables(packed, t, up, down, lead, weight)


def resample_layout(lengths, up: int, down: int, device=None) -> ResampleLayout:
    """The index tables of a ``resample`` call: utterance u is ``lengths[u]`` samples from the sum of the lengths before it
    and becomes ``ceil(lengths[u] up / down)`` samples from the sum of those before it.  ``lengths``: a Python list or CPU
    tensor.  Build it once for a captured graph and pass it as ``resample(layout=...)``: building it is host arithmetic and
    one small upload."""
    ls, up, down = _int_list(lengths), int(up), int(down)
    if up < 1 or down < 1:
        raise ValueError("resample needs up, down >= 1")
    out_lengths = [(n * up + down - 1) // down for n in ls]
    out_start, rows = _utterance_tables(ls, out_lengths, device)
    return ResampleLayout(*rows, out_start, ls, out_lengths, up, down)


def _resample_torch(t: ResampleTables, wav, lay: ResampleLayout, out):
    """The same samples with torch's ops on wav's device, what a caller without the kernel would write: per utterance a
    ``conv1d`` with ``up`` output channels of ``width`` taps at stride ``down`` over the zero-padded utterance; output n is
    channel n mod up at position n div up."""
    L, M, lead, W = t.up, t.down, t.lead, t.width
    shift, weight = (L - 1) * M // L, t.weight
    for u, (x, n, n_out) in enumerate(zip(_utterance_views(wav, lay), lay.lengths, lay.out_lengths)):
        if n_out:
            q = (n_out + L - 1) // L                      # positions: outputs n = c + L j, j < q
            right = max(0, (q - 1) * M + shift + lead + 1 - n)
            x = torch.nn.functional.pad(x, (W - 1 - lead, right))
            y = torch.nn.functional.conv1d(x[None, None], weight, stride=M)[0, :, :q]
            out[lay.out_start[u]:lay.out_start[u + 1]] = y.t().reshape(-1)[:n_out]
    return out


def resample(tables: ResampleTables, wav: torch.Tensor, lengths=None, *, out: Optional[torch.Tensor] = None,
             native: Optional[bool] = None, layout: Optional[ResampleLayout] = None):
    """ge2e_resample: waveforms at one rate to another in one launch on the current stream, no workspace -> ``(flat,
    out_lengths)``: ``flat`` float32, the resampled utterances back to back, and ``out_lengths`` a Python list of their
    sample counts, ceil(length up / down) (host arithmetic: nothing is read back).  ``tables``: ``resample_pack``'s.
    ``wav``: a flat float32 device tensor holding the utterances back to back, ``lengths`` their sample counts (a list or
    CPU tensor; None: ``wav`` is one utterance); every utterance is taken as zero outside its own extent.  ``layout``: a
    ``resample_layout`` built beforehand (a captured graph).  ``native=None`` takes the kernel where the shape has one and
    the torch route otherwise; ``native=True`` raises where it has none; ``native=False`` is the torch route (a strided
    ``conv1d``).  No change-over between the two: at every size measured the kernel is the faster one
    (profiles/resample_bench.txt)."""
    _require_cuda(wav, "wav")
    dev = wav.device
    w = _flat_wav(wav)
    if not isinstance(tables, ResampleTables):
        raise TypeError("tables must be resample_pack's ResampleTables")
    use_native = _use_native(native, tables.packed is not None, "resample",
                             lambda: f"up {tables.up}, down {tables.down}, width {tables.width}")
    if layout is None:
        layout = resample_layout([w.numel()] if lengths is None else lengths, tables.up, tables.down, device=dev)
    elif (layout.up, layout.down) != (tables.up, tables.down) or layout.in_start.device != dev:
        raise ValueError(f"layout was built for {layout.up} / {layout.down} on {layout.in_start.device}")
    _check_fits(layout.in_start, layout.lengths, w)
    U, total = len(layout.lengths), layout.out_start[-1]
    out = _out_tensor(out, (total,), dev)
    if total == 0:
        return out, layout.out_lengths
    if not use_native:
        return _resample_torch(tables, w, layout, out), layout.out_lengths
    pk = tables.packed
    if pk.device != dev:
        raise ValueError(f"the tables are on {pk.device}, wav on {dev}")
    _launch("ge2e_resample", dev, pk.data_ptr(), w.data_ptr(), layout.in_start.data_ptr(), layout.in_len.data_ptr(),
            layout.out_start_dev.data_ptr(), U, total, tables.up, tables.down, tables.lead, out.data_ptr(), _stream_ptr(w))
    return out, layout.out_lengths


def volume_gain(wav: torch.Tensor, lengths=None, target_dbfs: float = -30.0, increase_only: bool = True,
                native: Optional[bool] = None, *, layout=None, out: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ge2e_volume_gain: the factor ``normalize_volume`` multiplies every utterance by, (U,) float32 on wav's device, in two
    launches on the current stream: the sum of squares per utterance in float64 in a fixed order, without the float64
    copies of the whole buffer ``audio.volume_gain`` makes.  ``wav`` flat float32, ``lengths`` as ``resample`` (None: one
    utterance).  ``native=False``: ``audio.volume_gain``, the torch route; None and True: the kernel (it has no unsupported
    shape).  ``layout`` (a ``melspec_layout``, ``resample_layout`` or ``vad_layout`` of the utterances in ``wav``: its
    starts and lengths on the device are used), ``out`` (U,) and ``workspace`` (``volume_gain_workspace``) make the call
    allocation-free for a captured graph."""
    if native is not None and not native:
        from .audio import volume_gain as torch_route
        return torch_route(wav, lengths, target_dbfs, increase_only)
    _require_cuda(wav, "wav")
    dev = wav.device
    w = _flat_wav(wav)
    if layout is None:
        ls = [w.numel()] if lengths is None else _int_list(lengths)
        _, (start_dev, len_dev) = _utterance_tables(ls, None, dev)
    else:
        start_dev, len_dev, ls = _utterances(layout)
    _check_fits(start_dev, ls, w)
    U = len(ls)
    out = _out_tensor(out, (U,), dev)
    if workspace is None:
        workspace = volume_gain_workspace(w.numel(), U, dev)
    elif workspace.device != dev or workspace.dtype != torch.float64 or not workspace.is_contiguous() or \
            workspace.numel() * 8 < _lib.load().ge2e_volume_gain_workspace_bytes(w.numel(), U):
        raise TypeError(f"workspace must be volume_gain_workspace({w.numel()}, {U}) on {dev}")
    _launch("ge2e_volume_gain", dev, w.data_ptr(), start_dev.data_ptr(), len_dev.data_ptr(), U, float(target_dbfs),
            int(bool(increase_only)), out.data_ptr(), workspace.data_ptr(), _stream_ptr(w))
    return out


def volume_gain_workspace(total_samples: int, U: int, device) -> torch.Tensor:
    """A float64 tensor of ge2e_volume_gain_workspace_bytes for ``volume_gain(workspace=...)``."""
    return torch.empty(_lib.load().ge2e_volume_gain_workspace_bytes(int(total_samples), int(U)) // 8, dtype=torch.float64,
                       device=device)


VAD_DEFAULTS = dict(floor_span=100, ratio_db=9.0, min_level_dbfs=-60.0)     # the built-in detector's parameters
# vad_mask(native=None) takes the torch route for an utterance of more windows than this (41 min at 30 ms a window): the mask
# kernel walks an utterance in one workgroup, 12 us a chunk of 4096 windows, and torch's dozen launches cost about 0.28 ms at
# any size measured; at 30 chunks it is 0.39 ms against 0.29 ms (profiles/vad_bench.txt).  The other stages have no change-over.
VAD_MASK_TORCH_FROM = 20 * 4096


class VadLayout(NamedTuple):
    """Where the utterances of a flat waveform buffer lie and which windows of ``window`` samples they have: int64 device
    tensors for the kernels, ``win_start`` also as a Python list (U + 1 entries, the last one the total).  Pure arithmetic on
    lengths."""
    utt_start: torch.Tensor
    utt_len: torch.Tensor
    win_start_dev: torch.Tensor
    win_start: list
    lengths: list
    window: int

    @property
    def total_windows(self) -> int:
        return self.win_start[-1]


def vad_supported(window: int, floor_span: int = 0, avg_width: int = 1, max_silence: int = 0) -> bool:
    """Parameters the silence-trimming kernels run: a window of 2 .. 4096 samples, ``floor_span`` up to 1024 windows,
    ``avg_width`` and ``max_silence + 1`` up to 64."""
    return 2 <= int(window) <= 4096 and 0 <= int(floor_span) <= 1024 and 1 <= int(avg_width) <= 64 and 0 <= int(max_silence) <= 63


def vad_layout(lengths, window: int, device=None) -> VadLayout:
    """The index tables of the silence-trimming calls: utterance u is ``lengths[u]`` samples from the sum of the lengths
    before it and has ``lengths[u] // window`` windows.  ``lengths``: a Python list or CPU tensor.  Host arithmetic and one
    small upload; build it once for a captured graph."""
    ls, window = _int_list(lengths), int(window)
    if window < 1:
        raise ValueError("the window must be at least 1 sample")
    win_start, rows = _utterance_tables(ls, [n // window for n in ls], device)
    return VadLayout(*rows, win_start, ls, window)


def vad_detector_params(window: int, ratio_db: float, min_level_dbfs: float):
    """``(ratio_q8, min_energy)``: the integers ge2e_vad_flags compares with, from the detector's decibels."""
    return (int(round(10.0 ** (ratio_db / 10.0) * 256)),
            int(round(window * window * (32767.0 * 10.0 ** (min_level_dbfs / 20.0)) ** 2)))


def _vad_prologue(wav: torch.Tensor, lengths, window: int, layout: Optional[VadLayout]):
    """``(w, layout)`` of ``vad_flags`` and ``trim_silences``: the call's layout, built where None, and the checked wav."""
    if layout is None:
        layout = vad_layout([wav.numel()] if lengths is None else lengths, window, device=wav.device)
    elif layout.window != int(window):
        raise ValueError(f"layout was built for a window of {layout.window} samples, not {window}")
    w = _flat_wav(wav)
    _check_fits(layout.utt_start, layout.lengths, w)
    return w, layout


def _vad_window_index(lay: VadLayout):
    """Per window, on the device: the utterance it belongs to, its index there and its first sample."""
    counts = lay.win_start_dev[1:] - lay.win_start_dev[:-1]
    owner = torch.repeat_interleave(torch.arange(len(lay.lengths), device=counts.device), counts,
                                    output_size=lay.total_windows)
    local = torch.arange(lay.total_windows, device=counts.device) - lay.win_start_dev[owner]
    return owner, local, lay.utt_start[owner] + local * lay.window


def _vad_padded(values: torch.Tensor, lay: VadLayout, owner, local, fill):
    """(U, the longest utterance's windows): every utterance's per-window values in a row of its own, ``fill`` behind."""
    width = max(b - a for a, b in zip(lay.win_start, lay.win_start[1:]))
    m = torch.full((len(lay.lengths), width), fill, dtype=values.dtype, device=values.device)
    m[owner, local] = values
    return m


def _vad_window_sum(x: torch.Tensor, left: int, right: int) -> torch.Tensor:
    """Along the rows of x: the sum over [i - left, i + right], zeros outside."""
    c = torch.cumsum(torch.nn.functional.pad(x, (left + 1, right)), dim=1)
    return c[:, left + right + 1:] - c[:, :x.shape[1]]


def _vad_window_min(x: torch.Tensor, span: int, big: int) -> torch.Tensor:
    """Along the rows of x: the minimum over [i - span, i + span], ``big`` outside; log2(span) ``minimum`` passes."""
    K = 2 * span + 1
    m = torch.nn.functional.pad(x, (span, span), value=big)
    n, width = x.shape[1], 1
    while 2 * width <= K:
        m = torch.minimum(m[:, :-width], m[:, width:])
        width *= 2
    return torch.minimum(m[:, :n], m[:, K - width:K - width + n])


def _vad_flags_torch(w, lay: VadLayout, gain, span: int, ratio_q8: int, min_energy: int) -> torch.Tensor:
    """The same flags with torch's ops on wav's device, what a caller without the kernels would write: the windows as rows
    of an ``unfold`` view, the sums in int64, the sliding minimum by doubling, the 128-bit comparison as a division."""
    S = lay.window
    owner, local, first = _vad_window_index(lay)
    x = w.unfold(0, S, 1)[first]
    if gain is not None:
        x = x * gain[owner][:, None]
    r = torch.round(x * 32767.0)
    q = torch.nan_to_num(r, nan=0.0, posinf=32767.0, neginf=-32768.0).clamp(-32768.0, 32767.0).long()
    e = S * (q * q).sum(1) - q.sum(1) ** 2
    big = 1 << 62
    fl = _vad_window_min(_vad_padded(e, lay, owner, local, big), span, big)[owner, local]
    left = e * 256
    # left > fl * ratio without the product: fl <= (left - 1) // ratio
    above = (left > 0) & (fl <= torch.div(left - 1, max(ratio_q8, 1), rounding_mode="floor")) if ratio_q8 > 0 else left > 0
    return ((e >= min_energy) & above).to(torch.uint8)


def vad_flags(wav: torch.Tensor, lengths=None, gain: Optional[torch.Tensor] = None, *, window: int,
              floor_span: int = VAD_DEFAULTS["floor_span"], ratio_db: float = VAD_DEFAULTS["ratio_db"],
              min_level_dbfs: float = VAD_DEFAULTS["min_level_dbfs"], layout: Optional[VadLayout] = None,
              native: Optional[bool] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ge2e_vad_flags: one voice flag per window of ``window`` samples, (total_windows,) uint8 on wav's device, in two
    launches on the current stream.  This is the PROJECT'S OWN detector, not webrtcvad's: with the int16 value q of every
    sample (``round(x * gain * 32767)``, saturating) and e = S sum(q^2) - (sum q)^2 (S^2 times the window's variance), a
    window is voiced when its level is at least ``min_level_dbfs`` and more than ``ratio_db`` above the quietest window
    within ``floor_span`` windows of it in the same utterance.  All in integers: the kernel, the torch route
    (``native=False``) and ``tests/vad_ref.py`` agree to the bit.  ``wav`` flat float32, ``lengths`` as ``resample`` (None:
    one utterance), ``gain`` (U,) float32 on the device or None, ``layout`` a ``vad_layout`` built beforehand.
    ``native=None`` takes the kernels where they support the parameters (``vad_supported``) and the torch route otherwise;
    ``native=True`` raises there."""
    _require_cuda(wav, "wav")
    dev = wav.device
    w, layout = _vad_prologue(wav, lengths, window, layout)
    U, total, S = len(layout.lengths), layout.total_windows, layout.window
    gain = _check_gain(gain, U, dev)
    floor_span = int(floor_span)
    if floor_span < 0:
        raise ValueError("floor_span must not be negative")
    use_native = _use_native(native, vad_supported(S, floor_span), "vad_flags", lambda: f"window {S}, floor_span {floor_span}")
    ratio_q8, min_energy = vad_detector_params(S, ratio_db, min_level_dbfs)
    if total == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev)
    if not use_native:
        return _vad_flags_torch(w, layout, gain, floor_span, ratio_q8, min_energy)
    need = _lib.load().ge2e_vad_workspace_bytes(total, U)
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.int64, device=dev)
    elif workspace.device != dev or workspace.dtype != torch.int64 or not workspace.is_contiguous() or workspace.numel() * 8 < need:
        raise TypeError(f"workspace must be a contiguous torch.int64 tensor of {need // 8} elements on {dev}")
    flags = torch.empty(total, dtype=torch.uint8, device=dev)
    _launch("ge2e_vad_flags", dev, w.data_ptr(), layout.utt_start.data_ptr(), layout.utt_len.data_ptr(),
            None if gain is None else gain.data_ptr(), layout.win_start_dev.data_ptr(), U, total, S, floor_span, ratio_q8,
            min_energy, flags.data_ptr(), workspace.data_ptr(), _stream_ptr(w))
    return flags


def _vad_mask_torch(flags, lay: VadLayout, avg_width: int, max_silence: int):
    owner, local, _ = _vad_window_index(lay)
    A, n = avg_width, max_silence + 1
    f = _vad_padded((flags != 0).long(), lay, owner, local, 0)
    valid = _vad_padded(torch.ones_like(owner), lay, owner, local, 0)
    m = ((2 * _vad_window_sum(f, (A - 1) // 2, A // 2) > A) & (valid > 0)).long()
    keep = (_vad_window_sum(m, (n - 1) // 2, n // 2) > 0) & (valid > 0)
    rank = torch.cumsum(keep.long(), dim=1) - 1
    dst = torch.where(keep, rank, torch.full_like(rank, -1))[owner, local].to(torch.int32)
    return dst, keep.long().sum(1) * lay.window


def vad_mask(flags: torch.Tensor, layout: VadLayout, avg_width: int = 8, max_silence: int = 6, native: Optional[bool] = None):
    """ge2e_vad_mask: the reference's smoothing and dilation of the voice flags (its ``moving_average`` of width
    ``avg_width`` rounded half to even, scipy's ``binary_dilation`` with ``max_silence + 1`` ones) and the compaction's
    index, in one launch -> ``(dst, out_len_dev)``: ``dst`` (total_windows,) int32, the rank of a window among its
    utterance's kept windows or -1, and ``out_len_dev`` (U,) int64 on the device, the samples every utterance keeps.
    ``flags`` (total_windows,) uint8 or bool on the device: ``vad_flags``' or anyone's (webrtcvad's, a neural detector's),
    non-zero meaning voiced.  ``native`` as ``vad_flags``, with one change-over by size: ``native=None`` takes the torch
    route where an utterance has more than ``VAD_MASK_TORCH_FROM`` windows (the kernel walks an utterance in one
    workgroup; profiles/vad_bench.txt)."""
    _require_cuda(flags, "flags")
    dev = flags.device
    U, total = len(layout.lengths), layout.total_windows
    f = flags.detach()
    if f.dtype == torch.bool:
        f = f.to(torch.uint8)
    if f.dtype != torch.uint8 or tuple(f.shape) != (total,) or not f.is_contiguous() or layout.utt_start.device != dev:
        raise TypeError(f"flags must be a contiguous ({total},) uint8 or bool tensor on {layout.utt_start.device}")
    avg_width, max_silence = int(avg_width), int(max_silence)
    if avg_width < 1 or max_silence < 0:
        raise ValueError("avg_width must be at least 1 and max_silence at least 0")
    supported = vad_supported(layout.window, 0, avg_width, max_silence)
    longest = max(b - a for a, b in zip(layout.win_start, layout.win_start[1:]))
    use_native = _use_native(native, supported, "vad_mask", lambda: f"window {layout.window}, avg_width {avg_width}, "
                             f"max_silence {max_silence}", default=supported and longest <= VAD_MASK_TORCH_FROM)
    if total == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), torch.zeros(U, dtype=torch.int64, device=dev)
    if not use_native:
        return _vad_mask_torch(f, layout, avg_width, max_silence)
    dst = torch.empty(total, dtype=torch.int32, device=dev)
    out_len = torch.empty(U, dtype=torch.int64, device=dev)
    _launch("ge2e_vad_mask", dev, f.data_ptr(), layout.win_start_dev.data_ptr(), U, total, layout.window, avg_width,
            max_silence, dst.data_ptr(), out_len.data_ptr(), _stream_ptr(f))
    return dst, out_len


def trim_silences(wav: torch.Tensor, lengths=None, *, gain: Optional[torch.Tensor] = None, voice_flags=None, window: int,
                  floor_span: int = VAD_DEFAULTS["floor_span"], ratio_db: float = VAD_DEFAULTS["ratio_db"],
                  min_level_dbfs: float = VAD_DEFAULTS["min_level_dbfs"], avg_width: int = 8, max_silence: int = 6,
                  layout: Optional[VadLayout] = None, native: Optional[bool] = None):
    """The reference's ``trim_long_silences`` on the device -> ``(flat, out_lengths)`` as ``resample`` returns them:
    ``flat`` float32, the trimmed utterances back to back, and ``out_lengths`` a Python list of their sample counts.
    Every utterance is cut to whole windows of ``window`` samples (``vad_window_length * sampling_rate // 1000``), the
    windows get voice flags, the flags are smoothed and dilated (``vad_mask``) and the samples of the kept windows are
    copied, bits unchanged (``ge2e_vad_trim``).  ``gain`` (U,) scales the samples for the detector only, as the reference
    trims the normalised signal; the samples returned are wav's own, and the caller goes on passing ``gain`` to ``melspec``.
    ``voice_flags``: flags from elsewhere, (total_windows,) non-zero for voiced, utterance after utterance
    (``vad_layout(...).win_start`` says where); None: ``vad_flags``, the project's own detector -- NOT webrtcvad's, which
    the reference uses: pass webrtcvad's flags here to get the reference's trimming.

    ONE synchronisation: between the mask and the trim launch the U kept lengths (int64) are read back, because what comes
    next -- ``melspec``'s frame layout, the partial slices -- is host arithmetic on lengths.  Four launches otherwise (three
    with ``voice_flags``).  ``native=None`` takes the kernels where they support the parameters and torch ops otherwise
    (``unfold``, ``cumsum``, indexing: the same flags and the same bits).  Measured (profiles/vad_bench.txt) the kernels are
    the faster route at every size but one: the mask of a single utterance of more than ``VAD_MASK_TORCH_FROM`` windows
    (41 minutes), which ``native=None`` therefore leaves to torch's ops (``vad_mask``); the results are the same bits."""
    _require_cuda(wav, "wav")
    dev = wav.device
    w, layout = _vad_prologue(wav, lengths, window, layout)
    U, total, S = len(layout.lengths), layout.total_windows, layout.window
    if total == 0:
        return torch.empty(0, dtype=torch.float32, device=dev), [0] * U
    use_native = _use_native(native, vad_supported(S, floor_span if voice_flags is None else 0, avg_width, max_silence),
                             "trim_silences", lambda: f"window {S}, floor_span {floor_span}, avg_width {avg_width}, "
                             f"max_silence {max_silence}")
    if voice_flags is None:
        flags = vad_flags(w, gain=gain, window=S, floor_span=floor_span, ratio_db=ratio_db, min_level_dbfs=min_level_dbfs,
                          layout=layout, native=use_native)
    else:
        flags = (torch.as_tensor(voice_flags).reshape(-1) != 0).to(device=dev, dtype=torch.uint8)
        if flags.numel() != total:
            raise ValueError(f"voice_flags has {flags.numel()} entries; the utterances have {total} windows of {S} samples")
    dst, out_len = vad_mask(flags, layout, avg_width, max_silence, native=None if native is None else use_native)
    out_lengths = [int(v) for v in out_len.tolist()]           # the one read-back
    out = torch.empty(sum(out_lengths), dtype=torch.float32, device=dev)
    if out.numel() == 0:
        return out, out_lengths
    if not use_native:
        _, _, first = _vad_window_index(layout)
        return w.unfold(0, S, 1)[first[dst >= 0]].reshape(-1), out_lengths
    out_start = torch.tensor(list(accumulate(out_lengths[:-1], initial=0)), dtype=torch.int64).to(dev)
    _launch("ge2e_vad_trim", dev, w.data_ptr(), layout.utt_start.data_ptr(), layout.win_start_dev.data_ptr(), dst.data_ptr(),
            out_start.data_ptr(), U, total, S, out.data_ptr(), _stream_ptr(w))
    return out, out_lengths


SGD_CHUNK = _lib.MACROS["GE2E_SGD_CHUNK"]
SGD_MAX_GROUPS = _lib.MACROS["GE2E_SGD_MAX_GROUPS"]


class SgdLayout:
    """The tables of ``sgd_clip_step`` for a list of parameter groups (include/ge2e_hip.h, OPTIMIZER STEP): ``seg`` (S, 4)
    int64 -- address, offset in the flat gradient, numel, group of every tensor, sorted by group -- and ``chunk_start``
    (S + 1,) int32 on the tensors' device, with ``S``, ``C`` (chunks = workgroups of either launch) and ``G``.

    THE ADDRESSES ARE RAW.  The kernels write through ``seg`` whatever lives there now; a tensor whose storage was replaced
    (``p.data = ...``, ``module.to(...)``, ``load_state_dict(assign=True)``) leaves a stale address behind.  The ONLY defence
    is ``refresh()``: it compares every tensor's current ``data_ptr()`` with the table's and uploads the table again, in
    place, when one moved.  ``sgd_clip_step`` calls it on every call.  A caller who launches from the tables directly, or
    replays a captured graph, has to keep the storages alive and where they are -- or call ``refresh()`` before the replay:
    the table is rewritten in place, so a captured launch reads the new addresses.

    On CUDA the layout also owns what the call reuses from one step to the next: the workspace, the ``stats`` the call
    returns, and the counter of skipped steps."""

    def __init__(self, tensors, groups, offsets, G: int, device: torch.device):
        self.tensors, self.groups, self.offsets, self.G, self.device = tensors, groups, offsets, G, device
        self.S = len(tensors)
        self.extent = max(o + t.numel() for o, t in zip(offsets, tensors))      # elements of the flat gradient it reaches
        counts = [-(-t.numel() // SGD_CHUNK) for t in tensors]
        self.chunk_start_host = list(accumulate(counts, initial=0))
        self.C = self.chunk_start_host[-1]
        self.chunk_start = torch.tensor(self.chunk_start_host, dtype=torch.int32).to(device)
        self.ptrs = [t.data_ptr() for t in tensors]
        self.seg = self._table().to(device)
        self.workspace = self.stats = self.skipped = None
        if device.type == "cuda":
            with _on_device(device):
                need = int(_lib.load().ge2e_sgd_clip_workspace_bytes(self.C))
            self.workspace = alloc_workspace(need, device, init=False)
            self.stats = torch.zeros(G, 2, dtype=torch.float32, device=device)
            self.skipped = torch.zeros(1, dtype=torch.int32, device=device)

    def _table(self) -> torch.Tensor:
        return torch.tensor([[a, o, t.numel(), g] for a, o, t, g in zip(self.ptrs, self.offsets, self.tensors, self.groups)],
                            dtype=torch.int64)

    def refresh(self) -> bool:
        """Upload the table again if a tensor's storage moved; True if it did."""
        ptrs = [t.data_ptr() for t in self.tensors]
        if ptrs == self.ptrs:
            return False
        if self.device.type == "cuda" and _capturing is not None and _capturing():
            raise RuntimeError("a parameter's storage moved while the stream is being captured: refresh the layout before")
        self.ptrs = ptrs
        self.seg.copy_(self._table())
        return True


def sgd_layout(groups, flat_grad_offsets) -> SgdLayout:
    """The tables of ``sgd_clip_step``.  ``groups``: up to 8 lists of tensors (the parameter groups: one gradient norm, one
    ``hyper`` row each); ``flat_grad_offsets``: lists of the same lengths, the element offset of each tensor's gradient in
    the flat gradient (and in the momentum buffer).  Every tensor must be float32, contiguous and on one device, and appear
    once; an empty tensor has nothing to update and is left out.  Works on CPU tensors too (the tables, for inspection; the
    call itself needs the GPU).  Host arithmetic and two small uploads: build it once.  See ``SgdLayout`` on stale
    addresses."""
    groups = [list(g) for g in groups]
    offsets = [_int_list(o) for o in flat_grad_offsets]
    if not 1 <= len(groups) <= SGD_MAX_GROUPS:
        raise ValueError(f"1 .. {SGD_MAX_GROUPS} parameter groups, got {len(groups)}")
    if len(offsets) != len(groups) or any(len(o) != len(g) for o, g in zip(offsets, groups)):
        raise ValueError("flat_grad_offsets must name one offset per tensor, group by group")
    tensors, owner, offs, seen, dev = [], [], [], set(), None
    for gi, (g, o) in enumerate(zip(groups, offsets)):
        for t, off in zip(g, o):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise TypeError(f"group {gi}: float32 tensors only, got {getattr(t, 'dtype', type(t))}")
            if id(t) in seen:
                raise ValueError(f"group {gi}: a tensor appears twice (it would be updated twice)")
            seen.add(id(t))
            if dev is None:
                dev = t.device
            if t.device != dev:
                raise ValueError(f"group {gi}: every tensor on one device (got {t.device} beside {dev})")
            if not t.is_contiguous():
                raise ValueError(f"group {gi}: a parameter that is not contiguous has no flat range to update")
            if off < 0:
                raise ValueError(f"group {gi}: negative offset {off}")
            if t.numel() == 0:
                continue
            tensors.append(t)
            owner.append(gi)
            offs.append(off)
    if not tensors:
        raise ValueError("nothing to update: no tensor with elements")
    return SgdLayout(tensors, owner, offs, len(groups), dev)


def sgd_clip_step(layout: SgdLayout, grad: torch.Tensor, hyper: torch.Tensor, momentum: Optional[torch.Tensor] = None,
                  grad_scale: float = 1.0, zero_grad: bool = False, skip_nonfinite: bool = False):
    """``clip_grad_norm_`` per group, then ``torch.optim.SGD.step``, for every tensor of ``layout`` in two HIP launches
    (ge2e_sgd_clip_step; the arithmetic, operation by operation, is in include/ge2e_hip.h).  ``grad``: the flat float32
    gradient the layout's offsets index; it is left holding the clipped gradients, or zeros with ``zero_grad``.  ``hyper``
    (G, 4) float32 on the device: ``lr, max_norm, weight_decay, momentum`` per group, read by the launches -- write a new
    learning rate into it and the next call (or replay) uses it.  ``momentum``: the momentum buffer, shaped as ``grad``
    (zeros before the first step), or None.  ``grad_scale`` multiplies every gradient before the norm (1 / world size).
    ``skip_nonfinite``: a step in which any group's norm is inf or NaN leaves parameters and momentum untouched and counts.

    Returns ``stats`` (G, 2) -- the norm before the clip and the coefficient applied, per group -- and with
    ``skip_nonfinite`` ``(stats, skipped)``, the int32 count of skipped steps so far.  Both belong to the layout and are
    overwritten by the next call; nothing is allocated and nothing waits for the device.  The layout is refreshed first
    (``SgdLayout.refresh``): the only defence against a parameter whose storage moved."""
    _require_cuda(grad, "grad")
    dev = grad.device
    if layout.device != dev:
        raise RuntimeError(f"the layout's tensors are on {layout.device}, grad on {dev}")
    need = layout.extent
    for name, t in (("grad", grad), ("momentum", momentum)):
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() < need:
            raise ValueError(f"{name} must be a contiguous float32 tensor of at least {need} elements on {dev}")
    if hyper.dtype != torch.float32 or hyper.device != dev or not hyper.is_contiguous() or tuple(hyper.shape) != (layout.G, 4):
        raise ValueError(f"hyper must be a contiguous float32 ({layout.G}, 4) tensor on {dev}")
    layout.refresh()
    flags = (_lib.MACROS["GE2E_SGD_FLAG_ZERO_GRAD"] if zero_grad else 0) | \
        (_lib.MACROS["GE2E_SGD_FLAG_SKIP_NONFINITE"] if skip_nonfinite else 0)
    _launch("ge2e_sgd_clip_step", dev, layout.seg.data_ptr(), layout.chunk_start.data_ptr(), layout.S, layout.C, layout.G,
            grad.data_ptr(), _ptr(momentum), hyper.data_ptr(), float(grad_scale), flags, layout.stats.data_ptr(),
            layout.skipped.data_ptr() if skip_nonfinite else None, layout.workspace.data_ptr(), layout.workspace.numel(),
            _stream_ptr(grad))
    return (layout.stats, layout.skipped) if skip_nonfinite else layout.stats


def sgd_clip_plan(layout: SgdLayout, has_momentum: bool = False) -> list:
    """Diagnostics: the two launches of ``sgd_clip_step`` for this layout, ``["sgd_sqsum/4096/C", "sgd_update<mom>/4096/C"]``."""
    return _lib._plan(_lib.load().ge2e_sgd_clip_plan, layout.S, layout.C, layout.G, int(has_momentum), 0)


def raw_supported(N: int, M: int, D: int) -> bool:
    """Shapes ge2e_loss_raw runs as ONE launch (the one-wave-per-batch kernel's register-only shapes)."""
    return bool(_lib.load().ge2e_raw_supported(N, M, D))


class _GE2ELossRawFunction(torch.autograd.Function):
    """loss(normalize(y)[unperm].view(N,M,D)) and dL/dy in ONE launch (ge2e_loss_fwd_bwd_raw)."""

    @staticmethod
    def forward(ctx, y, src, w, b, N, M, eps, eps_cos, variant, unverified=False):
        rows, D = y.shape
        need = any(ctx.needs_input_grad[i] for i in (0, 2, 3))
        sc = torch.empty(3, dtype=torch.float32, device=y.device)    # loss | dw | db
        dY = (torch.zeros_like(y) if unverified else torch.empty_like(y)) if need else None
        _launch("ge2e_loss_fwd_bwd_raw", y.device,
                y.data_ptr(), src.data_ptr() if src is not None else None, 1, N, M, D, w.data_ptr(), b.data_ptr(),
                eps_cos, eps, _lib.VARIANTS[variant], sc.data_ptr(), None, dY.data_ptr() if need else None,
                sc.data_ptr() + 4 if need else None, sc.data_ptr() + 8 if need else None, _stream_ptr(y))
        ctx.w_shape, ctx.b_shape = w.shape, b.shape
        if need:
            ctx.save_for_backward(dY, sc)
        return sc[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        dY, sc = ctx.saved_tensors
        rows, D = dY.shape
        gY, gw, gb = _scale_grads(dY, sc.data_ptr() + 4, sc.data_ptr() + 8, grad_out, 1, (1, rows, 1, D),
                                  [ctx.needs_input_grad[i] for i in (0, 2, 3)], ctx.w_shape, ctx.b_shape)
        return gY, None, gw, gb, None, None, None, None, None, None


def ge2e_loss_raw(y: torch.Tensor, unperm, w: torch.Tensor, b: torch.Tensor, shape, *, eps: float = SMALL_ERR,
                  eps_cos: float = EPS_COS, variant: str = "softmax") -> torch.Tensor:
    """``GE2ELoss(normalize(y)[unperm].reshape(N, M, D))`` for the encoder's raw projection ``y`` (rows, D) -- s2:34,
    s4:186-189 and s3:19-30 -- as ONE launch that also yields dL/dy.  ``shape`` = (N, M); shapes outside
    ``raw_supported`` take the two-kernel route (normalize_unperm, then ge2e_loss)."""
    _require_cuda(y, "y")
    if y.dim() != 2:
        raise ValueError(f"y must be (rows, D), got {tuple(y.shape)}")
    N, M = int(shape[0]), int(shape[1])
    if N * M != y.shape[0]:
        raise ValueError(f"shape {tuple(shape)} does not match {y.shape[0]} rows")
    if not raw_supported(N, M, y.shape[1]):
        return ge2e_loss(normalize_unperm(y, unperm, shape=(N, M)), w, b, eps=eps, eps_cos=eps_cos, variant=variant)
    src = _unperm_index(unperm, y.shape[0], y.device)
    _check_scalar_params(w, b, y.device)
    y = y.contiguous().float()
    if y.data_ptr() % 16:          # a contiguous view at an odd storage offset: the kernels load 16 bytes per lane
        y = y.clone()
    return _GE2ELossRawFunction.apply(y, src, w, b, N, M, float(eps), float(eps_cos), variant, _index_is_unverified(unperm))


def eer_counts(sim_matrix: torch.Tensor, thresholds) -> torch.Tensor:
    """Integer counts of the calculate_ERR sweep (s5:57-98) for (N,M,N) or (B,N,M,N) similarities:
    -> int32 (T,2) or (B,T,2): [...,0] false accepts (s5:82), [...,1] accepts on the own column (s5:89).
    ``thresholds``: non-decreasing, compared in fp32 as numpy does for a float32 array (s5:58)."""
    _require_cuda(sim_matrix, "sim_matrix")
    s = sim_matrix
    squeeze = s.dim() == 3
    if squeeze:
        s = s.unsqueeze(0)
    if s.dim() != 4 or s.shape[1] != s.shape[3]:
        raise ValueError(f"sim_matrix must be (N,M,N) or (B,N,M,N), got {tuple(sim_matrix.shape)}")
    s = s.contiguous().float()
    thr = _threshold_table(thresholds, s.device, device_ok=False)
    B, N, M, _ = s.shape
    T = thr.numel()
    counts = torch.empty(B, T, 2, dtype=torch.int32, device=s.device)
    _launch("ge2e_eer_counts", s.device, s.data_ptr(), B, N, M, thr.data_ptr(), T, counts.data_ptr(), _stream_ptr(s))
    return counts[0] if squeeze else counts


def _scale_grads(dE, dw_ptr: int, db_ptr: int, g, g_count: int, dims: tuple, needs, w_shape, b_shape):
    """The backward of every fp32 loss node, one launch: gE = g dE, gw = sum g dw, gb = sum g db (no host sync; out of place,
    so a retained graph may run again).  ``dE`` and the device scalars at ``dw_ptr`` / ``db_ptr`` are what the forward
    launch left; ``g`` is the incoming gradient, ``g_count`` (1 or B) values; ``dims`` = (B, N, M, D); ``needs`` says
    which of (gE, gw, gb) to produce, the others are None.  gw / gb come back in the parameters' own shapes."""
    if g.dtype != torch.float32 or not g.is_contiguous():
        g = g.to(torch.float32).contiguous()
    need_e, need_w, need_b = needs
    gE = torch.empty_like(dE) if need_e else None
    gwb = torch.empty(2, dtype=torch.float32, device=dE.device) if (need_w or need_b) else None
    _launch("ge2e_scale_grads", dE.device, dE.data_ptr(), dw_ptr, db_ptr, g.data_ptr(), g_count, *dims,
            gE.data_ptr() if need_e else None, gwb.data_ptr() if need_w else None,
            gwb.data_ptr() + 4 if need_b else None, _stream_ptr(dE))
    gw = (gwb[0] if len(w_shape) == 0 else gwb[0].reshape(w_shape)) if need_w else None
    gb = (gwb[1] if len(b_shape) == 0 else gwb[1].reshape(b_shape)) if need_b else None
    return gE, gw, gb


def _loss_node_forward(ctx, embeddings, w, b, eps, eps_cos, variant, impl):
    """forward of both loss nodes (the launch follows the embeddings' dtype): one fused kernel launch that also produces
    dE, dw, db, kept for the backward."""
    need = any(ctx.needs_input_grad[:3])
    squeeze = embeddings.dim() == 3
    # (no .detach(): inside Function.forward nothing is recorded, and only the data pointers cross the boundary)
    o = loss_fwd_bwd(embeddings, w, b, eps=eps, eps_cos=eps_cos, variant=variant, impl=impl, need_grad=need)
    ctx.squeeze = squeeze
    ctx.w_shape, ctx.b_shape = w.shape, b.shape
    if need:
        ctx.save_for_backward(o.dE, o.dw, o.db)
    return o.loss[0] if squeeze else o.loss


class _GE2ELossFunction(torch.autograd.Function):
    """forward = one fused kernel launch that also produces dE, dw, db;
    backward only scales them by the incoming gradient (no host sync)."""

    forward = staticmethod(_loss_node_forward)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        dE, dw, db = ctx.saved_tensors
        # grad_out: 0-dim or (B,)
        gE, gw, gb = _scale_grads(dE, dw.data_ptr(), db.data_ptr(), grad_out, grad_out.numel(), dE.shape,
                                  ctx.needs_input_grad[:3], ctx.w_shape, ctx.b_shape)
        if gE is not None and ctx.squeeze:
            gE = gE[0]
        return gE, gw, gb, None, None, None, None


class _GE2ELossF64Function(torch.autograd.Function):
    """The same node over ge2e_loss_fwd_bwd_f64: float64 embeddings, w, b in, float64 loss and gradients out.  The
    upstream gradient is applied in float64 (a handful of elementwise torch ops on the launch's own dE / dw / db)."""

    forward = staticmethod(_loss_node_forward)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        dE, dw, db = ctx.saved_tensors
        g = grad_out.to(torch.float64).reshape(-1)               # (1,) for a 0-dim loss, (B,) for a stack
        need_e, need_w, need_b = ctx.needs_input_grad[:3]
        gE = gw = gb = None
        if need_e:
            gE = dE * g.view(-1, 1, 1, 1)
            if ctx.squeeze:
                gE = gE[0]
        if need_w:
            gw = (dw * g).sum().reshape(ctx.w_shape)
        if need_b:
            gb = (db * g).sum().reshape(ctx.b_shape)
        return gE, gw, gb, None, None, None, None


class _GE2ELossRowsFunction(torch.autograd.Function):
    """The same node over the ragged kernel's three entry points: embeddings (R,D) / (B,R,D) and the device table of
    ``launch`` in -- `loss_fwd_bwd_ragged` with offsets, or `loss_fwd_bwd_labeled` with labels and its ``num_speakers`` /
    ``masked`` bound (functools.partial).  The masked launch's `active` (int32, not differentiable) comes out behind the
    loss.  dE is in the caller's row order, 0 on the rows that do not count; the backward scales the launch's own dE / dw /
    db by the incoming gradient with ge2e_scale_grads (a batch of R rows as N = 1, M = R)."""

    @staticmethod
    def forward(ctx, embeddings, table, w, b, eps, eps_cos, variant, launch):
        need = any(ctx.needs_input_grad[i] for i in (0, 2, 3))
        o = launch(embeddings, table, w, b, eps=eps, eps_cos=eps_cos, variant=variant, need_grad=need)
        ctx.squeeze = embeddings.dim() == 2
        ctx.w_shape, ctx.b_shape = w.shape, b.shape
        if need:
            ctx.save_for_backward(o.dE, o.dw, o.db)
        loss = o.loss[0] if ctx.squeeze else o.loss
        if o.active is None:
            return loss
        active = o.active[0] if ctx.squeeze else o.active
        ctx.mark_non_differentiable(active)
        return loss, active

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out, *_grad_active):
        dE, dw, db = ctx.saved_tensors
        B, R, D = dE.shape
        gE, gw, gb = _scale_grads(dE, dw.data_ptr(), db.data_ptr(), grad_out, grad_out.numel(), (B, 1, R, D),
                                  [ctx.needs_input_grad[i] for i in (0, 2, 3)], ctx.w_shape, ctx.b_shape)
        if gE is not None and ctx.squeeze:
            gE = gE[0]
        return gE, None, gw, gb, None, None, None, None


# The autograd node in C++ (libge2e_torch.so,csrc_torch/ge2e_autograd.cpp: torch.ops.ge2e_amd.loss): the same two C-ABI
# calls as _GE2ELossFunction without the Python dispatch around them -- the eager module step at B = 1 is host-bound.
# Used when the library has been built (build.build() does); _GE2ELossFunction is the same node in Python.
_cpp_node = {"tried": False, "op": None, "enabled": True}


def _cpp_loss_op():
    if not _cpp_node["tried"]:
        _cpp_node["tried"] = True
        import os
        import warnings
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libge2e_torch.so")
        # libge2e_torch.so is linked (rpath $ORIGIN) against the IN-TREE libge2e_hip.so: with GE2E_HIP_LIB pointing somewhere
        # else (A/B runs of two libraries) the node would launch the wrong library's kernels -- the Python node is used then
        if os.path.exists(path) and not os.environ.get("GE2E_HIP_LIB"):
            _lib.load()                                   # the core library first: missing -> the loud error, not a dlopen one
            try:
                torch.ops.load_library(path)
                _cpp_node["op"] = torch.ops.ge2e_amd.loss
            except (OSError, RuntimeError) as ex:         # built against another torch / a relinked core library
                warnings.warn(f"libge2e_torch.so could not be loaded ({str(ex)[:120]}); using the Python autograd node "
                              f"(same launches).  Rebuild with `python -m speaker_embedding_ge2e_loss_amd.build --force`.")
    return _cpp_node["op"] if _cpp_node["enabled"] else None


def cpp_node_workspace(like: torch.Tensor):
    """The workspace the C++ autograd node keeps for `like`'s device and the current stream (None when it has none, or when
    the node is not in use): for `workspace_fallback_count`."""
    if _cpp_loss_op() is None:
        return None
    ws = torch.ops.ge2e_amd.cached_workspace(like)
    return ws if ws.numel() > 0 else None


def use_cpp_autograd(enabled: bool) -> None:
    """Choose between the C++ autograd node (default when libge2e_torch.so is built) and the Python one (same launches)."""
    _cpp_node["enabled"] = bool(enabled)


def ge2e_loss(embeddings: torch.Tensor, w: torch.Tensor, b: torch.Tensor, *, eps: float = SMALL_ERR,
              eps_cos: float = EPS_COS, variant: str = "softmax", impl: str = "auto") -> torch.Tensor:
    """Differentiable GE2E loss: 0-dim for (N,M,D) input, (B,) for (B,N,M,D)."""
    _require_cuda(embeddings, "embeddings")
    in_dtype = embeddings.dtype
    # The dtype contract.  The reference is dtype-generic (s3:19-30 computes in whatever dtype the embeddings have and
    # returns it).  Here:
    #   float32           native: the fp32 kernels;
    #   float64           native with impl="auto": the double-precision kernel (ge2e_loss_fwd_bwd_f64), float64 loss and
    #                     gradients.  w and b may be float32 (the module's parameters: the reference's `self.w * cos`
    #                     promotes) or float64; the cast is a differentiable torch op, so each leaf's gradient comes
    #                     back in the leaf's own dtype.  An explicit impl names an fp32 kernel and takes the cast route;
    #   float16/bfloat16  computed in fp32, the casts either side are differentiable torch ops.
    # (The static helpers -- cos_sim, calc_loss, centroids, ... -- compute in fp32 whatever they are given.)
    if in_dtype == torch.float64 and impl == "auto":
        return _GE2ELossF64Function.apply(embeddings, w.to(torch.float64), b.to(torch.float64), float(eps),
                                          float(eps_cos), variant, impl)
    if in_dtype != torch.float32:
        embeddings = embeddings.float()
    op = None if _ws_override else _cpp_loss_op()         # (a caller-owned workspace -- a graph capture -- goes through Python)
    if op is not None:
        loss = op(embeddings, w, b, float(eps), float(eps_cos), _lib.VARIANTS[variant], _lib.IMPLS[impl])
    else:
        loss = _GE2ELossFunction.apply(embeddings, w, b, float(eps), float(eps_cos), variant, impl)
    return loss if in_dtype == torch.float32 else loss.to(in_dtype)


def _rows_loss_input(embeddings: torch.Tensor, who: str, instead: str):
    """What `ge2e_loss_ragged` and `ge2e_loss_labeled` do to their embeddings first: float64 is refused (``who`` and
    ``instead`` word the message), float16 / bfloat16 are cast up (a differentiable torch op), a view at an odd storage
    offset is copied.  Returns the fp32 embeddings, the caller's dtype, B and R."""
    if embeddings.dtype == torch.float64:
        raise NotImplementedError(f"{who}: float64 embeddings are not implemented (the ragged kernel is fp32 and nothing "
                                  f"casts float64 down silently); pass float32, or {instead} for ge2e_loss")
    _require_cuda(embeddings, "embeddings")
    in_dtype = embeddings.dtype
    if in_dtype != torch.float32:
        embeddings = embeddings.float()
    _, _, (B, R, _), _ = _as_rows(embeddings)
    if embeddings.data_ptr() % 16:     # a contiguous view at an odd storage offset
        embeddings = embeddings.clone()
    return embeddings, in_dtype, B, R


def ge2e_loss_ragged(embeddings: torch.Tensor, counts, w: torch.Tensor, b: torch.Tensor, *, eps: float = SMALL_ERR,
                     eps_cos: float = EPS_COS, variant: str = "softmax") -> torch.Tensor:
    """Differentiable GE2E loss of speakers with DIFFERENT utterance counts: 0-dim for (R, D) input, (B,) for (B, R, D).

    ``embeddings`` holds the rows of speaker 0, then speaker 1, ... (what concatenating each speaker's utterances
    gives); ``counts`` says how many each has: (N,) for every batch alike or (B, N), a sequence or an integer CPU tensor,
    every count >= 2, each row summing to R.  They are validated on the host and uploaded once (the last few tables are
    kept, keyed by their contents).  A ``torch.int32`` DEVICE tensor is taken as the OFFSETS (N+1,) / (B, N+1) instead --
    0, m_0, m_0 + m_1, ..., R -- as is and UNVERIFIED (checking would cost a synchronisation): the kernel clamps what it
    reads, so a broken table gives wrong numbers, not a wild access.  With all counts equal to M this is
    ``ge2e_loss(embeddings.view(N, M, D))``.  float16 / bfloat16 are computed in fp32 behind differentiable casts;
    float64 is not implemented (there is no fp64 ragged kernel, and no silent fp32 arithmetic in its place)."""
    embeddings, in_dtype, B, R = _rows_loss_input(embeddings, "ge2e_loss_ragged", "pad to equal counts")
    with _on_device(embeddings.device):
        off = _ragged_offsets_on_device(counts, B, R, embeddings.device)
    loss = _GE2ELossRowsFunction.apply(embeddings, off, w, b, float(eps), float(eps_cos), variant, loss_fwd_bwd_ragged)
    return loss if in_dtype == torch.float32 else loss.to(in_dtype)


def ge2e_loss_labeled(embeddings: torch.Tensor, labels, w: torch.Tensor, b: torch.Tensor, *,
                      num_speakers: Optional[int] = None, eps: float = SMALL_ERR, eps_cos: float = EPS_COS,
                      variant: str = "softmax", masked: Optional[bool] = None, return_active: bool = False,
                      wide: bool = False):
    """Differentiable GE2E loss of rows in ANY order with one speaker label each: 0-dim for (R, D) input, (B,) for
    (B, R, D).  What `ge2e_loss_ragged` computes on the rows sorted by speaker (stable), with the embeddings' gradient in
    the caller's row order; nothing is sorted or copied on the way: the index kernel orders the rows on the device and the
    loss kernel gathers as it loads.

    ``labels`` (R,) for every batch alike or (B, R).  On the HOST -- a sequence or an integer CPU tensor -- the ids are
    arbitrary integers: every batch is compacted to dense ids by ascending id, validated (at least 2 rows per speaker, the
    same number of speakers in every batch) and uploaded once (the last few tables are kept, keyed by their contents).
    On the DEVICE -- torch.int32 or torch.int64 -- they are taken as dense ids in [0, num_speakers), as is and UNVERIFIED
    (checking would cost a synchronisation), and ``num_speakers`` must be given: the kernel clamps what it reads, so broken
    labels give wrong numbers, not a wild access.  float16 / bfloat16 are computed in fp32 behind differentiable casts;
    float64 is not implemented (there is no fp64 ragged kernel, and no silent fp32 arithmetic in its place).

    ``masked=True`` takes the batch as it is (ge2e_loss_fwd_bwd_labeled_masked): ``num_speakers`` is an upper bound of the
    ids (the data set's speaker count works; required for device labels), a row whose label is outside [0, num_speakers)
    -- on the host: negative -- is ignored, and a speaker left with fewer than 2 rows is left out, rows and centroid
    alike.  Device labels may hold any values; host labels may hold lone speakers and a different number of speakers per
    batch.  Everything is decided on the device, without a synchronisation.  The rows that do not count are never read
    and get a zero gradient; a batch in which nothing counts has loss 0.  ``return_active=True`` (with ``masked``) returns
    ``(loss, active)``: active (2,) / (B, 2) int32 on the device, not differentiable, holds the numbers of speakers and
    of rows that counted, so ``loss / active[..., 1].clamp(min=1)`` is the mean over those rows.

    ``wide=True`` computes the masked loss (``masked`` is implied) with ge2e_loss_fwd_bwd_labeled_wide, many workgroups per
    batch: for few, large batches (`loss_fwd_bwd_labeled`)."""
    masked = _masked_for(masked, wide)
    if return_active and not masked:
        raise ValueError("return_active needs masked=True: without masking every row counts")
    embeddings, in_dtype, B, R = _rows_loss_input(embeddings, "ge2e_loss_labeled", "group equal counts")
    with _on_device(embeddings.device):
        lab, N = _labels_on_device(labels, num_speakers, B, R, embeddings.device, masked)
    launch = functools.partial(loss_fwd_bwd_labeled, num_speakers=N, masked=masked, wide=wide)
    res = _GE2ELossRowsFunction.apply(embeddings, lab, w, b, float(eps), float(eps_cos), variant, launch)
    loss, active = res if masked else (res, None)
    loss = loss if in_dtype == torch.float32 else loss.to(in_dtype)
    return (loss, active) if return_active else loss
