"""GE2ELoss(hp, graph=True) -- loss.py's _forward_graphed over graphed.StaticLossStep, the route the README recommends for a
training step -- where its correctness depends on state kept across calls: the team kernel's control block under graph
replay, the device the capture runs on, the autograd contract of the ``loss.backward()`` shortcut, and the default random
generator.  Every number is held to the fp64 closed form (dense_harness.check_dense, strict); where bits are the claim, to the
eager module or an eager launch too -- never to the graph route alone."""
import os
import socket

import numpy as np
import pytest
import torch

from capi import functional as GF  # noqa: F401
from dense_harness import check_dense
from oracle import ge2e_oracle as orc

pytestmark = pytest.mark.gpu

CTL_BYTES = 2048        # sizeof(TeamCtl), csrc/ge2e_team.hpp: the control block at the head of a team workspace


def _fp64(E, w, b, impl, what, loss, dE=None, dw=None, db=None, per=None):
    """check_dense() against closed_form(E, w, b) in fp64, strict.  A route that does not produce a quantity (the graph route has no
    per-row losses; a forward-only launch no gradients; DDP keeps dE inside the encoder's backward) passes the oracle's own
    value for it, so that only what the route produced is under test."""
    ref = orc.closed_form(np.asarray(E, np.float64), float(w), float(b))
    cpu = lambda t, k: ref[k] if t is None else t.detach().double().cpu().numpy()  # noqa: E731
    check_dense({"loss": cpu(loss, "loss"), "per": cpu(per, "per"), "dE": cpu(dE, "dE"), "dw": cpu(dw, "dw"), "db": cpu(db, "db")},
                ref, impl, what, strict=True)


def _inputs(shape, seed, k):
    return [orc.synth_embeddings(shape, "unit", seed=seed + i) for i in range(k)]


# ---- A. the team kernel's control block under graph replay ---------------------------------------------------------------

class _ModuleRoute:
    """GE2ELoss(hp, graph=True): call 0 eager, call 1 captures StaticLossStep and replays it, later calls replay."""

    def __init__(self, dev, shape):
        from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
        self.mod = GE2ELoss(HParams(device=dev), impl="team", graph=True)
        self.dev = dev

    def __call__(self, E):
        e = torch.as_tensor(E, device=self.dev).requires_grad_(True)
        self.mod.zero_grad(set_to_none=True)
        loss = self.mod(e)
        loss.backward()
        return {"loss": loss.detach().clone(), "dE": e.grad.clone(), "dw": self.mod.w.grad.clone(), "db": self.mod.b.grad.clone()}

    def workspace(self):
        assert len(self.mod._steps) == 1
        return next(iter(self.mod._steps.values())).workspace


class _DirectRoute:
    """graphed.GraphedLossStep(module, shape, direct=True): the fused launch captured alone."""

    def __init__(self, dev, shape):
        from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
        from speaker_embedding_ge2e_loss_amd.graphed import GraphedLossStep
        self.mod = GE2ELoss(HParams(device=dev), impl="team")
        self.step = GraphedLossStep(self.mod, shape, direct=True)
        self.dev = dev

    def __call__(self, E):
        loss = self.step(torch.as_tensor(E, device=self.dev))
        return {"loss": loss.clone(), "dE": self.step.input_grad.clone(), "dw": self.mod.w.grad.clone(),
                "db": self.mod.b.grad.clone()}

    def workspace(self):
        return self.step.workspace


class _ForwardRoute:
    """A caller's own capture (graphed.py: every launch of the library is capture-safe) of a forward-only team launch:
    loss and per-row losses, no gradients -- the pipelined forward kernel (ge2e_team_fwd.hip)."""

    def __init__(self, dev, shape, GF):
        n, m, d = shape
        self.GF, self.dev = GF, dev
        self.w, self.b = torch.tensor(10.0, device=dev), torch.tensor(-5.0, device=dev)
        self.x = torch.as_tensor(orc.synth_embeddings((1, n, m, d), "unit", seed=77), device=dev)
        self.ws = GF.alloc_workspace(GF.workspace_bytes(1, n, m, d, "softmax", "team"), dev)
        self.out = GF.LossOutputs(loss=torch.empty(1, device=dev), per=torch.empty(1, n, m, device=dev), dE=None, dw=None,
                                  db=None)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                self._launch()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self._launch()

    def _launch(self):
        self.GF.loss_fwd_bwd(self.x, self.w, self.b, impl="team", need_grad=False, need_per=True, out=self.out,
                             workspace=self.ws)

    def __call__(self, E):
        self.x.copy_(torch.as_tensor(E, device=self.dev).unsqueeze(0))
        self.graph.replay()
        return {"loss": self.out.loss[0].clone(), "per": self.out.per[0].clone()}

    def workspace(self):
        return self.ws


@pytest.mark.parametrize("route", ["module", "direct", "forward"])
@pytest.mark.parametrize("shape", [(64, 10, 256), (40, 7, 80)], ids=["metric", "padded_D"])
def test_replays_after_an_untrusted_control_block(GF, shape, route):
    """Capture, replay once, then write 0xA5 over the step's own control block (as another implementation would) and replay
    five times more on new inputs.  The first of those replays finds no magic word and is redone without counters -- ONE redo:
    from the next replay on the team kernel must run again, i.e. give the bits of an eager team launch on a clean workspace
    (team output is bitwise repeatable; the redo's are other bits).  A graph replays the kernel arguments it captured, so a
    launch number taken from them cannot tell one replay from the next.  Every replay is held to fp64, and the workspace's
    fall-back count goes up by exactly one."""
    dev = torch.device("cuda:0")
    n, m, d = shape
    assert GF.resolve_impl(1, n, m, d, "softmax", "team") == "team"
    r = {"module": _ModuleRoute, "direct": _DirectRoute}.get(route)
    r = r(dev, shape) if r is not None else _ForwardRoute(dev, shape, GF)
    fwd = route == "forward"
    w, b = torch.tensor(10.0, device=dev), torch.tensor(-5.0, device=dev)
    clean = GF.alloc_workspace(GF.workspace_bytes(1, n, m, d, "softmax", "team"), dev)
    Es = _inputs(shape, 900 + n, 8)
    for E in Es[:2]:                                          # (module route: eager call, then capture + first replay)
        r(E)
    ws = r.workspace()
    torch.cuda.synchronize()
    c0 = GF.workspace_fallback_count(ws)
    ws[:CTL_BYTES].fill_(0xA5)                                # on the current stream: between two replays
    for k, E in enumerate(Es[2:]):
        o = r(E)
        ref = GF.loss_fwd_bwd(torch.as_tensor(E, device=dev), w, b, impl="team", need_grad=not fwd, need_per=fwd,
                              workspace=clean)
        torch.cuda.synchronize()
        what = f"{route} {shape} replay {k} after the corruption"
        if fwd:
            _fp64(E, 10.0, -5.0, "team", what, o["loss"], per=o["per"])
        else:
            _fp64(E, 10.0, -5.0, "team", what, o["loss"], dE=o["dE"], dw=o["dw"], db=o["db"])
        assert GF.workspace_fallback_count(ws) == c0 + 1, (what, GF.workspace_fallback_count(ws), c0)
        if k == 0:
            continue                                          # the one replay the redo may compute
        assert torch.equal(o["loss"], ref.loss[0]), (what, float(o["loss"]), float(ref.loss[0]))
        if fwd:
            assert torch.equal(o["per"], ref.per[0]), what
        else:
            assert torch.equal(o["dE"], ref.dE[0]), what
            assert torch.equal(o["dw"].reshape(()), ref.dw[0]) and torch.equal(o["db"].reshape(()), ref.db[0]), what
    assert GF.workspace_fallback_count(clean) == 0


# ---- B. the capture runs on the module's device ---------------------------------------------------------------------------

def test_capture_on_a_device_that_is_not_current(GF):
    """The module and its input on cuda:1 while cuda:0 is current, after a capture on cuda:0 has created torch's default
    capture stream there: a capture that went to that stream would record nothing (torch only warns), and from the third
    call on the module would hand out the warm-up launch's loss and gradients."""
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs two GPUs (module on cuda:1 while cuda:0 is current); this machine has {torch.cuda.device_count()}")
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams

    torch.cuda.set_device(0)
    x0 = torch.zeros(16, device="cuda:0")
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0):                                # torch's default capture stream, created on cuda:0
        x0.add_(1.0)
    g0.replay()
    dev = torch.device("cuda:1")
    mod = GE2ELoss(HParams(device=dev), graph=True)
    shape = (64, 10, 256)
    for it, E in enumerate(_inputs(shape, 1100, 6)):
        e = torch.as_tensor(E, device=dev).requires_grad_(True)
        mod.zero_grad(set_to_none=True)
        loss = mod(e)
        loss.backward()
        torch.cuda.synchronize(dev)
        assert torch.cuda.current_device() == 0
        assert (len(mod._steps) == 1) == (it >= 1), it
        _fp64(E, 10.0, -5.0, "auto", f"cuda:1 call {it}", loss, dE=e.grad, dw=mod.w.grad, db=mod.b.grad)
    assert float(x0[0]) == 1.0


# ---- C. the autograd contract of the loss.backward() shortcut -------------------------------------------------------------

@pytest.fixture(params=[True, False], ids=["cpp_node", "python_node"])
def node(request, GF):
    """The graph=False twin (and the graph=True module's eager first call) through the C++ or the Python autograd node."""
    GF.use_cpp_autograd(request.param)
    yield request.param
    GF.use_cpp_autograd(True)


SHAPE = (64, 10, 256)


def _pair(dev):
    """A graph=True module that is past its capture (its next call replays) and its graph=False twin."""
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    g, eg = GE2ELoss(HParams(device=dev), graph=True), GE2ELoss(HParams(device=dev))
    for E in _inputs(SHAPE, 1200, 2):
        for mod in (g, eg):
            mod(torch.as_tensor(E, device=dev).requires_grad_(True)).backward()
    assert len(g._steps) == 1
    for mod in (g, eg):
        mod.zero_grad(set_to_none=True)
    return g, eg


def test_second_backward_raises_like_eager(GF, node):
    dev = torch.device("cuda:0")
    E = _inputs(SHAPE, 1300, 1)[0]
    for mod in _pair(dev):
        e = torch.as_tensor(E, device=dev).requires_grad_(True)
        loss = mod(e)
        loss.backward()
        w1, e1 = mod.w.grad.clone(), e.grad.clone()
        with pytest.raises(RuntimeError, match="second time"):
            loss.backward()
        assert torch.equal(mod.w.grad, w1) and torch.equal(e.grad, e1), f"graph={mod.graph}: gradients added again"
        _fp64(E, 10.0, -5.0, "auto", f"graph={mod.graph}", loss, dE=e.grad, dw=mod.w.grad, db=mod.b.grad)


def test_retained_backward_accumulates_like_eager(GF, node):
    """Three backward calls, the first two with retain_graph=True: three times the gradients, bit for bit as eager (the first
    call hands out the static buffers as .grad -- the later ones must not add into those in place), then a fourth raises."""
    dev = torch.device("cuda:0")
    E = _inputs(SHAPE, 1400, 1)[0]
    got = []
    for mod in _pair(dev):
        e = torch.as_tensor(E, device=dev).requires_grad_(True)
        loss = mod(e)
        loss.backward(retain_graph=True)
        loss.backward(retain_graph=True)
        loss.backward()
        with pytest.raises(RuntimeError, match="second time"):
            loss.backward()
        got.append((e.grad.clone(), mod.w.grad.clone(), mod.b.grad.clone()))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    ref = orc.closed_form(np.asarray(E, np.float64), 10.0, -5.0)
    assert abs(float(got[0][1]) - 3 * ref["dw"]) <= 1e-4 * abs(3 * ref["dw"]) + 1e-5


def test_backward_with_nothing_requiring_grad_raises_like_eager(GF, node):
    dev = torch.device("cuda:0")
    E = _inputs(SHAPE, 1500, 1)[0]
    for mod in _pair(dev):
        mod.w.requires_grad_(False)
        mod.b.requires_grad_(False)
        loss = mod(torch.as_tensor(E, device=dev))
        with pytest.raises(RuntimeError, match="does not require grad"):
            loss.backward()
        _fp64(E, 10.0, -5.0, "auto", f"graph={mod.graph}", loss)


def test_autograd_grad_leaves_dot_grad_alone(GF, node):
    dev = torch.device("cuda:0")
    E = _inputs(SHAPE, 1600, 1)[0]
    got = []
    for mod in _pair(dev):
        e = torch.as_tensor(E, device=dev).requires_grad_(True)
        loss = mod(e)
        gs = torch.autograd.grad(loss, (e, mod.w, mod.b))
        assert e.grad is None and mod.w.grad is None and mod.b.grad is None, f"graph={mod.graph}"
        _fp64(E, 10.0, -5.0, "auto", f"graph={mod.graph}", loss, dE=gs[0], dw=gs[1], db=gs[2])
        got.append(gs)
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_hooks_on_the_accumulate_grad_node_fire(GF, node):
    """Hooks registered from Python on w's AccumulateGrad node (the way DDP's reducer hooks a parameter, there from C++) fire
    once per backward, as in eager, and the gradients stay eager's bits."""
    dev = torch.device("cuda:0")
    Es = _inputs(SHAPE, 1700, 3)
    got = []
    for mod in _pair(dev):
        acc = mod.w.view_as(mod.w).grad_fn.next_functions[0][0]
        fired = {"pre": 0, "post": 0}
        seen = []
        h1 = acc.register_prehook(lambda go: fired.__setitem__("pre", fired["pre"] + 1))

        def post(gi, go):
            fired["post"] += 1
            seen.append(go[0].clone())
        h2 = acc.register_hook(post)
        grads = []
        for E in Es:
            mod.zero_grad(set_to_none=True)
            e = torch.as_tensor(E, device=dev).requires_grad_(True)
            loss = mod(e)
            loss.backward()
            grads.append((loss.detach().clone(), e.grad.clone(), mod.w.grad.clone(), mod.b.grad.clone()))
            _fp64(E, 10.0, -5.0, "auto", f"graph={mod.graph}", loss, dE=e.grad, dw=mod.w.grad, db=mod.b.grad)
        h1.remove()
        h2.remove()
        assert fired == {"pre": len(Es), "post": len(Es)}, (mod.graph, fired)
        got.append((grads, seen))
    for a, b in zip(got[0][0], got[1][0]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    for x, y in zip(got[0][1], got[1][1]):
        assert torch.equal(x, y)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_ddp_single_rank_nccl(GF, node):
    """DistributedDataParallel (one rank, nccl) over an encoder with GE2ELoss(graph=True) inside: the reducer hooks every
    parameter's AccumulateGrad node from C++, so w and b must reach the engine to be marked ready (else the next forward
    fails with 'Expected to have finished reduction').  Five SGD steps; every gradient equals the graph=False twin's bit for
    bit, the loss and dw / db match fp64."""
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_free_port())
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        N, M, D = SHAPE

        class Net(torch.nn.Module):
            def __init__(self, graph):
                super().__init__()
                self.enc = torch.nn.Linear(40, D)
                self.ge2e = GE2ELoss(HParams(device=dev), graph=graph)

            def forward(self, x):
                emb = torch.nn.functional.normalize(self.enc(x), dim=-1).reshape(N, M, D)
                return self.ge2e(emb), emb.detach()

        torch.manual_seed(0)
        nets = [Net(True).to(dev), Net(False).to(dev)]
        nets[1].load_state_dict(nets[0].state_dict())
        ddps = [DDP(n, device_ids=[dev.index]) for n in nets]
        opts = [torch.optim.SGD(n.parameters(), lr=0.05) for n in nets]
        for it in range(5):
            x = torch.randn(N * M, 40, device=dev)
            res = []
            for ddp, opt, net in zip(ddps, opts, nets):
                opt.zero_grad(set_to_none=True)
                wb = (float(net.ge2e.w), float(net.ge2e.b))
                loss, emb = ddp(x)
                loss.backward()
                res.append((loss.detach().clone(), emb, [p.grad.clone() for p in net.parameters()], wb))
                opt.step()
            torch.cuda.synchronize()
            assert len(nets[0].ge2e._steps) == (1 if it >= 1 else 0), it
            assert torch.equal(res[0][0], res[1][0]), it
            for g0, g1 in zip(res[0][2], res[1][2]):
                assert torch.equal(g0, g1), it
            names = [k for k, _ in nets[0].named_parameters()]
            loss, emb, grads, (w, b) = res[0]
            _fp64(emb.double().cpu().numpy(), w, b, "auto", f"DDP step {it}", loss,
                  dw=grads[names.index("ge2e.w")], db=grads[names.index("ge2e.b")])
    finally:
        if created:
            dist.destroy_process_group()


# ---- D. the default random generator ---------------------------------------------------------------------------------------

def test_graph_route_leaves_the_default_generator_alone(GF):
    """Eight steps with graph=True (the capture included) leave the default CUDA generator where eight graph=False steps do:
    the same dropout masks, the same sampled batches afterwards."""
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams

    dev = torch.device("cuda:0")
    draws = {}
    for graph in (False, True):
        torch.manual_seed(4321)
        mod = GE2ELoss(HParams(device=dev), graph=graph)
        for _ in range(8):
            e = torch.nn.functional.normalize(torch.randn(*SHAPE, device=dev), dim=-1).requires_grad_(True)
            mod.zero_grad(set_to_none=True)
            loss = mod(e)
            loss.backward()
        _fp64(e.detach().double().cpu().numpy(), 10.0, -5.0, "auto", f"graph={graph}", loss, dE=e.grad, dw=mod.w.grad,
              db=mod.b.grad)
        assert (len(mod._steps) == 1) == graph
        draws[graph] = torch.randn(1000, device=dev)
    assert torch.equal(draws[False], draws[True])
