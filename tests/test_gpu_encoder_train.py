"""GPU: the native encoder's training path (ge2e_encode_train, ge2e_encoder_pack_bwd, ge2e_encode_bwd,
functional.encode_train, SpeakerEncoder(native_train=True), DPTrainer on top of it) against tests/encoder_grad_ref.py in
float64.  The C ABI is called with raw pointers on guarded buffers (tests/guarded.py): the mels and the upstream gradient
between NaN guards; the output, the tape and the flat gradient buffer NaN-poisoned between guards; the workspace poisoned
with one byte pattern for the first backward call and another for the second.

The gate is calibrated on the reference, never on the code under test: per gradient tensor, err_ref is the relative
Frobenius error of torch's CPU float32 autograd against encoder_grad_ref in float64 on the case's own inputs and upstream
gradient (a seeded standard normal), and the native tensor must satisfy err <= 4 err_ref + 2^-22 (encoder_ref.gate).  A
tensor that is exactly zero in float64 must be exactly zero natively.  There is no row-by-row form of the gate: the rows of
a weight gradient cancel.

native(name, normalize) runs a case ONCE -- ge2e_encode, ge2e_encode_train, two backward calls -- and every test of the
case reads that record: the forward's bits, the repeated gradients' bits, the guards, the poison.

Measured on an MI355X, err / err_ref of the worst gradient tensor of a case (the gate allows 4 plus the floor; normalised /
raw).  The worst tensor is projection.weight or projection.bias nearly everywhere (errors of 2e-7 .. 4e-7 under gates of
6e-7 .. 9e-7: the floor carries a third of the gate); the LSTM tensors sit at 1.0 .. 1.8.
t1 2.54 / 2.95, t2 1.94 / 2.19; rows 1: 2.33 / 2.31, 15: 2.39 / 2.37, 16: 2.19 / 2.35, 17: 2.17 / 2.26, 31: 2.04 / 1.98,
32: 1.94 / 2.00, 33: 2.03 / 2.18 (rows1 raw: projection.bias is exact on both sides).
(H, L) grid at (17, 5, 20, ., ., 24): (128, 1) 1.58 / 1.63, (128, 2) 2.00 / 1.94, (128, 3) 1.94 / 1.94, (128, 4) 2.39 / 1.84,
(256, 1) 2.17 / 2.04, (256, 2) 2.36 / 2.38, (256, 3) 2.35 / 2.37, (256, 4) 2.19 / 2.24.
n_mels 1: 3.54 / 2.06 (projection.bias, three rows: 1.5e-7 under a gate of 4.1e-7), 13: 2.14 / 2.13, 16: 2.15 / 1.78,
17: 1.85 / 1.90, 256: 1.43 / 1.33.  D 1: exact zeros / 2.07, 15: 1.66 / 1.84, 16: 2.63 / 2.55, 17: 1.68 / 1.71, 256: 1.94 / 2.11.
K-slices 511: 1.33 / 2.06, 512: 1.37 / 1.38, 513: 1.70 / 1.51, 1056: 1.73 / 1.49.  reference 1.94; saturated 2.31 / 2.40
(weight_ih_l1, bias_ih_l1 at 3e-6); far out 1.33 / 2.93 (bias_ih_l0 at 8.5e-7).  Windows in place 2.01; rows 16 .. 32
without gradient 2.08 / 2.34; the module 2.03, its raw() 2.18, after an update 2.28.  No ratio above 4."""
import functools

import numpy as np
import pytest
import torch

import encoder_cases as ec
import encoder_grad_ref as gref
import encoder_ref as enc
from capi import GF, lib, ok  # noqa: F401
from guarded import Buf, Workspace, dev, same_bits
from speaker_embedding_ge2e_loss_amd import functional

pytestmark = pytest.mark.gpu

# name -> (R, T, n_mels, H, L, D, weight scale, input scale, the normalize settings)
BOTH = (True, False)
CASES = {
    "t1": (3, 1, 12, 128, 4, 37, 1.0, 1.0, BOTH),                # no recurrence: every weight_hh gradient is exactly zero
    "t2": (3, 2, 12, 128, 1, 16, 1.0, 1.0, BOTH),                # the first recurrent step
    **{f"rows{R}": (R, 2, 40, 128, 2, 64, 1.0, 1.0, BOTH) for R in (1, 15, 16, 17, 31, 32, 33)},   # both tile heights, the tails
    **{f"mels{n}": (3, 2, n, 128, 1, 8, 1.0, 1.0, BOTH) for n in (1, 13, 16, 17, 256)},            # input padding
    "d1": (3, 2, 12, 128, 1, 1, 1.0, 1.0, BOTH),                 # normalised: the gradient is identically zero
    **{f"d{D}": (3, 2, 12, 128, 1, D, 1.0, 1.0, BOTH) for D in (15, 16, 17, 256)},                 # projection padding
    # the weight gradient's K-slices of 512 (t, r) pairs: one below, at, one above, and three slices
    "k511": (73, 7, 12, 128, 1, 16, 1.0, 1.0, BOTH),
    "k512": (32, 16, 12, 128, 1, 16, 1.0, 1.0, BOTH),
    "k513": (27, 19, 12, 128, 1, 16, 1.0, 1.0, BOTH),
    "k1056": (33, 32, 12, 128, 1, 16, 1.0, 1.0, BOTH),
    "reference": (33, 160, 80, 256, 3, 256, 1.0, 1.0, (True,)),  # the reference's model at its real length, once
    "saturated": (17, 40, 40, 128, 2, 64, 4.0, 1.0, BOTH),       # weights x 4: saturated gates
    "far_out": (33, 40, 40, 128, 2, 64, 1.0, 30.0, BOTH),        # inputs x 30: every gradient finite
}
ALL = [(n, nz) for n, c in CASES.items() for nz in c[8]] + [(n, nz) for n in ec.GRID for nz in BOTH]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Parameters, mels and the upstream gradient of a case (encoder_cases.GRID's are that table's own)."""
    if name in ec.GRID:
        c = ec.case(name)
        shape, ps, x = c["shape"], c["params"], c["x"]
    else:
        R, T, n_mels, H, L, D, wscale, xscale, _ = CASES[name]
        seed = sorted(CASES).index(name)
        ps = enc.random_params(n_mels, H, L, D, seed=500 + seed, scale=wscale)
        x = (np.random.default_rng(600 + seed).uniform(0.0, 0.96, (R, T, n_mels)) * xscale).astype(np.float32)
        shape = (R, T, n_mels, H, L, D)
    g = np.random.default_rng(700 + len(name) + shape[0]).standard_normal((shape[0], shape[5])).astype(np.float32)
    for a in (x, g):
        a.setflags(write=False)
    return dict(shape=shape, params=ps, x=x, g=g)


@functools.lru_cache(maxsize=None)
def reference(name, normalize, zero_rows=None):
    """The float64 gradients (and dz) and torch's CPU float32 autograd on the same inputs: computed once, shared."""
    c = inputs(name)
    g = c["g"].copy()
    if zero_rows:
        g[zero_rows[0]:zero_rows[1]] = 0
    grads, dzs = gref.encode_grads(c["params"], c["x"].astype(np.float64), g.astype(np.float64), normalize, with_dz=True)
    return dict(g=g, grads=grads, dzs=dzs, grads32=gref.torch_grads(c["params"], c["x"], g, torch.float32, normalize))


def device_packs(lib, ps, shape):
    _, _, n_mels, H, L, D = shape
    flat = torch.as_tensor(enc.flat(ps)).to(dev())
    packed = functional.encoder_pack(flat, n_mels, H, L, D)
    packed_bwd = Buf((lib.ge2e_encoder_packed_bwd_bytes(n_mels, H, L, D) // 4,))
    ok(lib.ge2e_encoder_pack_bwd(flat.data_ptr(), n_mels, H, L, D, packed_bwd.ptr, None), "ge2e_encoder_pack_bwd")
    packed_bwd.get("ge2e_encoder_pack_bwd")               # every element written, the guards intact
    return packed, packed_bwd


def run_abi(lib, ps, x, g, shape, normalize, row_start=None):
    """ge2e_encode, ge2e_encode_train and ge2e_encode_bwd (twice, the workspace poisoned differently) through raw pointers
    on guarded buffers -> dict(out, out_train, flat, flat_again, dz).  `x` dense (R, T, n_mels) or, with row_start, flat."""
    R, T, n_mels, H, L, D = shape
    packed, packed_bwd = device_packs(lib, ps, shape)
    mel, gbuf = Buf(x.shape, data=x), Buf((R, D), data=g)
    rs = None if row_start is None else torch.as_tensor(np.asarray(row_start, dtype=np.int64)).to(dev())
    rs_ptr = None if rs is None else rs.data_ptr()
    out, out_train = Buf((R, D)), Buf((R, D))
    tape = Buf((lib.ge2e_encode_train_tape_bytes(*shape) // 4,))
    ws = Workspace(lib.ge2e_encode_bwd_workspace_bytes(*shape), pattern=0xFF)
    ok(lib.ge2e_encode(packed.data_ptr(), mel.ptr, rs_ptr, R, T, n_mels, H, L, D, int(normalize), out.ptr, None), "ge2e_encode")
    ok(lib.ge2e_encode_train(packed.data_ptr(), mel.ptr, rs_ptr, R, T, n_mels, H, L, D, int(normalize), out_train.ptr, tape.ptr,
                             None), "ge2e_encode_train")
    tape.get("the tape")                                   # every element written and finite, the guards intact
    res = dict(out=out.get("ge2e_encode", finite=False), out_train=out_train.get("ge2e_encode_train", finite=False))
    for key, pattern in (("flat", 0xFF), ("flat_again", 0x7F)):
        ws.fill(pattern)
        flat = Buf((functional.encoder_flat_numel(n_mels, H, L, D),))
        ok(lib.ge2e_encode_bwd(packed_bwd.ptr, mel.ptr, rs_ptr, R, T, n_mels, H, L, D, int(normalize), tape.ptr, gbuf.ptr,
                               flat.ptr, ws.ptr, None), "ge2e_encode_bwd")
        res[key] = flat.get("ge2e_encode_bwd", finite=False)
        ws.check("ge2e_encode_bwd")
    res["dz"] = ws.t[:L * T * R * 4 * H * 4].view(torch.float32).view(L, T, R, 4 * H).cpu().numpy()
    for b in (mel, gbuf, tape, packed_bwd, out, out_train):
        assert b.guards_intact()
    return res


@functools.lru_cache(maxsize=None)
def native(name, normalize):
    from speaker_embedding_ge2e_loss_amd import _lib
    c = inputs(name)
    return run_abi(_lib.load(), c["params"], c["x"], c["g"], c["shape"], normalize)


def check_gate(what, flat, ps, ref):
    """Every gradient tensor of a flat buffer against the float64 reference, under the gate calibrated on torch's float32."""
    assert np.isfinite(flat).all(), f"{what}: NaN or inf in the gradients"
    worst = 0.0
    for name, got, want, want32 in zip(gref.names(ps), gref.split_flat(flat, ps), ref["grads"], ref["grads32"]):
        if not np.any(want):
            assert not np.any(got), f"{what} {name}: exactly zero in float64, not natively"
            continue
        err, err_ref = gref.rel_err(got, want), gref.rel_err(want32, want)
        ratio = err / err_ref if err_ref > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        print(f"{what} {name}: err {err:.3e}, err_ref {err_ref:.3e}, ratio {ratio:.2f}, gate {enc.gate(err_ref):.3e}")
        assert err <= enc.gate(err_ref), (what, name, err, err_ref)
    print(f"{what}: worst ratio {worst:.2f}")


@pytest.mark.parametrize("name,normalize", ALL)
def test_gradients_against_float64(lib, name, normalize):
    c, got = inputs(name), native(name, normalize)
    ref = reference(name, normalize)
    # 1. the training forward has ge2e_encode's bits
    assert same_bits(got["out_train"], got["out"]), "ge2e_encode_train's output differs from ge2e_encode's"
    # 2. two backward calls, the workspace poisoned differently: the same bits; 3. every element written
    assert same_bits(got["flat"], got["flat_again"]), "the second backward call gave other bits"
    check_gate(f"{name} {'normalised' if normalize else 'raw'}", got["flat"], c["params"], ref)
    if name == "t1":
        L = c["shape"][4]
        assert all(not gref.split_flat(got["flat"], c["params"])[4 * l + 1].any() for l in range(L))
    if name == "d1" and normalize:
        assert not got["flat"].any()


def test_dz_planes_against_float64(lib):
    """The dZ planes the ABI documents at the workspace's start, [L][T][R][4H] in torch's gate order."""
    for name in ("rows33", "h256_l4"):
        dz, ref = native(name, True)["dz"], reference(name, True)
        for l, want in enumerate(ref["dzs"]):
            got = dz[l].transpose(1, 0, 2)                   # (R, T, 4H)
            assert gref.rel_err(got, want) <= 1e-4, (name, l)


@pytest.mark.parametrize("shape", ec.PACK_SHAPES + ((12, 128, 4, 17),))
def test_pack_bwd_on_its_own(lib, shape):
    """Whatever the order inside a tile (the gradient tests prove that): the backward pack holds weight_hh of layer 0,
    weight_ih and weight_hh of every layer above and the projection weight, each value once -- no bias, no weight_ih of
    layer 0 -- and +0.0 in the projection's rows past D."""
    n_mels, H, L, D = shape
    ps, _ = ec.integer_params(*shape)
    kept = [ps[4 * l + i] for l in range(L) for i in (0, 1) if (l, i) != (0, 0)] + [ps[-2]]
    expected = np.sort(np.concatenate([w.ravel() for w in kept]))
    n_pad = ((D + 15) // 16 * 16 - D) * H
    assert lib.ge2e_encoder_packed_bwd_bytes(*shape) == 4 * (expected.size + n_pad)
    flat = Buf((functional.encoder_flat_numel(*shape),), data=enc.flat(ps))      # a read past either end is a NaN
    packed = Buf((expected.size + n_pad,))                                       # NaN poison: every byte is written
    ok(lib.ge2e_encoder_pack_bwd(flat.ptr, n_mels, H, L, D, packed.ptr, None), "ge2e_encoder_pack_bwd")
    got = packed.get("ge2e_encoder_pack_bwd")
    assert flat.guards_intact() and packed.guards_intact()
    assert np.array_equal(np.sort(got[got != 0]), expected)
    assert int((got.view(np.uint32) == 0).sum()) == n_pad


def test_windows_addressed_in_place(lib):
    T, hop, n_mels, H, L, D = 20, 7, 13, 128, 2, 64
    starts = [i * hop for i in range(5)] + [hop]            # five windows, one of them used twice
    n, frames = len(starts), T + 4 * hop
    ps = enc.random_params(n_mels, H, L, D, seed=320)
    flat = np.full((frames + 9, n_mels), np.nan, dtype=np.float32)           # frames past the last window: NaN
    flat[:frames] = np.random.default_rng(hop).uniform(0, 0.96, (frames, n_mels))
    dense = np.stack([flat[s:s + T] for s in starts])
    g = np.random.default_rng(321).standard_normal((n, D)).astype(np.float32)
    shape = (n, T, n_mels, H, L, D)
    for normalize in BOTH:
        want = run_abi(lib, ps, dense, g, shape, normalize)
        got = run_abi(lib, ps, flat, g, shape, normalize, row_start=starts)
        assert np.isfinite(got["flat"]).all()
        assert same_bits(got["out_train"], want["out_train"]) and same_bits(got["flat"], want["flat"])
        assert same_bits(got["flat"], got["flat_again"])
    grads = gref.encode_grads(ps, dense.astype(np.float64), g.astype(np.float64), False)
    check_gate("windows in place", got["flat"], ps, dict(grads=grads, grads32=gref.torch_grads(ps, dense, g, torch.float32, False)))


def test_zero_upstream_gradient_rows(lib):
    c = inputs("rows33")
    for normalize in BOTH:
        ref = reference("rows33", normalize, zero_rows=(16, 33))
        got = run_abi(lib, c["params"], c["x"], ref["g"], c["shape"], normalize)
        check_gate("rows33, rows 16 .. 32 without gradient", got["flat"], c["params"], ref)
        assert not got["dz"][:, :, 16:33].any(), "a row without an upstream gradient has a non-zero dz"
        assert got["dz"][:, :, :16].any(axis=(0, 1, 3)).all()


def module_pair(GF, name="rows33", H=None):
    from speaker_embedding_ge2e_loss_amd.encoder import SpeakerEncoder
    c = inputs(name)
    _, _, n_mels, h, L, D = c["shape"]
    ps = c["params"] if H is None else enc.random_params(n_mels, H, L, D, seed=9)
    mods = []
    for native_train in (True, False):
        m = SpeakerEncoder(n_mels, H or h, L, D, native_train=native_train).to(dev())
        with torch.no_grad():
            for p, v in zip(m._parameters_in_pack_order(), ps):
                p.copy_(torch.as_tensor(v))
        mods.append(m)
    return c, ps, mods[0], mods[1]


def module_grads(m):
    return np.concatenate([p.grad.detach().cpu().numpy().ravel() for p in m._parameters_in_pack_order()])


def test_module_native_train(GF):
    c, ps, m, plain = module_pair(GF)
    ref = reference("rows33", True)
    x, G = torch.as_tensor(c["x"]).to(dev()), torch.as_tensor(c["g"]).to(dev())
    y = m(x)
    assert "EncodeTrain" in type(y.grad_fn).__name__
    assert same_bits(y.detach().cpu().numpy(), native("rows33", True)["out"])
    (y * G).sum().backward()
    check_gate("module", module_grads(m), ps, ref)
    # native_train=False on the same weights: torch's route as before
    y0 = plain(x)
    assert "EncodeTrain" not in type(y0.grad_fn).__name__
    (y0 * G).sum().backward()
    for a, b in zip(gref.split_flat(module_grads(plain), ps), ref["grads"]):
        assert gref.rel_err(a, b) < 1e-4
    # raw(): the projection before the norm, natively, with its own backward
    m.zero_grad(set_to_none=True)
    (m.raw(x) * G).sum().backward()
    check_gate("module raw", module_grads(m), ps, reference("rows33", False))
    # an in-place update of the parameters: the second step runs on the new weights
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.5)
    ps2 = [p.detach().cpu().numpy() for p in m._parameters_in_pack_order()]
    m.zero_grad(set_to_none=True)
    y2 = m(x)
    (y2 * G).sum().backward()
    want = enc.encode_ref(ps2, c["x"].astype(np.float64))
    assert enc.rel_err(y2.detach().cpu().numpy(), want) <= enc.gate(enc.rel_err(enc.torch_encode(ps2, c["x"], torch.float32), want))
    grads2 = gref.encode_grads(ps2, c["x"].astype(np.float64), c["g"].astype(np.float64))
    check_gate("module after an update", module_grads(m), ps2,
               dict(grads=grads2, grads32=gref.torch_grads(ps2, c["x"], c["g"], torch.float32)))
    # embed() is unchanged: the inference kernel, no graph
    with torch.no_grad():
        for p, q in zip(plain.parameters(), m.parameters()):
            p.copy_(q)
    e = m.embed(x, native=True)
    assert not e.requires_grad and same_bits(e.cpu().numpy(), plain.embed(x, native=True).cpu().numpy())
    assert same_bits(m.embed(x).cpu().numpy(), plain.embed(x).cpu().numpy())
    with torch.no_grad():
        assert m(x).grad_fn is None
    # no gradient goes to the mels
    with pytest.raises(ValueError, match="mel"):
        m(x.clone().requires_grad_(True))


def test_module_without_a_kernel_falls_back_and_functional_raises(GF):
    c, ps, m, plain = module_pair(GF, H=64)
    x, G = torch.as_tensor(c["x"]).to(dev()), torch.as_tensor(c["g"]).to(dev())
    assert not m.native_supported()
    y = m.raw(x)
    assert "EncodeTrain" not in type(y.grad_fn).__name__
    assert torch.equal(y, plain.raw(x))
    _, _, n_mels, _, L, D = c["shape"]
    with pytest.raises(ValueError, match="no native kernel"):
        GF.encode_train(m._parameters_in_pack_order(), x, hidden=64, layers=L, dim=D)
    assert GF.encode_train_tape_bytes(33, 2, n_mels, 64, L, D) == 0 and GF.encode_bwd_workspace_bytes(33, 2, n_mels, 64, L, D) == 0
    assert GF.encode_train_tape_bytes(33, 2, n_mels, 128, L, D) == 4 * (6 * L * 2 * 33 * 128 + 33 * D)


@pytest.mark.parametrize("fused_tail", [False, True])
def test_trainer_step_on_the_native_route(GF, fused_tail):
    from oracle import ge2e_oracle as orc
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    from speaker_embedding_ge2e_loss_amd.encoder import SpeakerEncoder
    from speaker_embedding_ge2e_loss_amd.trainer import DPTrainer
    N, M, T, n_mels, H, L, D = 4, 5, 8, 20, 128, 2, 64
    ps = enc.random_params(n_mels, H, L, D, seed=77)
    mel = np.random.default_rng(78).uniform(0, 0.96, (N, M, T, n_mels)).astype(np.float32)
    e64 = enc.encode_ref(ps, mel.reshape(N * M, T, n_mels).astype(np.float64)).reshape(N, M, D)
    loss64 = orc.closed_form(e64, 10.0, -5.0)["loss"]
    losses = {}
    for native_train in (False, True):
        model = SpeakerEncoder(n_mels, H, L, D, normalize=not fused_tail, native_train=native_train).to(dev())
        with torch.no_grad():
            for p, v in zip(model._parameters_in_pack_order(), ps):
                p.copy_(torch.as_tensor(v))
        trainer = DPTrainer(model, GE2ELoss(HParams("cuda:0")), lr=0.05, seed=5, fused_tail=fused_tail)
        losses[native_train] = float(trainer.step(torch.as_tensor(mel).to(dev())))
        if native_train:
            for p, v in zip(model._parameters_in_pack_order(), ps):
                now = p.detach().cpu().numpy()
                assert np.isfinite(now).all() and not np.array_equal(now, v), "a parameter did not move (or is not finite)"
    err_ref = abs(losses[False] - loss64) / abs(loss64)
    err = abs(losses[True] - loss64) / abs(loss64)
    print(f"trainer fused_tail={fused_tail}: loss {losses[True]:.7f}, torch route {losses[False]:.7f}, float64 {loss64:.7f}")
    assert err <= enc.gate(err_ref), (losses, loss64)


def test_forward_and_backward_in_one_captured_graph(lib):
    c = inputs("rows33")
    R, T, n_mels, H, L, D = shape = c["shape"]
    packed, packed_bwd = device_packs(lib, c["params"], shape)
    mel = torch.zeros(R, T, n_mels, device=dev())
    g = torch.zeros(R, D, device=dev())
    out = torch.empty(R, D, device=dev())
    tape = torch.empty(lib.ge2e_encode_train_tape_bytes(*shape) // 4, device=dev())
    ws = torch.empty(lib.ge2e_encode_bwd_workspace_bytes(*shape) // 4, device=dev())
    flat = torch.empty(functional.encoder_flat_numel(n_mels, H, L, D), device=dev())

    def both():
        s = torch.cuda.current_stream().cuda_stream
        ok(lib.ge2e_encode_train(packed.data_ptr(), mel.data_ptr(), None, R, T, n_mels, H, L, D, 1, out.data_ptr(),
                                 tape.data_ptr(), s), "ge2e_encode_train")
        ok(lib.ge2e_encode_bwd(packed_bwd.ptr, mel.data_ptr(), None, R, T, n_mels, H, L, D, 1, tape.data_ptr(), g.data_ptr(),
                               flat.data_ptr(), ws.data_ptr(), s), "ge2e_encode_bwd")

    feeds = [(torch.as_tensor(c["x"]).to(dev()), torch.as_tensor(c["g"]).to(dev())),
             (torch.as_tensor(c["x"][::-1].copy()).to(dev()) * 0.5, torch.as_tensor(c["g"] * 2).to(dev()))]
    eager = []
    for x, gg in feeds:                                     # (the eager calls also prepare the kernels before the capture)
        mel.copy_(x)
        g.copy_(gg)
        both()
        torch.cuda.synchronize()
        eager.append((out.cpu().numpy(), flat.cpu().numpy()))
    assert same_bits(eager[0][1], native("rows33", True)["flat"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for (x, gg), (want_out, want_flat) in zip(feeds, eager):
        mel.copy_(x)
        g.copy_(gg)
        out.fill_(float("nan"))
        flat.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out.cpu().numpy(), want_out) and same_bits(flat.cpu().numpy(), want_flat)
