"""CPU: the C-ABI library builds/loads, exports every symbol the header declares and
rejects bad arguments before touching the GPU.  No compute is launched here."""
import ctypes
import os
import re

import pytest

from capi import built_lib as lib  # noqa: F401
from capi import header_symbols, header_text
from speaker_embedding_ge2e_loss_amd import _lib, build



def test_library_exports_every_declared_symbol(lib):
    syms = header_symbols()
    assert "ge2e_loss_fwd_bwd" in syms and "ge2e_cos_sim" in syms and len(syms) >= 8
    raw = ctypes.CDLL(build.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in include/ge2e_hip.h but not exported"
    assert set(syms) == set(_lib.PROTOTYPES), "ctypes binding and header disagree"


# ---- the binding is derived from the header (_lib.parse_prototypes, _lib.parse_macros); where these tests read the header
# itself, they do it with regexes of their own ----

_TYPES_HEADER = """
#ifdef __cplusplus
extern "C" {
#endif
#define GE2E_SOME_LIMIT 48   /* a comment
                                over two lines */
#define GE2E_ERR_SOME (-7)
/* ge2e_in_a_comment(int x); */
const char* ge2e_a(void);   // ge2e_in_a_line_comment(int x);
size_t ge2e_b(long long n, double x, char* buf, size_t k, const long long* p /* [U] or NULL */,
              unsigned* out, float f, const char* name, void* stream);
#ifdef __cplusplus
}
#endif
"""


def test_parser_maps_the_types_the_header_uses():
    c = ctypes
    assert _lib.parse_prototypes(_TYPES_HEADER) == {
        "ge2e_a": (c.c_char_p, []),
        "ge2e_b": (c.c_size_t, [c.c_longlong, c.c_double, c.c_char_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_float, c.c_char_p,
                                c.c_void_p])}
    assert _lib.parse_macros(_TYPES_HEADER) == {"GE2E_SOME_LIMIT": 48, "GE2E_ERR_SOME": -7}


@pytest.mark.parametrize("decl", ["int ge2e_bad(short x);", "int ge2e_bad(int B, unsigned long n);", "int ge2e_bad(struct S s);",
                                  "short ge2e_bad(int B);", "int ge2e_bad(int);",
                                  "int ge2e_bad(int B, void (*done)(int));",          # no declaration the pattern matches
                                  "int ge2e_a(int B);"])                              # declared twice
def test_parser_refuses_what_it_does_not_know(decl):
    """Never a default: an unknown scalar type, and a declaration the pattern cannot take, raise and name the symbol."""
    with pytest.raises(ValueError, match=decl.split("(")[0].split()[-1]):
        _lib.parse_prototypes(_TYPES_HEADER + decl)


def test_missing_header_fails_loudly(tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "INCLUDE", str(tmp_path))
    with pytest.raises(_lib.GE2ELibraryError, match=os.path.join(str(tmp_path), "ge2e_hip.h")):
        _lib._header()


def test_constants_are_the_headers_macros(lib):
    from speaker_embedding_ge2e_loss_amd import functional
    macros = {name: int(value) for name, value in re.findall(r"#define\s+(GE2E_[A-Z0-9_]+)\s+\(?(-?\d+)\)?", header_text())}

    def family(prefix):
        return {name[len(prefix):].lower(): value for name, value in macros.items() if name.startswith(prefix)}
    assert len(family("GE2E_IMPL_")) >= 8 and _lib.IMPLS == family("GE2E_IMPL_")
    assert len(family("GE2E_VARIANT_")) >= 2 and _lib.VARIANTS == family("GE2E_VARIANT_")
    assert _lib.IMPL_NAMES == {value: name for name, value in _lib.IMPLS.items()}
    assert (_lib.IMPL_AUTO, _lib.IMPL_AUTO_NO_TEAM, _lib.VARIANT_CONTRAST) == \
        (macros["GE2E_IMPL_AUTO"], macros["GE2E_IMPL_AUTO_NO_TEAM"], macros["GE2E_VARIANT_CONTRAST"])
    assert _lib.ABI_VERSION == macros["GE2E_ABI_VERSION"] == lib.ge2e_abi_version()
    assert functional.IDENTIFY_MAX_TOP == macros["GE2E_IDENTIFY_MAX_TOP"] == 32
    assert functional.COHORT_MAX == macros["GE2E_COHORT_MAX"] == 65536
    assert _lib.MACROS == macros
    errors = family("GE2E_ERR_")
    assert len(errors) >= 6 and all(value < 0 for value in errors.values())
    for value in errors.values():
        assert len(lib.ge2e_strerror(value)) > 3


def test_wide_parameters_bind_wide():
    """A `long long` bound as c_int, or a size_t as c_int, passes every call with small values and corrupts the arguments of
    a large one: every by-value parameter (and return value) of those types in the header binds at full width."""
    wide = {"long long": ctypes.c_longlong, "size_t": ctypes.c_size_t}
    seen = {ctype: 0 for ctype in wide.values()}
    for ret, symbol, params in re.findall(r"([\w \t*]+?)\b(ge2e_\w+)\s*\(([^()]*)\)\s*;", header_text()):
        restype, argtypes = _lib.PROTOTYPES[symbol]
        if ret.strip() in wide:
            assert restype is wide[ret.strip()], symbol
            seen[restype] += 1
        for i, param in enumerate(params.split(",")):
            m = re.fullmatch(r"\s*(long long|size_t)\s+\w+\s*", param)
            if m:
                assert argtypes[i] is wide[m.group(1)], (symbol, param)
                seen[argtypes[i]] += 1
    assert seen[ctypes.c_longlong] >= 2 and seen[ctypes.c_size_t] >= 40, seen      # total_frames twice; every workspace


def test_bind_types_every_prototype_of_a_library(lib):
    raw = _lib.bind(ctypes.CDLL(build.LIB_PATH))
    assert len(_lib.PROTOTYPES) >= 82
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(raw, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    with pytest.raises(_lib.GE2ELibraryError, match="does not export ge2e_"):
        _lib.bind(ctypes.CDLL(None))          # the interpreter itself: no ge2e_* symbol


def test_abi_version_and_errors(lib):
    assert lib.ge2e_abi_version() == 2
    assert lib.ge2e_strerror(0) == b"ok"
    for code in (-1, -2, -3, -4, -5, -6):
        assert len(lib.ge2e_strerror(code)) > 3


def test_argument_validation_returns_codes_without_gpu(lib):
    f = lib.ge2e_loss_fwd_bwd
    # NULL E
    assert f(None, 1, 4, 5, 8, 16, 16, 1e-8, 1e-6, 0, 0, 16, None, None, None, None, None, 0, None) == -1
    # M = 1 divides by zero in the reference (s3:110-111) -> shape error
    assert f(16, 1, 4, 1, 8, 16, 16, 1e-8, 1e-6, 0, 0, 16, None, None, None, None, 256, 1 << 30, None) == -2
    assert f(16, 0, 4, 5, 8, 16, 16, 1e-8, 1e-6, 0, 0, 16, None, None, None, None, 256, 1 << 30, None) == -2
    # unknown variant / impl
    assert f(16, 1, 4, 5, 8, 16, 16, 1e-8, 1e-6, 7, 0, 16, None, None, None, None, 256, 1 << 30, None) == -4
    assert f(16, 1, 4, 5, 8, 16, 16, 1e-8, 1e-6, 0, 99, 16, None, None, None, None, 256, 1 << 30, None) == -5
    # workspace too small / missing
    assert f(16, 1, 4, 5, 8, 16, 16, 1e-8, 1e-6, 0, 1, 16, None, None, None, None, 256, 8, None) == -3
    assert f(16, 1, 4, 5, 8, 16, 16, 1e-8, 1e-6, 0, 1, 16, None, None, None, None, None, 0, None) == -3
    # dE without dw/db
    assert f(16, 1, 4, 5, 8, 16, 16, 1e-8, 1e-6, 0, 1, 16, None, 32, None, None, 256, 1 << 30, None) == -1
    # misaligned E
    assert f(20, 1, 4, 5, 8, 16, 16, 1e-8, 1e-6, 0, 1, 16, None, None, None, None, 256, 1 << 30, None) == -6
    assert lib.ge2e_cos_sim(None, 1, 4, 5, 8, 1e-8, 1e-6, None, None, 0, None) == -1
    assert lib.ge2e_centroids(None, 1, 4, 5, 8, None, None) == -1
    assert lib.ge2e_calc_loss(None, 1, 4, 5, 1e-6, 0, None, None, None) == -1


# The order of the host checks is part of the ABI (callers tell a bad shape from a missing workspace by the code): for every
# ADJACENT pair of checks of an entry point, one call that violates both must return the earlier one's code.  Pointers are
# fake integers; every call fails a check, so nothing is launched.
_LOSS_ARGS = ("E", "B", "N", "M", "D", "w", "b", "eps_cos", "eps", "variant", "loss", "per", "dE", "dw", "db")
_ORDER_OK = dict(E=16, src=None, B=1, N=4, M=5, D=64, w=16, b=16, eps_cos=1e-8, eps=1e-6, variant=0, loss=16, per=None,
                 dE=None, dw=None, db=None, ws=256, ws_bytes=1 << 40, stream=None, max_workgroups=64,
                 table=16, R=20, active=None, thr=16, T=50, cos=16, col=None, speakers=None, counts=16)
_ROW_ARGS = ("E", "table", "B", "N", "R", "D") + _LOSS_ARGS[5:]        # (B, R, D) rows plus a table: offsets or labels
_ORDER_ARGS = {
    "ge2e_loss_fwd_bwd_f64": _LOSS_ARGS + ("ws", "ws_bytes", "stream"),
    "ge2e_loss_fwd_bwd_raw": ("E", "src") + _LOSS_ARGS[1:] + ("stream",),
    "ge2e_selftest_team_fallback": _LOSS_ARGS + ("ws", "ws_bytes", "stream"),
    "ge2e_selftest_team_grid": _LOSS_ARGS + ("ws", "ws_bytes", "stream", "max_workgroups"),
    "ge2e_loss_fwd_bwd_ragged": _ROW_ARGS + ("ws", "ws_bytes", "stream"),
    "ge2e_loss_fwd_bwd_labeled": _ROW_ARGS + ("ws", "ws_bytes", "stream"),
    "ge2e_loss_fwd_bwd_labeled_masked": _ROW_ARGS + ("active", "ws", "ws_bytes", "stream"),
    "ge2e_cos_sim_labeled": ("E", "table", "B", "N", "R", "D", "eps_cos", "eps", "thr", "T", "cos", "col", "speakers", "active",
                             "counts", "ws", "ws_bytes", "stream"),
}
_NULL, _SHAPE, _WORKSPACE, _VARIANT, _IMPL, _ALIGN = -1, -2, -3, -4, -5, -6
_BAD = {_NULL: dict(E=None), _SHAPE: dict(M=1), _VARIANT: dict(variant=7), _WORKSPACE: dict(ws=None, ws_bytes=0),
        _ALIGN: dict(E=24),
        _IMPL: dict(N=64, M=10, D=512)}     # no one-wave raw shape (N = 64) and none of the team kernel (D > 256)
_ORDERS = {
    "ge2e_loss_fwd_bwd_f64": (_NULL, _SHAPE, _VARIANT, _WORKSPACE, _ALIGN),
    "ge2e_loss_fwd_bwd_raw": (_NULL, _SHAPE, _VARIANT, _IMPL, _ALIGN),
    "ge2e_selftest_team_fallback": (_NULL, _SHAPE, _VARIANT, _IMPL, _WORKSPACE, _ALIGN),
    "ge2e_selftest_team_grid": (_NULL, _SHAPE, _VARIANT, _IMPL, _WORKSPACE, _ALIGN),
}
_ORDER_CASES = [(entry, dict(_BAD[first], **_BAD[second]), first)
                for entry, order in _ORDERS.items() for first, second in zip(order, order[1:])]
# ge2e_selftest_team_grid: its own SHAPE check (max_workgroups < 64) sits between NULL and the common sequence
_ORDER_CASES += [("ge2e_selftest_team_grid", dict(E=None, max_workgroups=8), _NULL),
                 ("ge2e_selftest_team_grid", dict(max_workgroups=8, variant=7), _SHAPE),
                 ("ge2e_selftest_team_grid", dict(max_workgroups=8, ws=None, ws_bytes=0), _SHAPE)]
# the second half of the NULL rule (dE without dw / db) is NULL too, ahead of everything else
_ORDER_CASES += [(entry, dict(dE=32, M=1), _NULL) for entry in _ORDERS]
# The row-list entry points: the adjacent pairs of their common sequence are asserted next to each of them
# (test_argument_validation_returns_codes_without_gpu of their own files); here is what those leave out.  Their shape
# violation is a batch without rows.
_ROW_BAD = {**_BAD, _SHAPE: dict(R=0)}
_ROW_ORDERS = {
    "ge2e_loss_fwd_bwd_ragged": (_NULL, _SHAPE, _VARIANT, _WORKSPACE, _ALIGN),
    "ge2e_loss_fwd_bwd_labeled": (_NULL, _SHAPE, _VARIANT, _WORKSPACE, _ALIGN),
    "ge2e_loss_fwd_bwd_labeled_masked": (_NULL, _SHAPE, _VARIANT, _WORKSPACE, _ALIGN),
    "ge2e_cos_sim_labeled": (_NULL, _SHAPE, _WORKSPACE, _ALIGN),          # no loss: no variant step
}
# ... the second half of the NULL rule ahead of the shape,
_ORDER_CASES += [(entry, dict(dE=32, R=0), _NULL) for entry in _ROW_ORDERS if entry != "ge2e_cos_sim_labeled"]
# ... and of the evaluation call: its own half of the NULL rule (neither cos nor counts) ahead of a batch without rows, and
# the threshold half of its shape rule (counts without thresholds, counts with T = 0) ahead of the workspace
_ORDER_CASES += [("ge2e_cos_sim_labeled", dict(cos=None, counts=None, R=0), _NULL),
                 ("ge2e_cos_sim_labeled", dict(thr=None, ws=None, ws_bytes=0), _SHAPE),
                 ("ge2e_cos_sim_labeled", dict(T=0, ws=None, ws_bytes=0), _SHAPE)]


@pytest.mark.parametrize("entry, violate, expect", _ORDER_CASES,
                         ids=[f"{e[5:]}-{'+'.join(sorted(v))}" for e, v, _ in _ORDER_CASES])
def test_checks_come_in_the_documented_order(lib, entry, violate, expect):
    def call(**kw):
        a = dict(_ORDER_OK, **kw)
        return getattr(lib, entry)(*[a[k] for k in _ORDER_ARGS[entry]])

    # each violation alone draws its own code (so the pair really violates two checks) ...
    assert lib.ge2e_raw_supported(4, 5, 64) == 1 and lib.ge2e_raw_supported(64, 10, 512) == 0
    assert lib.ge2e_resolve_impl(1, 4, 5, 64, 0, _lib.IMPLS["team"]) == _lib.IMPLS["team"]
    assert lib.ge2e_resolve_impl(1, 64, 10, 512, 0, _lib.IMPLS["team"]) == _IMPL
    order, bads = (_ROW_ORDERS[entry], _ROW_BAD) if entry in _ROW_ORDERS else (_ORDERS[entry], _BAD)
    for code, bad in bads.items():
        if code in order and all(violate.get(k, 0) == v for k, v in bad.items()):
            assert call(**bad) == code, (entry, bad)
    # ... and together the earlier check answers
    assert call(**violate) == expect, (entry, violate)


def test_workspace_and_impl_queries(lib):
    assert lib.ge2e_workspace_bytes(1, 4, 1, 8, 0, 0) == 0  # bad shape -> 0
    assert lib.ge2e_workspace_bytes(1, 64, 10, 256, 0, 1) > 64 * 256 * 4
    assert lib.ge2e_resolve_impl(1, 64, 10, 256, 0, 1) == 1
    assert lib.ge2e_resolve_impl(1, 64, 10, 256, 0, 0) in (1, 2, 3, 4, 5)
    assert lib.ge2e_workspace_bytes(1, 64, 10, 256, 0, 5) > 8 * 64 * 256 * 4  # team: exchange area, sized without a GPU
    assert lib.ge2e_resolve_impl(1, 64, 1, 256, 0, 0) == -2
    # every impl AUTO can resolve to must report a workspace
    for shape in [(1, 4, 5, 256), (1024, 64, 10, 256), (8, 256, 10, 256), (1, 1024, 10, 768)]:
        impl = lib.ge2e_resolve_impl(*shape, 0, 0)
        assert impl > 0
        assert lib.ge2e_workspace_bytes(*shape, 0, impl) == lib.ge2e_workspace_bytes(*shape, 0, 0)


def test_auto_leaves_the_team_kernel_out_on_request(lib):
    """impl = auto_no_team (a caller that shares the GPU with other streams or processes): AUTO's choice without the
    eight-CU team kernel; an explicit impl=team is still honoured; the workspace query follows the resolved kernel."""
    assert lib.ge2e_resolve_impl(1, 64, 10, 256, 0, _lib.IMPLS["auto"]) == _lib.IMPLS["team"]
    assert lib.ge2e_resolve_impl(1, 64, 10, 256, 0, _lib.IMPLS["auto_no_team"]) == _lib.IMPLS["fused_split"]
    assert lib.ge2e_resolve_impl(1, 64, 10, 256, 0, _lib.IMPLS["team"]) == _lib.IMPLS["team"]
    assert lib.ge2e_resolve_impl(4096, 4, 5, 256, 0, _lib.IMPLS["auto_no_team"]) == _lib.IMPLS["wave"]
    assert lib.ge2e_workspace_bytes(8, 64, 10, 256, 0, _lib.IMPLS["auto_no_team"]) == \
        lib.ge2e_workspace_bytes(8, 64, 10, 256, 0, _lib.IMPLS["fused_split"])


def test_no_environment_override_of_the_implementation_choice():
    """Rounds 2-3 honoured GE2E_AUTO_NO_TEAM=1; the choice is an argument of the call now (impl="auto_no_team") and the
    variable changes nothing."""
    import subprocess
    import sys
    code = ("from speaker_embedding_ge2e_loss_amd import _lib; lib = _lib.load(); "
            "print(lib.ge2e_resolve_impl(1, 64, 10, 256, 0, 0))")
    import os
    env = dict(os.environ, GE2E_AUTO_NO_TEAM="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip().splitlines()[-1]) == _lib.IMPLS["team"]


def test_product_refuses_cpu_tensors():
    import torch
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    hp = HParams(device="cpu")
    mod = GE2ELoss(hp)
    assert [n for n, _ in mod.named_parameters()] == ["w", "b"]
    assert mod.w.shape == torch.Size([]) and float(mod.w) == 10.0 and float(mod.b) == -5.0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod(torch.randn(4, 5, 8))


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(_lib.GE2ELibraryError, match="not built"):
        _lib.load(str(tmp_path / "nope.so"))


def test_cpp_autograd_library_builds_loads_and_refuses_cpu_tensors():
    """libge2e_torch.so (the autograd node in C++): built next to libge2e_hip.so, registers torch.ops.ge2e_amd.loss, and has
    no CPU path either."""
    import torch
    from speaker_embedding_ge2e_loss_amd import build, functional as GF
    assert os.path.exists(build.build_torch_ext(force=False, verbose=False))
    op = GF._cpp_loss_op()
    assert op is not None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op(torch.randn(4, 5, 8), torch.tensor(10.0), torch.tensor(-5.0), 1e-6, 1e-8, 0, 0)


def test_graph_route_module_copies_start_without_captured_graphs():
    """GE2ELoss(hp, graph=True) keeps captured HIP graphs and their static buffers: a copy (deepcopy, pickle) must not drag
    them along (a CUDAGraph cannot be copied) -- it starts empty and captures its own.  Parameters and options copy."""
    import copy
    import pickle
    from speaker_embedding_ge2e_loss_amd import GE2ELoss, HParams
    m = GE2ELoss(HParams(device="cpu"), variant="contrast", graph=True)
    m._steps["k"] = object()          # stands in for a captured step
    m._last_shape = ("k",)
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert c._steps == {} and c._last_shape is None
        assert c.graph and c.variant == "contrast" and list(c.state_dict()) == ["w", "b"]
    assert "k" in m._steps
