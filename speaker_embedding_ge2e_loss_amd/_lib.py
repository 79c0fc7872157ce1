"""ctypes binding of libge2e_hip.so, derived from include/ge2e_hip.h.  Plumbing only.

The header is the one description of the C ABI: the library is compiled against it, and this module reads it -- every
`#define GE2E_<NAME> <int>` becomes a constant at import, every `ge2e_*` declaration a ctypes prototype at the first use of
PROTOTYPES, bind() or load() (that parse costs more than importing ctypes does).  A new entry point is declared in the header
and nowhere here.  The parser knows the types the header uses and refuses any other.

The library is loaded lazily and there is NO fallback: if the shared object is
missing or a symbol is absent, every product entry point raises.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import re

from .build import INCLUDE, LIB_PATH


class GE2ELibraryError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "long long": C.c_longlong}


def _ctype(decl: str, symbol: str, what: str):
    """A return type, or a parameter with its name, as the header writes it -> the ctypes class."""
    base, star, _ = decl.partition("*")
    words = base.split()
    if words[:1] == ["const"]:
        words = words[1:]
    if star:                                   # device pointers travel as integers
        return C.c_char_p if words == ["char"] else C.c_void_p
    if what != "return type":
        words = words[:-1]                     # the parameter's name
    try:
        return _SCALARS[" ".join(words)]
    except KeyError:
        raise ValueError(f"{symbol}: {what} `{' '.join(decl.split())}` is not of a type the binding knows") from None


def _without_comments(text: str) -> str:
    return re.sub(r"/\*[^*]*\*+(?:[^/*][^*]*\*+)*/|//[^\n]*", " ", text)      # /* ... */ without backtracking, // ...


def parse_macros(text: str) -> dict:
    """GE2E_NAME -> value of every `#define GE2E_NAME <int or (-int)>` of a header."""
    return {name: int(value) for name, value in re.findall(r"#[ \t]*define[ \t]+(GE2E_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$",
                                                           _without_comments(text), flags=re.M)}


def parse_prototypes(text: str) -> dict:
    """symbol -> (restype, [argtypes]) of every declaration `<ret> ge2e_name(<params>);` of a header."""
    text = re.sub(r'#[^\n]*|extern\s+"C"\s*\{|\}', " ", _without_comments(text))     # preprocessor lines, the C++ wrapper
    prototypes = {}
    for statement in text.split(";"):
        m = re.fullmatch(r"\s*([^()]+?)\s*\b(ge2e_\w+)\s*\(([^()]*)\)\s*", statement)
        if m is None:
            continue
        ret, symbol, params = m.groups()
        params = [] if params.strip() == "void" else params.split(",")
        prototypes[symbol] = (_ctype(ret, symbol, "return type"),
                              [_ctype(p, symbol, f"parameter {i + 1}") for i, p in enumerate(params)])
    named = re.findall(r"(ge2e_\w+)\s*\(", text)
    if len(named) != len(prototypes):
        odd = sorted(n for n in set(named) if n not in prototypes or named.count(n) > 1)
        raise ValueError(f"{len(named)} ge2e_* declarations, {len(prototypes)} parsed; not understood or declared twice: {odd}")
    return prototypes


def _header() -> str:
    path = os.path.join(INCLUDE, "ge2e_hip.h")
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise GE2ELibraryError(f"{path} not readable: the ctypes binding is derived from it") from e


MACROS = parse_macros(_header())


def _family(prefix: str) -> dict:
    return {name[len(prefix):].lower(): value for name, value in MACROS.items() if name.startswith(prefix)}


ABI_VERSION = MACROS["GE2E_ABI_VERSION"]
VARIANTS = _family("GE2E_VARIANT_")
# "auto_no_team": AUTO without the eight-CU team kernel, for a GPU that other streams / processes keep busy (ge2e_hip.h)
IMPLS = _family("GE2E_IMPL_")
IMPL_NAMES = {v: k for k, v in IMPLS.items()}
# VARIANT_SOFTMAX, VARIANT_CONTRAST, IMPL_AUTO ... IMPL_AUTO_NO_TEAM as module names
globals().update({name[5:]: value for name, value in MACROS.items() if name.startswith(("GE2E_VARIANT_", "GE2E_IMPL_"))})


@functools.lru_cache(maxsize=None)
def _prototypes() -> dict:
    return parse_prototypes(_header())


def __getattr__(name: str):
    if name == "PROTOTYPES":                   # made at its first use, once
        return _prototypes()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


_lib = None


def bind(lib):
    """Set restype and argtypes of every prototype on a ctypes.CDLL (the product library or a variant build of it)."""
    for name, (res, args) in _prototypes().items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise GE2ELibraryError(f"{lib._name} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    return lib


def load(path: str | None = None):
    """Load (once) and type the shared library.  Raises if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("GE2E_HIP_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise GE2ELibraryError(
            f"{path} not found: the HIP extension is not built. Run "
            "`python -m speaker_embedding_ge2e_loss_amd.build` (needs hipcc); there is no CPU fallback.")
    lib = bind(C.CDLL(path))
    if lib.ge2e_abi_version() != ABI_VERSION:
        raise GE2ELibraryError(f"ABI mismatch: library {lib.ge2e_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def split_plan(text: str) -> list[str]:
    """The kernel names of a plan string: split at the commas outside <>."""
    names, depth, cur = [], 0, ""
    for ch in text:
        depth += (ch == "<") - (ch == ">")
        if ch == "," and depth == 0:
            names.append(cur)
            cur = ""
        else:
            cur += ch
    return names + [cur] if cur else names


def _plan(fn, *args) -> list[str]:
    buf = C.create_string_buffer(4096)
    n = fn(*args, buf, len(buf))
    if n < 0:
        raise ValueError(f"{fn.__name__}{args}: [{n}] {load().ge2e_strerror(n).decode()}")
    if n >= len(buf):
        buf = C.create_string_buffer(n + 1)
        fn(*args, buf, len(buf))
    return split_plan(buf.value.decode())


def loss_plan(B: int, N: int, M: int, D: int, variant: str = "softmax", impl: str = "auto", want_grad: bool = True,
              raw: bool = False) -> list[str]:
    """Diagnostics: the kernels ge2e_loss_fwd_bwd (raw: ge2e_loss_fwd_bwd_raw) would launch, in order.  No GPU needed.
    ValueError where the call itself would be refused."""
    return _plan(load().ge2e_loss_plan, B, N, M, D, VARIANTS[variant], IMPLS[impl], int(want_grad), int(raw))


def cos_sim_plan(B: int, N: int, M: int, D: int) -> list[str]:
    """... ge2e_cos_sim on a workspace of ge2e_cos_sim_workspace_bytes would launch."""
    return _plan(load().ge2e_cos_sim_plan, B, N, M, D)


def encode_plan(R: int, T: int, n_mels: int, H: int, L: int, D: int) -> list[str]:
    """... ge2e_encode would launch: ["encode<H>/tiles"]."""
    return _plan(load().ge2e_encode_plan, R, T, n_mels, H, L, D)


def encode_train_plan(R: int, T: int, n_mels: int, H: int, L: int, D: int) -> list[str]:
    """... ge2e_encode_train would launch: ["encode_train<H>/tiles"]."""
    return _plan(load().ge2e_encode_train_plan, R, T, n_mels, H, L, D)


def encode_bwd_plan(R: int, T: int, n_mels: int, H: int, L: int, D: int) -> list[str]:
    """... ge2e_encode_bwd would launch: the recurrence "encode_bwd<H>/tiles", L + 1 "encode_wgrad/NxMxS" (column blocks x
    row blocks x K-slices; the last is the projection's) and "encode_reduce/blocks"."""
    return _plan(load().ge2e_encode_bwd_plan, R, T, n_mels, H, L, D)


def melspec_plan(U: int, total_frames: int, n_fft: int, hop: int, n_mels: int) -> list[str]:
    """... ge2e_melspec would launch: ["melspec<n_fft>/tiles"]."""
    return _plan(load().ge2e_melspec_plan, U, total_frames, n_fft, hop, n_mels)


def resample_plan(U: int, total_out: int, L: int, M: int, lead: int) -> list[str]:
    """... ge2e_resample would launch: ["resample<lds,R>/tile/grid"] ("global": the samples are not staged in LDS)."""
    return _plan(load().ge2e_resample_plan, U, total_out, L, M, lead)


def plan_atoms() -> list[str]:
    """Every kernel name the two queries can return."""
    return _plan(load().ge2e_plan_atoms)


def check(code: int, what: str):
    if code != 0:
        msg = load().ge2e_strerror(code).decode()
        raise RuntimeError(f"{what} failed: [{code}] {msg}")
