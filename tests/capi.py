"""The fixtures and the ctypes odds and ends the test modules share (a plain helper module beside guarded.py; not a conftest).

A test module gets a fixture by importing it by name -- `from capi import GF, lib  # noqa: F401` -- and pytest registers what
it finds in the module's namespace, under the name it is bound to there:

    lib           GPU tests: skips without a GPU, then the loaded library
    GF            GPU tests: `functional`, once `lib` has loaded the library
    functional    GPU tests: skips without a GPU, then `functional`, without loading the library first (bound as GF)
    built_lib     CPU tests: builds the library if it is stale, then loads it (bound as lib)
"""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from speaker_embedding_ge2e_loss_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def GF(lib):
    from speaker_embedding_ge2e_loss_amd import functional
    return functional


@pytest.fixture(scope="module")
def functional():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from speaker_embedding_ge2e_loss_amd import functional
    return functional


@pytest.fixture(scope="module")
def built_lib():
    from speaker_embedding_ge2e_loss_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def ok(code, what):
    assert code == 0, f"{what} returned {code}"


def header_text():
    """include/ge2e_hip.h without its comments."""
    text = open(os.path.join(ROOT, "include", "ge2e_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def header_symbols():
    """Every ge2e_* function the header declares, sorted."""
    return sorted(set(re.findall(r"\b(ge2e_[a-z_0-9]+)\s*\(", header_text())))
