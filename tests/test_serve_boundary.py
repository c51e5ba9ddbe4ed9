"""CPU: the small-batch serving forward's C boundary (include/dfwfm_serve.h) -- its own header and ABI version in
the same libdfwfm.so, bound separately from include/dfwfm.h's function set; no compute without a GPU."""
import ctypes
import os
import re

import pytest

from conftest import REPO

SERVE_API = ["dfwfm_serve_abi_version", "dfwfm_serve_forward", "dfwfm_serve_workspace_bytes"]


@pytest.fixture(scope="module")
def built():
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.build()
    return _lib


def serve_header_functions():
    src = open(os.path.join(REPO, "include", "dfwfm_serve.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dfwfm_[a-z_]+)\s*\(", src)))


def test_serve_header_declares_exactly_the_three_functions():
    assert serve_header_functions() == SERVE_API
    src = open(os.path.join(REPO, "include", "dfwfm_serve.h")).read()
    assert re.search(r"#define\s+DFWFM_SERVE_ABI_VERSION\s+1\b", src)


def test_library_exports_the_serve_symbols(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in SERVE_API:
        assert hasattr(L, name), name
    assert set(built.SERVE_SIGNATURES) == set(serve_header_functions())
    assert not set(built.SERVE_SIGNATURES) & set(built.SIGNATURES)  # include/dfwfm.h's set is pinned on its own


def test_serve_abi_version_and_null_arguments(built):
    L = built.lib()
    assert L.dfwfm_serve_abi_version() == 1
    # invalid arguments are reported, never abort (no HIP call is reached)
    n = ctypes.c_size_t(0)
    assert L.dfwfm_serve_forward(None, None, 0, None, 0, 1, None, None, 0, None) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_serve_workspace_bytes(None, 1, ctypes.byref(n)) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_serve_workspace_bytes(None, 1, None) == -1
