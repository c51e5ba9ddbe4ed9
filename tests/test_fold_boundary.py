"""CPU: the folded layer 1's C boundary (include/dfwfm_fold.h) -- its own header and ABI version in the same
libdfwfm.so, bound separately from include/dfwfm.h's, dfwfm_serve.h's and dfwfm_bf16.h's function sets; no compute
without a GPU."""
import ctypes
import os
import re

import pytest

from conftest import REPO

FOLD_API = ["dfwfm_fold_abi_version", "dfwfm_model_fold_numerical"]


@pytest.fixture(scope="module")
def built():
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.build()
    return _lib


def header_functions(name):
    src = open(os.path.join(REPO, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dfwfm_[a-z0-9_]+)\s*\(", src)))


def test_fold_header_declares_exactly_the_two_functions():
    assert header_functions("dfwfm_fold.h") == FOLD_API
    src = open(os.path.join(REPO, "include", "dfwfm_fold.h")).read()
    assert re.search(r"#define\s+DFWFM_FOLD_ABI_VERSION\s+1\b", src)
    # the numeric contract is stated: the K order, how P is rounded, the bar against the unfolded forward
    for word in ("ascending", "rounded to f32 once", "1e-5"):
        assert word in src, word


def test_library_exports_the_fold_symbols(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in FOLD_API:
        assert hasattr(L, name), name
    assert set(built.FOLD_SIGNATURES) == set(header_functions("dfwfm_fold.h"))
    # the other headers' sets are pinned on their own
    for other in (built.SIGNATURES, built.SERVE_SIGNATURES, built.BF16_SIGNATURES):
        assert not set(built.FOLD_SIGNATURES) & set(other)


def test_fold_abi_version_and_null_arguments(built):
    L = built.lib()
    assert L.dfwfm_fold_abi_version() == 1
    # invalid arguments are reported, never abort (no HIP call is reached)
    en = ctypes.c_int32(7)
    assert L.dfwfm_model_fold_numerical(None, 1, ctypes.byref(en), None) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_model_fold_numerical(None, 0, ctypes.byref(en), None) == -1
    assert L.dfwfm_model_fold_numerical(None, 1, None, None) == -1
    assert b"null" in L.dfwfm_last_error()


def test_dfwfm_h_is_untouched(built):
    """include/dfwfm.h keeps its function list (the binding's SIGNATURES) and ABI version 4: the fold adds nothing
    to it."""
    assert set(header_functions("dfwfm.h")) == set(built.SIGNATURES)
    assert not set(FOLD_API) & set(header_functions("dfwfm.h"))
    src = open(os.path.join(REPO, "include", "dfwfm.h")).read()
    assert re.search(r"#define\s+DFWFM_ABI_VERSION\s+4\b", src)
    assert built.lib().dfwfm_abi_version() == 4


def test_fold_flag_reaches_the_module():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    sizes = [1] * 13 + [7] * 26
    m = DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_cuda=False)
    assert m.fold_numerical is True
    assert "fold" not in "".join(m.state_dict())  # derived state: the state_dict is unchanged
