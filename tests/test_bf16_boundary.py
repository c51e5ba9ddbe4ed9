"""CPU: the bf16 deep tower's C boundary (include/dfwfm_bf16.h) -- its own header and ABI version in the same
libdfwfm.so, bound separately from include/dfwfm.h's and include/dfwfm_serve.h's function sets; no compute without a
GPU."""
import ctypes
import os
import re

import pytest

from conftest import REPO

BF16_API = ["dfwfm_bf16_abi_version", "dfwfm_bf16_forward", "dfwfm_bf16_workspace_bytes", "dfwfm_model_pack_bf16"]


@pytest.fixture(scope="module")
def built():
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.build()
    return _lib


def bf16_header_functions():
    src = open(os.path.join(REPO, "include", "dfwfm_bf16.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dfwfm_[a-z0-9_]+)\s*\(", src)))


def test_bf16_header_declares_exactly_the_four_functions():
    assert bf16_header_functions() == BF16_API
    src = open(os.path.join(REPO, "include", "dfwfm_bf16.h")).read()
    assert re.search(r"#define\s+DFWFM_BF16_ABI_VERSION\s+1\b", src)


def test_library_exports_the_bf16_symbols(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in BF16_API:
        assert hasattr(L, name), name
    assert set(built.BF16_SIGNATURES) == set(bf16_header_functions())
    # the other two headers' sets are pinned on their own
    assert not set(built.BF16_SIGNATURES) & set(built.SIGNATURES)
    assert not set(built.BF16_SIGNATURES) & set(built.SERVE_SIGNATURES)
    assert "dfwfm_bf16.hip" in built.SOURCES


def test_bf16_abi_version_and_null_arguments(built):
    L = built.lib()
    assert L.dfwfm_bf16_abi_version() == 1
    # invalid arguments are reported, never abort (no HIP call is reached)
    n = ctypes.c_size_t(0)
    assert L.dfwfm_bf16_forward(None, None, 0, None, 0, 1, None, None, 0, None) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_model_pack_bf16(None, 1, None) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_model_pack_bf16(None, 0, None) == -1
    assert L.dfwfm_bf16_workspace_bytes(None, 1, ctypes.byref(n)) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_bf16_workspace_bytes(None, 1, None) == -1


def test_mlp_dtype_flag_reaches_the_module():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    assert p.parse_args([]).mlp_dtype == "f32"
    with pytest.raises(SystemExit):
        p.parse_args(["-mlp_dtype", "fp8"])
    sizes = [1] * 13 + [7] * 26
    for flag in ("f32", "bf16"):
        pars = p.parse_args(["-mlp_dtype", flag])
        m = get_model(cuda=False, feature_sizes=sizes, pars=pars)
        assert m.mlp_dtype == flag
        assert "mlp_dtype" not in "".join(m.state_dict())  # derived state: the state_dict is unchanged
    assert DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_cuda=False).mlp_dtype == "f32"
    # the reference's fbgemm axis stays refused
    with pytest.raises(NotImplementedError):
        get_model(cuda=False, feature_sizes=sizes, pars=p.parse_args([]), static_quantization=True)
