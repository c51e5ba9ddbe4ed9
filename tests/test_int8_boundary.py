"""CPU: the int8 forward's C boundary (include/dfwfm_int8.h) -- its own header and ABI version in the same libdfwfm.so,
bound separately from the other headers' function sets -- and the mlp_dtype = "int8" switch's plumbing; no compute
without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

INT8_API = ["dfwfm_int8_abi_version", "dfwfm_int8_forward", "dfwfm_int8_forward_batches", "dfwfm_int8_supported",
            "dfwfm_model_pack_int8"]
OTHER_HEADERS = {
    "dfwfm_bf16.h": ["dfwfm_bf16_abi_version", "dfwfm_bf16_forward", "dfwfm_bf16_workspace_bytes",
                     "dfwfm_model_pack_bf16"],
    "dfwfm_bf16_fold.h": ["dfwfm_bf16_fold_abi_version", "dfwfm_model_fold_bf16"],
    "dfwfm_bf16_fused.h": ["dfwfm_bf16_fused_abi_version", "dfwfm_bf16_fused_forward",
                           "dfwfm_bf16_fused_forward_batches", "dfwfm_bf16_fused_supported"],
    "dfwfm_fold.h": ["dfwfm_fold_abi_version", "dfwfm_model_fold_numerical"],
    "dfwfm_lazy_adam.h": ["dfwfm_lazy_adam_abi_version", "dfwfm_lazy_adam_step_dev"],
    "dfwfm_serve.h": ["dfwfm_serve_abi_version", "dfwfm_serve_forward", "dfwfm_serve_workspace_bytes"],
}


@pytest.fixture(scope="module")
def built():
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.build()
    return _lib


def header_functions(name):
    src = open(os.path.join(REPO, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dfwfm_[a-z0-9_]+)\s*\(", src)))


def test_int8_header_declares_exactly_the_five_functions():
    assert header_functions("dfwfm_int8.h") == INT8_API
    src = open(os.path.join(REPO, "include", "dfwfm_int8.h")).read()
    assert re.search(r"#define\s+DFWFM_INT8_ABI_VERSION\s+1\b", src)


def test_other_headers_are_unchanged(built):
    for name, api in OTHER_HEADERS.items():
        assert header_functions(name) == api, name
    assert set(header_functions("dfwfm.h")) == set(built.SIGNATURES) and len(built.SIGNATURES) == 35


def test_library_exports_the_int8_symbols(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in INT8_API:
        assert hasattr(L, name), name
    assert set(built.INT8_SIGNATURES) == set(header_functions("dfwfm_int8.h"))
    for other in (built.SIGNATURES, built.SERVE_SIGNATURES, built.BF16_SIGNATURES, built.BF16_FUSED_SIGNATURES,
                  built.FOLD_SIGNATURES, built.BF16_FOLD_SIGNATURES, built.LAZY_ADAM_SIGNATURES):
        assert not set(built.INT8_SIGNATURES) & set(other)
    assert "dfwfm_int8.hip" in built.SOURCES


def test_int8_abi_version_and_null_arguments(built):
    L = built.lib()
    assert L.dfwfm_int8_abi_version() == 1
    # invalid arguments are reported, never abort (no HIP call is reached)
    v = ctypes.c_int(7)
    assert L.dfwfm_model_pack_int8(None, None) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_int8_forward(None, None, 0, None, 0, 1, None, None) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_int8_forward_batches(None, 1, None, 0, None, 0, 1, None, None) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_int8_forward_batches(None, 0, None, 0, None, 0, 0, None, None) == -1
    assert L.dfwfm_int8_supported(None, ctypes.byref(v)) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_int8_supported(None, None) == -1
    assert v.value == 7


def test_mlp_dtype_int8_reaches_the_module():
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    with pytest.raises(SystemExit):
        p.parse_args(["-mlp_dtype", "fp8"])
    sizes = [1] * 13 + [7] * 26
    m = get_model(cuda=False, feature_sizes=sizes, pars=p.parse_args(["-mlp_dtype", "int8"]))
    assert m.mlp_dtype == "int8"
    f32 = get_model(cuda=False, feature_sizes=sizes, pars=p.parse_args([]))
    assert f32.mlp_dtype == "f32"
    assert list(m.state_dict()) == list(f32.state_dict())  # derived state: the state_dict is unchanged


def test_cpu_module_with_int8_raises_at_forward():
    from xsdeepfwfm_deprecated_amd import DeepFMs, DfwfmError
    sizes = [1] * 13 + [7] * 26
    m = DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_cuda=False)
    m.eval()
    xi = torch.zeros(4, 26, 1, dtype=torch.int64)
    xv = torch.ones(4, 13)
    with torch.no_grad():
        ref = m(xi, xv)
        m.mlp_dtype = "int8"
        with pytest.raises(DfwfmError, match="int8"):
            m(xi, xv)
        m.mlp_dtype = "fp8"  # any other string: the ValueError as before
        with pytest.raises(ValueError, match="mlp_dtype must be"):
            m(xi, xv)
        m.mlp_dtype = "f32"
        assert np.array_equal(m(xi, xv).numpy(), ref.numpy())
