"""CPU: the one-launch bf16 forward's C boundary (include/dfwfm_bf16_fused.h) -- its own header and ABI version in the
same libdfwfm.so, bound separately from the other headers' function sets -- and the bf16_fused switch's plumbing; no
compute without a GPU."""
import ctypes
import os
import re

import pytest

from conftest import REPO

FUSED_API = ["dfwfm_bf16_fused_abi_version", "dfwfm_bf16_fused_forward", "dfwfm_bf16_fused_forward_batches",
             "dfwfm_bf16_fused_supported"]
BF16_API = ["dfwfm_bf16_abi_version", "dfwfm_bf16_forward", "dfwfm_bf16_workspace_bytes", "dfwfm_model_pack_bf16"]


@pytest.fixture(scope="module")
def built():
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.build()
    return _lib


def header_functions(name):
    src = open(os.path.join(REPO, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dfwfm_[a-z0-9_]+)\s*\(", src)))


def test_fused_header_declares_exactly_the_four_functions():
    assert header_functions("dfwfm_bf16_fused.h") == FUSED_API
    src = open(os.path.join(REPO, "include", "dfwfm_bf16_fused.h")).read()
    assert re.search(r"#define\s+DFWFM_BF16_FUSED_ABI_VERSION\s+1\b", src)
    # nothing was added to the per-layer path's header
    assert header_functions("dfwfm_bf16.h") == BF16_API


def test_library_exports_the_fused_symbols(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in FUSED_API:
        assert hasattr(L, name), name
    assert set(built.BF16_FUSED_SIGNATURES) == set(header_functions("dfwfm_bf16_fused.h"))
    for other in (built.SIGNATURES, built.SERVE_SIGNATURES, built.BF16_SIGNATURES, built.FOLD_SIGNATURES):
        assert not set(built.BF16_FUSED_SIGNATURES) & set(other)
    assert "dfwfm_bf16_fused.hip" in built.SOURCES


def test_fused_abi_version_and_null_arguments(built):
    L = built.lib()
    assert L.dfwfm_bf16_fused_abi_version() == 1
    # invalid arguments are reported, never abort (no HIP call is reached)
    v = ctypes.c_int(7)
    assert L.dfwfm_bf16_fused_forward(None, None, 0, None, 0, 1, None, None) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_bf16_fused_forward_batches(None, 1, None, 0, None, 0, 1, None, None) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_bf16_fused_forward_batches(None, 0, None, 0, None, 0, 0, None, None) == -1
    assert L.dfwfm_bf16_fused_supported(None, ctypes.byref(v)) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_bf16_fused_supported(None, None) == -1
    assert v.value == 7


def test_bf16_fused_flag_reaches_the_module():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    assert p.parse_args([]).bf16_fused == 0
    with pytest.raises(SystemExit):
        p.parse_args(["-bf16_fused", "2"])
    sizes = [1] * 13 + [7] * 26
    for flag in (0, 1):
        pars = p.parse_args(["-mlp_dtype", "bf16", "-bf16_fused", str(flag)])
        m = get_model(cuda=False, feature_sizes=sizes, pars=pars)
        assert m.bf16_fused is bool(flag) and m.mlp_dtype == "bf16"
        assert "bf16_fused" not in "".join(m.state_dict())  # derived state: the state_dict is unchanged
    assert get_model(cuda=False, feature_sizes=sizes, pars=p.parse_args([])).bf16_fused is False
    assert DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_cuda=False).bf16_fused is False
