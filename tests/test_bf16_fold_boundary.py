"""CPU: the C boundary of the folded layer 1 of the one-launch bf16 forward (include/dfwfm_bf16_fold.h) -- its own header
and ABI version in the same libdfwfm.so, the other headers' function lists untouched -- and the bf16_fold switch's
plumbing; no compute without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden, model_kwargs

FOLD_API = ["dfwfm_bf16_fold_abi_version", "dfwfm_model_fold_bf16"]
FUSED_API = ["dfwfm_bf16_fused_abi_version", "dfwfm_bf16_fused_forward", "dfwfm_bf16_fused_forward_batches",
             "dfwfm_bf16_fused_supported"]
BF16_API = ["dfwfm_bf16_abi_version", "dfwfm_bf16_forward", "dfwfm_bf16_workspace_bytes", "dfwfm_model_pack_bf16"]
F32_FOLD_API = ["dfwfm_fold_abi_version", "dfwfm_model_fold_numerical"]


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
    assert header_functions("dfwfm_bf16_fold.h") == FOLD_API
    src = open(os.path.join(REPO, "include", "dfwfm_bf16_fold.h")).read()
    assert re.search(r"#define\s+DFWFM_BF16_FOLD_ABI_VERSION\s+1\b", src)
    # the numeric contract is stated: the K order, how P is formed and rounded, the instruction
    for word in ("ascending", "accumulated in f64", "round to nearest even", "v_mfma_f32_16x16x32_bf16"):
        assert word in src, word


def test_the_other_headers_are_untouched():
    assert header_functions("dfwfm_bf16_fused.h") == FUSED_API
    assert header_functions("dfwfm_bf16.h") == BF16_API
    assert header_functions("dfwfm_fold.h") == F32_FOLD_API
    assert len(header_functions("dfwfm.h")) == 35 and not any("bf16" in f for f in header_functions("dfwfm.h"))


def test_library_exports_the_fold_symbols(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in FOLD_API:
        assert hasattr(L, name), name
    assert set(built.BF16_FOLD_SIGNATURES) == set(header_functions("dfwfm_bf16_fold.h"))
    for other in (built.SIGNATURES, built.SERVE_SIGNATURES, built.BF16_SIGNATURES, built.BF16_FUSED_SIGNATURES,
                  built.FOLD_SIGNATURES):
        assert not set(built.BF16_FOLD_SIGNATURES) & set(other)
    assert set(built.SIGNATURES) == set(header_functions("dfwfm.h"))
    assert set(built.BF16_FUSED_SIGNATURES) == set(FUSED_API) and set(built.BF16_SIGNATURES) == set(BF16_API)
    assert any(h.endswith("dfwfm_bf16_fold.h") for h in built.HEADERS)  # a changed header rebuilds the library


def test_fold_abi_version_and_null_arguments(built):
    L = built.lib()
    assert L.dfwfm_bf16_fold_abi_version() == 1
    # invalid arguments are reported, never abort (no HIP call is reached)
    en = ctypes.c_int32(7)
    assert L.dfwfm_model_fold_bf16(None, 1, ctypes.byref(en), None) == -1
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_model_fold_bf16(None, 0, ctypes.byref(en), None) == -1
    assert L.dfwfm_model_fold_bf16(None, 1, None, None) == -1
    assert b"null" in L.dfwfm_last_error()
    assert en.value == 7


def test_bf16_fold_flag_reaches_the_module():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    assert p.parse_args([]).bf16_fold == 0
    with pytest.raises(SystemExit):
        p.parse_args(["-bf16_fold", "2"])
    sizes = [1] * 13 + [7] * 26
    for flag in (0, 1):
        pars = p.parse_args(["-mlp_dtype", "bf16", "-bf16_fused", "1", "-bf16_fold", str(flag)])
        m = get_model(cuda=False, feature_sizes=sizes, pars=pars)
        assert m.bf16_fold is bool(flag) and m.bf16_fused is True and m.mlp_dtype == "bf16"
        assert "bf16_fold" not in "".join(m.state_dict())  # derived state: the state_dict is unchanged
    assert get_model(cuda=False, feature_sizes=sizes, pars=p.parse_args([])).bf16_fold is False
    assert DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_cuda=False).bf16_fold is False


def test_asking_for_the_fold_on_a_cpu_model_changes_nothing():
    """A module on the CPU runs the host library's f32 forward: the switch alone (mlp_dtype f32) is ignored."""
    from xsdeepfwfm_deprecated_amd import DeepFMs
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    m = DeepFMs(**model_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m.eval()
    with torch.no_grad():
        want = m(torch.from_numpy(xi[:32]), torch.from_numpy(xv[:32])).numpy()
        m.bf16_fused = m.bf16_fold = True
        got = m(torch.from_numpy(xi[:32]), torch.from_numpy(xv[:32])).numpy()
    assert np.array_equal(got, want)


def test_the_emulation_of_the_exact_case_equals_the_oracle():
    """The helper's own check (bf16_fold_emul.exact_case asserts it): P exact in bf16, the folded contract the float64
    oracle bit for bit; and on a golden the folded contract is another rounding than the unfolded one."""
    import bf16_fold_emul
    cfg, params, xi, xv, ref = bf16_fold_emul.exact_case()
    assert ref.dtype == np.float32 and ref.shape == (96,)
    cfg, params, xi, xv, y, r, ef = bf16_fold_emul.golden_case("deepfwfm_lw")
    import bf16_emul
    eu = bf16_emul.golden_case("deepfwfm_lw")[6]
    assert ef.shape == eu.shape == r.shape and not np.array_equal(ef, eu)
