"""CPU: the fp16 serving copy's C boundary (include/dfwfm_half_tables.h) -- its own header and ABI version in the same
libdfwfm.so -- the table_dtype switch's plumbing, the rounding helper the GPU tests compare against, and what the
rounding costs in the float64 oracle; no GPU compute."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import half_tables_ref
from conftest import REPO, golden_names, load_golden
from oracle import dfwfm_oracle

HALF_API = ["dfwfm_half_tables_abi_version", "dfwfm_model_pack_tables_half", "dfwfm_model_serving_copy_bytes"]
INVALID_ARG, HIP_ERROR, STATE = -1, -3, -4


@pytest.fixture(scope="module")
def built():
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.build()
    return _lib


def header_functions(name):
    src = open(os.path.join(REPO, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dfwfm_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_exactly_the_three_functions():
    assert header_functions("dfwfm_half_tables.h") == HALF_API
    src = open(os.path.join(REPO, "include", "dfwfm_half_tables.h")).read()
    assert re.search(r"#define\s+DFWFM_HALF_TABLES_ABI_VERSION\s+1\b", src)


def test_library_exports_the_symbols_with_their_signatures(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in HALF_API:
        assert hasattr(L, name), name
    S = built.HALF_TABLES_SIGNATURES
    assert set(S) == set(HALF_API)
    P = ctypes.c_void_p
    assert S["dfwfm_model_pack_tables_half"] == (ctypes.c_int, [P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                                ctypes.POINTER(ctypes.c_int64), P])
    assert S["dfwfm_model_serving_copy_bytes"] == (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_int64)])
    for other in (built.SIGNATURES, built.SERVE_SIGNATURES, built.BF16_SIGNATURES, built.BF16_FUSED_SIGNATURES,
                  built.FOLD_SIGNATURES, built.BF16_FOLD_SIGNATURES, built.LAZY_ADAM_SIGNATURES,
                  built.INT8_SIGNATURES):
        assert not set(S) & set(other)
    assert len(built.SIGNATURES) == 35  # include/dfwfm.h is as it was
    fn = built.lib().dfwfm_model_pack_tables_half
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == S["dfwfm_model_pack_tables_half"][1]


def test_abi_version_and_null_arguments(built):
    L = built.lib()
    assert L.dfwfm_half_tables_abi_version() == 1
    en, over, nb = ctypes.c_int32(7), ctypes.c_int64(7), ctypes.c_int64(7)
    assert L.dfwfm_model_pack_tables_half(None, 1, ctypes.byref(en), ctypes.byref(over), None) == INVALID_ARG
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_model_pack_tables_half(None, 1, None, None, None) == INVALID_ARG
    assert L.dfwfm_model_serving_copy_bytes(None, ctypes.byref(nb)) == INVALID_ARG
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_model_serving_copy_bytes(None, None) == INVALID_ARG
    assert (en.value, over.value, nb.value) == (7, 7, 7)  # nothing written on an invalid call


def test_pack_tables_half_before_set_tables_is_a_state_error(built):
    """A model needs a HIP device to exist: where there is none dfwfm_model_create reports the HIP error (and this
    test ends there; tests/test_gpu_half_tables.py makes the same calls on a device)."""
    L = built.lib()
    cfg = built.dfwfm_config(field_size=39, numerical=13, embedding_size=10, use_fwfm=1, use_fm=0, use_logit=0,
                             use_deep=0, use_lw=1, use_fwlw=0, h_depth=1, deep_nodes=16)
    h = ctypes.c_void_p()
    rc = L.dfwfm_model_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc != 0:
        assert rc == HIP_ERROR and not torch.cuda.is_available()
        return
    try:
        en, over, nb = ctypes.c_int32(7), ctypes.c_int64(7), ctypes.c_int64(7)
        assert L.dfwfm_model_pack_tables_half(h, 1, ctypes.byref(en), ctypes.byref(over), None) == STATE
        assert b"set_tables" in L.dfwfm_last_error()
        assert (en.value, over.value) == (0, 0)
        assert L.dfwfm_model_pack_tables_half(h, 0, ctypes.byref(en), None, None) == 0  # dropping needs no tables
        assert L.dfwfm_model_serving_copy_bytes(h, ctypes.byref(nb)) == 0 and nb.value == 0
    finally:
        L.dfwfm_model_destroy(h)


def test_table_dtype_reaches_the_module():
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    with pytest.raises(SystemExit):
        p.parse_args(["-table_dtype", "bf16"])
    sizes = [1] * 13 + [7] * 26
    m = get_model(cuda=False, feature_sizes=sizes, pars=p.parse_args(["-table_dtype", "fp16"]))
    assert m.table_dtype == "fp16"
    f32 = get_model(cuda=False, feature_sizes=sizes, pars=p.parse_args([]))
    assert f32.table_dtype == "f32"
    assert list(m.state_dict()) == list(f32.state_dict())  # derived state: the state_dict is unchanged


def test_main_all_refuses_fp16_tables_without_a_device(capsys):
    if torch.cuda.is_available():
        return  # (the refusal is about a missing device)
    import main_all
    with pytest.raises(SystemExit):
        main_all.main(["-table_dtype", "fp16", "-use_cuda", "0"])
    assert "-table_dtype fp16" in capsys.readouterr().err


def test_cpu_module_with_fp16_tables_raises_at_forward():
    from xsdeepfwfm_deprecated_amd import DeepFMs, DfwfmError
    sizes = [1] * 13 + [7] * 26
    m = DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_cuda=False)
    assert m.table_dtype == "f32"
    m.eval()
    xi = torch.zeros(4, 26, 1, dtype=torch.int64)
    xv = torch.ones(4, 13)
    with torch.no_grad():
        ref = m(xi, xv)
        m.table_dtype = "fp16"
        with pytest.raises(DfwfmError, match="fp16"):
            m(xi, xv)
        m.table_dtype = "half"
        with pytest.raises(ValueError, match="table_dtype must be"):
            m(xi, xv)
        m.table_dtype = "f32"
        assert np.array_equal(m(xi, xv).numpy(), ref.numpy())
    m.table_dtype = "f16"
    with pytest.raises(ValueError, match="table_dtype must be"):  # a grad-mode forward validates it too
        m(xi, xv)


@pytest.mark.parametrize("name", ["deepfwfm_lw", "tiny_fwfm_lw", "deepfwfm_qr_mult", "deepfwfm_fwlw_lw", "logit"])
def test_rounded_params_touch_only_the_categorical_second_order(name):
    cfg, params, *_ = load_golden(name)
    r = half_tables_ref.rounded_params(cfg, params)
    assert list(r) == list(params)
    keys = set(half_tables_ref.categorical_second_order_keys(cfg, params))
    has_second = any(k.startswith("fm_2nd_embeddings.") for k in params)
    assert len(keys) >= (cfg["field_size"] - cfg["numerical"] if has_second else 0)
    assert not any(k.startswith(f"fm_2nd_embeddings.{f}.") for k in keys for f in range(cfg["numerical"]))
    changed = 0
    for k, v in params.items():
        assert r[k].dtype == v.dtype and r[k].shape == v.shape and r[k] is not v
        if k in keys:
            assert np.array_equal(r[k], v.astype(np.float16).astype(np.float32))
            changed += int(not np.array_equal(r[k], v))
        else:  # first order, numerical fields, R, lw / fwlw, the MLP: the same bits
            assert np.array_equal(r[k].view(np.uint32), v.view(np.uint32)), k
    assert changed > 0 or not keys


def test_rounding_is_nearest_even_with_subnormals():
    """The helper's cast on the values the GPU test seeds: ties to even, subnormals kept, 65519 down to 65504."""
    cfg = dict(numerical=0, field_size=1)
    v = np.array([[1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1e-6, 3e-8, -0.0, 65504.0, 65519.0, -65519.0]], np.float32)
    r = half_tables_ref.rounded_params(cfg, {"fm_2nd_embeddings.0.weight": v})["fm_2nd_embeddings.0.weight"][0]
    assert r[0] == 1.0 and r[1] == 1 + 2.0 ** -9  # ties: to the even mantissa
    assert r[2] == 17 * 2.0 ** -24 and r[3] == 2.0 ** -24 * 1  # subnormals: multiples of 2^-24, not flushed
    assert r[4] == 0 and np.signbit(r[4])
    assert r[5] == 65504.0 and r[6] == 65504.0 and r[7] == -65504.0 and np.all(np.isfinite(r))


def test_oracle_cost_of_the_rounding_is_finite(capsys):
    """What fp16 tables cost in the float64 oracle, per golden the copy covers: max |oracle(rounded) -
    oracle(original)| / max(1, |logit|), and the AUC change on tiny_deepfwfm_lw (printed: DESIGN.md section 3.15
    quotes these).  Asserted: finite."""
    from xsdeepfwfm_deprecated_amd import metrics
    lines = []
    for name in golden_names():
        cfg, params, xi, xv, y, *_ = load_golden(name)
        if cfg["qr_flag"] or cfg["use_fwlw"] or not (cfg["use_fwfm"] or cfg["use_fm"]):
            continue
        a = dfwfm_oracle.forward(cfg, params, xi, xv)
        b = dfwfm_oracle.forward(cfg, half_tables_ref.rounded_params(cfg, params), xi, xv)
        err = float(np.max(np.abs(b - a) / np.maximum(1.0, np.abs(a))))
        assert np.isfinite(err), name
        lines.append(f"half_tables oracle: {name}: max rel logit change {err:.3e}")
        if name == "tiny_deepfwfm_lw":
            p = lambda z: 1.0 / (1.0 + np.exp(-z))
            d = metrics.roc_auc_score(y, p(b)) - metrics.roc_auc_score(y, p(a))
            assert np.isfinite(d)
            lines.append(f"half_tables oracle: {name}: AUC change {d:+.3e}")
    assert len(lines) >= 4
    with capsys.disabled():
        print("\n" + "\n".join(lines))
