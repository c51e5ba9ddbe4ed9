"""CPU: the int8 serving copy's C boundary (include/dfwfm_int8_tables.h) -- its own header and ABI version in the same
libdfwfm.so -- the table_dtype switch's plumbing, the quantizer of the helper the GPU tests compare against, and what
the quantization costs in the float64 oracle; no GPU compute."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import int8_tables_ref
from conftest import REPO, golden_names, load_golden
from oracle import dfwfm_oracle

INT8_API = ["dfwfm_int8_tables_abi_version", "dfwfm_model_pack_tables_int8"]
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


def test_header_declares_exactly_the_two_functions():
    assert header_functions("dfwfm_int8_tables.h") == INT8_API
    src = open(os.path.join(REPO, "include", "dfwfm_int8_tables.h")).read()
    assert re.search(r"#define\s+DFWFM_INT8_TABLES_ABI_VERSION\s+1\b", src)


def test_library_exports_the_symbols_with_their_signatures(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in INT8_API:
        assert hasattr(L, name), name
    S = built.INT8_TABLES_SIGNATURES
    assert set(S) == set(INT8_API)
    P = ctypes.c_void_p
    assert S["dfwfm_int8_tables_abi_version"] == (ctypes.c_int, [])
    assert S["dfwfm_model_pack_tables_int8"] == (ctypes.c_int, [P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                                ctypes.POINTER(ctypes.c_int64), P])
    for other in (built.SIGNATURES, built.SERVE_SIGNATURES, built.BF16_SIGNATURES, built.BF16_FUSED_SIGNATURES,
                  built.FOLD_SIGNATURES, built.BF16_FOLD_SIGNATURES, built.LAZY_ADAM_SIGNATURES,
                  built.INT8_SIGNATURES, built.HALF_TABLES_SIGNATURES):
        assert not set(S) & set(other)
    fn = built.lib().dfwfm_model_pack_tables_int8
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == S["dfwfm_model_pack_tables_int8"][1]


def test_abi_version_and_null_arguments(built):
    L = built.lib()
    assert L.dfwfm_int8_tables_abi_version() == 1
    en, bad = ctypes.c_int32(7), ctypes.c_int64(7)
    assert L.dfwfm_model_pack_tables_int8(None, 1, ctypes.byref(en), ctypes.byref(bad), None) == INVALID_ARG
    assert b"null" in L.dfwfm_last_error()
    assert L.dfwfm_model_pack_tables_int8(None, 1, None, None, None) == INVALID_ARG
    assert L.dfwfm_model_pack_tables_int8(None, 0, ctypes.byref(en), None, None) == INVALID_ARG
    assert (en.value, bad.value) == (7, 7)  # nothing written on an invalid call


def test_pack_tables_int8_before_set_tables_is_a_state_error(built):
    """A model needs a HIP device to exist: where there is none dfwfm_model_create reports the HIP error (and this
    test ends there; tests/test_gpu_int8_tables.py makes the same calls on a device)."""
    L = built.lib()
    cfg = built.dfwfm_config(field_size=39, numerical=13, embedding_size=10, use_fwfm=1, use_fm=0, use_logit=0,
                             use_deep=0, use_lw=1, use_fwlw=0, h_depth=1, deep_nodes=16)
    h = ctypes.c_void_p()
    rc = L.dfwfm_model_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc != 0:
        assert rc == HIP_ERROR and not torch.cuda.is_available()
        return
    try:
        en, bad, nb = ctypes.c_int32(7), ctypes.c_int64(7), ctypes.c_int64(7)
        assert L.dfwfm_model_pack_tables_int8(h, 1, ctypes.byref(en), ctypes.byref(bad), None) == STATE
        assert b"set_tables" in L.dfwfm_last_error()
        assert (en.value, bad.value) == (0, 0)
        assert L.dfwfm_model_pack_tables_int8(h, 0, ctypes.byref(en), None, None) == 0  # dropping needs no tables
        assert L.dfwfm_model_serving_copy_bytes(h, ctypes.byref(nb)) == 0 and nb.value == 0
    finally:
        L.dfwfm_model_destroy(h)


def test_table_dtype_reaches_the_module():
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    with pytest.raises(SystemExit):
        p.parse_args(["-table_dtype", "int4"])
    sizes = [1] * 13 + [7] * 26
    m = get_model(cuda=False, feature_sizes=sizes, pars=p.parse_args(["-table_dtype", "int8"]))
    assert m.table_dtype == "int8"
    f32 = get_model(cuda=False, feature_sizes=sizes, pars=p.parse_args([]))
    assert f32.table_dtype == "f32"
    assert list(m.state_dict()) == list(f32.state_dict())  # derived state: the state_dict is unchanged


def test_main_all_refuses_int8_tables_without_a_device(capsys):
    if torch.cuda.is_available():
        return  # (the refusal is about a missing device)
    import main_all
    with pytest.raises(SystemExit):
        main_all.main(["-table_dtype", "int8", "-use_cuda", "0"])
    assert "-table_dtype int8" in capsys.readouterr().err


def test_cpu_module_with_int8_tables_raises_at_forward():
    from xsdeepfwfm_deprecated_amd import DeepFMs, DfwfmError
    sizes = [1] * 13 + [7] * 26
    m = DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_cuda=False)
    assert m.table_dtype == "f32"
    m.eval()
    xi = torch.zeros(4, 26, 1, dtype=torch.int64)
    xv = torch.ones(4, 13)
    with torch.no_grad():
        ref = m(xi, xv)
        m.table_dtype = "int8"
        with pytest.raises(DfwfmError, match="table_dtype='int8'"):
            m(xi, xv)
        m.table_dtype = "int4"
        with pytest.raises(ValueError, match="^table_dtype must be .*'int8'"):
            m(xi, xv)
        m.table_dtype = "f32"
        assert np.array_equal(m(xi, xv).numpy().view(np.uint32), ref.numpy().view(np.uint32))
    m.table_dtype = "i8"
    with pytest.raises(ValueError, match="^table_dtype must be"):  # a grad-mode forward validates it too
        m(xi, xv)


@pytest.mark.parametrize("name", ["deepfwfm_lw", "tiny_fwfm_lw", "deepfwfm_qr_mult", "deepfwfm_fwlw_lw", "logit"])
def test_quantized_params_touch_only_the_categorical_second_order(name):
    cfg, params, *_ = load_golden(name)
    r = int8_tables_ref.quantized_params(cfg, params)
    assert list(r) == list(params)
    keys = set(int8_tables_ref.categorical_second_order_keys(cfg, params))
    has_second = any(k.startswith("fm_2nd_embeddings.") for k in params)
    assert len(keys) >= (cfg["field_size"] - cfg["numerical"] if has_second else 0)
    assert not any(k.startswith(f"fm_2nd_embeddings.{f}.") for k in keys for f in range(cfg["numerical"]))
    changed = 0
    for k, v in params.items():
        assert r[k].dtype == v.dtype and r[k].shape == v.shape and r[k] is not v
        if k in keys:
            q, s = int8_tables_ref.quantize_rows(v.reshape(-1, v.shape[-1]))
            assert q.dtype == np.int8 and q.min() >= -127 and s.dtype == np.float32
            assert np.all(s.view(np.uint32) & 0xFFFF == 0)  # a bf16
            assert np.array_equal(r[k].reshape(q.shape), q.astype(np.float32) * s[:, None])
            changed += int(not np.array_equal(r[k], v))
        else:  # first order, numerical fields, R, lw / fwlw, the MLP: the same bits
            assert np.array_equal(r[k].view(np.uint32), v.view(np.uint32)), k
    assert changed > 0 or not keys


# the rows the GPU test seeds too: (row, expected scale or None, expected q or None)
TIES = [127, .5, 1.5, 2.5, -.5, -1.5, 63.5, -126.5, 126.5, -127]
ODD254 = [1.0] + [(2 * i + 1) / 254.0 for i in range(9)]  # 1, 1/254, 3/254, ...: halves of t = 1/127
CRITICAL_ROWS = [
    [0.0] * 10,
    [1e-45] * 10,
    TIES,
    ODD254,
    [3e38, -1e38, 1.0, 0.0, 2e37, -3e38, 1e30, 5e36, -7e37, 2.9e38],
]


def test_quantizer_on_hand_made_rows():
    """The header's quantizer, step by step, on the rows where it can go wrong."""
    w = np.array(CRITICAL_ROWS, dtype=np.float32)
    q, s = int8_tables_ref.quantize_rows(w)
    d = int8_tables_ref.dequantized(w)
    # an all-zero row, and a row of the smallest subnormal: scale 0, zeros served
    for i in (0, 1):
        assert s[i] == 0 and not np.any(q[i]) and np.array_equal(d[i].view(np.uint32), np.zeros(10, np.uint32))
    # scale exactly 1: q = rint(w), ties to even (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 63.5 -> 64, 126.5 -> 126)
    assert s[2] == 1.0
    assert q[2].tolist() == [127, 0, 2, 2, 0, -2, 64, -126, 126, -127]
    assert d[2].tolist() == [127.0, 0.0, 2.0, 2.0, 0.0, -2.0, 64.0, -126.0, 126.0, -127.0]
    # t = 1/127 is no bf16: the scale is the next bf16 ABOVE it, so |w / s| <= 127 before the clamp
    t = np.float32(1.0) / np.float32(127.0)
    assert s[3] > t and (s[3].view(np.uint32) & 0xFFFF) == 0
    assert s[3].view(np.uint32) == (t.view(np.uint32) & 0xFFFF0000) + 0x10000
    assert np.abs(q[3].astype(int)).max() <= 127 and q[3][0] == np.rint(np.float32(1.0) / s[3])
    assert q[3].tolist() == np.rint(w[3] / s[3]).astype(int).tolist()
    # a maximum of 3e38 (beyond what the pack serves, within what the arithmetic holds): everything stays finite
    assert np.isfinite(s[4]) and np.all(np.isfinite(d[4])) and abs(int(q[4][0])) <= 127
    assert np.isfinite(np.float32(127.0) * s[4])
    # -128 never; q * s exact: the float32 product is the float64 product
    assert q.min() >= -127 and q.max() <= 127
    assert np.array_equal(d.astype(np.float64), q.astype(np.float64) * s.astype(np.float64)[:, None])


def test_oracle_cost_of_the_quantization(capsys):
    """What int8 tables cost in the float64 oracle, per golden the copy covers: max |oracle(quantized) -
    oracle(original)| / max(1, |logit|), and the AUC change on tiny_deepfwfm_lw (printed: DESIGN.md section 3.16
    quotes these).  Asserted: finite and <= 2e-3 -- a bar that a wrong quantizer (a per-table scale, say) misses; the
    quantizer is deterministic numpy and its worst figure is 7.9e-4, on fm_deep."""
    from xsdeepfwfm_deprecated_amd import metrics
    lines = []
    for name in golden_names():
        cfg, params, xi, xv, y, *_ = load_golden(name)
        if cfg["qr_flag"] or cfg["use_fwlw"] or not (cfg["use_fwfm"] or cfg["use_fm"]):
            continue
        a = dfwfm_oracle.forward(cfg, params, xi, xv)
        b = dfwfm_oracle.forward(cfg, int8_tables_ref.quantized_params(cfg, params), xi, xv)
        err = float(np.max(np.abs(b - a) / np.maximum(1.0, np.abs(a))))
        lines.append(f"int8_tables oracle: {name}: max rel logit change {err:.3e}")
        assert np.isfinite(err) and err <= 2e-3, lines[-1]
        if name == "tiny_deepfwfm_lw":
            p = lambda z: 1.0 / (1.0 + np.exp(-z))
            d = metrics.roc_auc_score(y, p(b)) - metrics.roc_auc_score(y, p(a))
            lines.append(f"int8_tables oracle: {name}: AUC change {d:+.3e}")
            assert np.isfinite(d) and abs(d) <= 2e-3, lines[-1]
    assert len(lines) >= 4
    with capsys.disabled():
        print("\n" + "\n".join(lines))
