"""CPU: the C boundary of the row-lazy Adam step (include/dfwfm_lazy_adam.h) -- its own header and ABI version in the
same libdfwfm.so, the other headers' function lists untouched --, the lazy_table_adam switch's plumbing (CLI, module,
fit's refusal to train with another optimizer's semantics) and the reference helper's own bookkeeping
(tests/lazy_adam_ref.py); no compute on the device without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lazy_adam_ref as ref
from conftest import REPO

LAZY_API = ["dfwfm_lazy_adam_abi_version", "dfwfm_lazy_adam_step_dev"]
FOLD_API = ["dfwfm_bf16_fold_abi_version", "dfwfm_model_fold_bf16"]
FUSED_API = ["dfwfm_bf16_fused_abi_version", "dfwfm_bf16_fused_forward", "dfwfm_bf16_fused_forward_batches",
             "dfwfm_bf16_fused_supported"]
BF16_API = ["dfwfm_bf16_abi_version", "dfwfm_bf16_forward", "dfwfm_bf16_workspace_bytes", "dfwfm_model_pack_bf16"]
F32_FOLD_API = ["dfwfm_fold_abi_version", "dfwfm_model_fold_numerical"]
SERVE_API = ["dfwfm_serve_abi_version", "dfwfm_serve_forward", "dfwfm_serve_workspace_bytes"]


@pytest.fixture(scope="module")
def built():
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.build()
    return _lib


def header_functions(name):
    src = open(os.path.join(REPO, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dfwfm_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_exactly_its_two_functions():
    assert header_functions("dfwfm_lazy_adam.h") == LAZY_API
    src = open(os.path.join(REPO, "include", "dfwfm_lazy_adam.h")).read()
    assert re.search(r"#define\s+DFWFM_LAZY_ADAM_ABI_VERSION\s+1\b", src)


def test_header_states_the_contract():
    src = " ".join(open(os.path.join(REPO, "include", "dfwfm_lazy_adam.h")).read().replace("*", " ").split())
    for phrase in ("touched", "clamp", "step counter", "weight decay acts on touched rows only", "zeroed gradient",
                   "not a per-row count", "updated once", "2^32", "HIP graph", "bit-identical from run to run",
                   "STILL advances"):
        assert phrase in src, phrase


def test_the_other_headers_are_untouched():
    assert header_functions("dfwfm_bf16_fold.h") == FOLD_API
    assert header_functions("dfwfm_bf16_fused.h") == FUSED_API
    assert header_functions("dfwfm_bf16.h") == BF16_API
    assert header_functions("dfwfm_fold.h") == F32_FOLD_API
    assert header_functions("dfwfm_serve.h") == SERVE_API
    main = header_functions("dfwfm.h")
    assert len(main) == 35 and not any("lazy" in f for f in main)
    assert not any("lazy" in f for f in header_functions("dfwfm_cpu.h"))


def test_library_exports_the_symbols_and_the_binding_matches(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in LAZY_API:
        assert hasattr(L, name), name
    assert set(built.LAZY_ADAM_SIGNATURES) == set(header_functions("dfwfm_lazy_adam.h"))
    for other in (built.SIGNATURES, built.SERVE_SIGNATURES, built.BF16_SIGNATURES, built.BF16_FUSED_SIGNATURES,
                  built.FOLD_SIGNATURES, built.BF16_FOLD_SIGNATURES, built.CPU_SIGNATURES, built.INGEST_SIGNATURES):
        assert not set(built.LAZY_ADAM_SIGNATURES) & set(other)
    assert set(built.SIGNATURES) == set(header_functions("dfwfm.h"))
    assert any(h.endswith("dfwfm_lazy_adam.h") for h in built.HEADERS)  # a changed header rebuilds the library
    assert "dfwfm_lazy_adam.hip" in built.SOURCES
    # the descriptor's layout is the header's: five pointers, three int64, four int32
    assert ctypes.sizeof(built.dfwfm_lazy_adam_table) == 5 * 8 + 3 * 8 + 4 * 4
    assert [f[0] for f in built.dfwfm_lazy_adam_table._fields_] == [
        "param", "grad", "exp_avg", "exp_avg_sq", "stamp", "rows", "key_range", "c", "width", "column", "kind",
        "reserved"]


def _table(built, **kw):
    """A descriptor with fake non-null pointers: an invalid one is refused before anything is dereferenced."""
    d = dict(param=0x1000, grad=0x2000, exp_avg=0x3000, exp_avg_sq=0x4000, stamp=0x5000, rows=7, key_range=7, c=0,
             width=10, column=0, kind=0, reserved=0)
    d.update(kw)
    return (built.dfwfm_lazy_adam_table * 1)(built.dfwfm_lazy_adam_table(**d))


def _call(L, tabs, n=1, xi=0x6000, stride=1, batch=4, state=0x7000):
    return L.dfwfm_lazy_adam_step_dev(tabs, n, ctypes.c_void_p(xi) if xi else None, stride, batch, 1e-3, 0.9, 0.999,
                                      1e-8, 3e-7, ctypes.c_void_p(state) if state else None, None)


def test_abi_version_and_invalid_arguments(built):
    """Invalid arguments return DFWFM_ERR_INVALID_ARG (-1) with a message and never abort; no HIP call is reached
    (this process has no device: one would return DFWFM_ERR_HIP)."""
    L = built.lib()
    assert L.dfwfm_lazy_adam_abi_version() == 1
    ok = _table(built)
    assert _call(L, ok, state=0) == -1 and b"null" in L.dfwfm_last_error()
    assert _call(L, None) == -1 and b"null" in L.dfwfm_last_error()
    assert _call(L, ok, xi=0) == -1 and b"null" in L.dfwfm_last_error()
    assert _call(L, ok, n=-1) == -1 and b"negative" in L.dfwfm_last_error()
    assert _call(L, ok, batch=-1) == -1 and b"negative" in L.dfwfm_last_error()
    for field in ("param", "grad", "exp_avg", "exp_avg_sq", "stamp"):
        assert _call(L, _table(built, **{field: None})) == -1 and b"null" in L.dfwfm_last_error(), field
    for bad, word in ((dict(width=0), b"width"), (dict(rows=0), b"rows"), (dict(key_range=0), b"key_range"),
                      (dict(kind=3), b"kind"), (dict(kind=-1), b"kind"), (dict(kind=1, c=0), b"c < 1"),
                      (dict(kind=2, c=0), b"c < 1"), (dict(column=-1), b"column"), (dict(column=1), b"column"),
                      (dict(key_range=8), b"reaches"),                    # plain: key 7 has no row
                      (dict(kind=1, c=4, key_range=29), b"reaches"),     # quotient: 28 / 4 = row 7 of 7
                      (dict(kind=2, c=8, key_range=23), b"reaches")):    # remainder: row 7 of 7
        assert _call(L, _table(built, **bad)) == -1, bad
        assert word in L.dfwfm_last_error(), (bad, L.dfwfm_last_error())
    # the largest key ranges that fit pass validation (and then need a device: not called here)
    assert _call(L, _table(built, kind=1, c=4, key_range=28, width=0)) == -1 and b"width" in L.dfwfm_last_error()


def _sizes():
    return [1] * 13 + [7] * 26


def test_lazy_adam_flag_parses_and_reaches_the_module():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    assert p.parse_args([]).lazy_adam == 0
    assert p.parse_args(["-lazy_adam", "1"]).lazy_adam == 1
    with pytest.raises(SystemExit):
        p.parse_args(["-lazy_adam", "2"])
    for flag in (0, 1):
        m = get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args(["-lazy_adam", str(flag)]))
        assert m.lazy_table_adam is bool(flag)
        assert "lazy" not in "".join(m.state_dict())  # a training switch, not state
    assert get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args([])).lazy_table_adam is False
    assert DeepFMs(field_size=39, feature_sizes=_sizes(), numerical=13, use_cuda=False).lazy_table_adam is False


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_fit_refuses_the_switch_off_the_fused_step(opt):
    """A module on the CPU (torch.optim.Adam through autograd), or any optimizer but Adam: fit() raises before the
    first batch instead of training with dense semantics."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = _sizes()
    xi, xv = synth.synth_inputs(sizes, 13, 64, seed=2)
    y = (np.arange(64) % 2).astype(np.float32)
    m = DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1,
                h_depth=1, deep_nodes=16, n_epochs=1, batch_size=32, optimizer_type=opt, use_cuda=False)
    m.lazy_table_adam = True
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(ValueError, match="lazy_table_adam"):
        m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    m.lazy_table_adam = False  # the same call trains without the switch
    m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    assert any(not torch.equal(before[k], v) for k, v in m.state_dict().items())


def test_fused_step_signature_has_the_switch_off_by_default():
    import inspect
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    assert inspect.signature(FusedTrainStep.__init__).parameters["lazy_table_adam"].default is False


# ------------------------------------------------------------------------------------- the reference helper itself
def _state(rows, width, seed):
    r = np.random.default_rng(seed)
    p = r.standard_normal((rows, width)).astype(np.float32)
    g = (r.standard_normal((rows, width)) * 10.0 ** r.integers(-8, 1, (rows, width))).astype(np.float32)
    return p, g, np.zeros_like(p), np.zeros_like(p)


def _torch_adam_rows(p, gs, steps, **kw):
    """torch.optim.Adam on one compact tensor whose state.step is preset before each of `steps` (global numbers)."""
    q = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([q], foreach=False, **kw)
    for g, s in zip(gs, steps):
        q.grad = torch.from_numpy(g.copy())
        if opt.state[q]:
            opt.state[q]["step"] = torch.tensor(float(s - 1))
        else:
            assert s == 1
        opt.step()
    return q.detach().numpy(), opt.state[q]["exp_avg"].numpy(), opt.state[q]["exp_avg_sq"].numpy()


def test_reference_touched_rows_mapping_and_clamp():
    assert ref.touched_rows([5, 2, 2, -1, 23, 22], 23).tolist() == [0, 2, 5, 22]
    assert ref.touched_rows([5, 2, 22, 23, -7], 23, ref.QUOTIENT, 4).tolist() == [0, 1, 5]
    assert ref.touched_rows([5, 2, 22, 23, -7], 23, ref.REMAINDER, 4).tolist() == [0, 1, 2]
    assert ref.touched_rows([], 23).size == 0


def test_reference_row_touched_at_steps_one_and_three_only():
    """Row 3 is touched at steps 1 and 3: at step 3 it gets step 3's bias corrections (the global step), and step 2
    leaves it alone (no moment decay, no weight decay); rows nobody touched never change."""
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=3e-7)
    p0, g1, m0, v0 = _state(9, 10, seed=1)
    g2, g3 = _state(9, 10, seed=2)[1], _state(9, 10, seed=3)[1]
    p, g, m, v = ref.lazy_adam_ref(p0, g1, m0, v0, [3, 7, 3], 9, 1, **kw)
    after1 = (p.copy(), m.copy(), v.copy())
    assert not g[[3, 7]].any() and np.array_equal(g[[0, 1, 2, 4, 5, 6, 8]], g1[[0, 1, 2, 4, 5, 6, 8]])
    p, g, m, v = ref.lazy_adam_ref(p, g2, m, v, [1, 2], 9, 2, **kw)
    for a, b in zip((p, m, v), after1):  # step 2 does not touch rows 3 and 7
        assert np.array_equal(a[[3, 7]], b[[3, 7]])
    p, g, m, v = ref.lazy_adam_ref(p, g3, m, v, [3, 4], 9, 3, **kw)
    want = _torch_adam_rows(p0[[3]], [g1[[3]], g3[[3]]], [1, 3], **kw)
    for a, b in zip((p, m, v), want):
        assert np.array_equal(a[[3]], b)
    # ... which is NOT what a per-row count (step 2 for the second update) would give
    other = _torch_adam_rows(p0[[3]], [g1[[3]], g3[[3]]], [1, 2], **kw)
    assert not np.array_equal(p[[3]], other[0])
    # and not the dense optimizer's either (its step 2 decays row 3's moments)
    dense = _torch_adam_rows(p0[[3]], [g1[[3]], np.zeros_like(g1[[3]]), g3[[3]]], [1, 2, 3], **kw)
    assert not np.array_equal(m[[3]], dense[1])
    untouched = [0, 5, 6, 8]
    assert np.array_equal(p[untouched], p0[untouched]) and not m[untouched].any() and not v[untouched].any()


def test_reference_out_of_range_keys_update_row_zero():
    p0, g0, m0, v0 = _state(7, 1, seed=4)
    p, g, m, v = ref.lazy_adam_ref(p0, g0, m0, v0, [-1, 7, 100], 7, 1, weight_decay=3e-7)
    assert p[0] != p0[0] and g[0] == 0 and m[0] != 0
    assert np.array_equal(p[1:], p0[1:]) and np.array_equal(g[1:], g0[1:]) and not m[1:].any() and not v[1:].any()
    # a touched row with an exactly zero gradient is still updated: weight decay acts, the moments move
    g0[:] = 0
    p, g, m, v = ref.lazy_adam_ref(p0, g0, m0, v0, [2], 7, 1, weight_decay=0.5)
    assert p[2] != p0[2] and m[2] != 0 and np.array_equal(np.delete(p, 2, 0), np.delete(p0, 2, 0))
