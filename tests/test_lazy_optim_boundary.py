"""CPU: the C boundary of the row-lazy SGD / Adagrad / RMSprop step (include/dfwfm_lazy_optim.h) -- its own header and
ABI version in the same libdfwfm.so, the other headers' function lists untouched --, every invalid argument, the
lazy_tables switch's plumbing (CLI, module, fit's refusal to train through the dense update) and the reference helper's
own bookkeeping (tests/lazy_optim_ref.py) against torch.optim on the compacted rows; no compute on the device without a
GPU.

Against torch.optim 2.10 (foreach=False) on a 7 x 10 table at global steps 1 and 3, weight_decay 0 and 3e-7: SGD's
parameters and momentum buffer, Adagrad's sum and RMSprop's square_avg bit-identical; Adagrad's and RMSprop's parameters
within one rounding (one unit in the last place of the parameter), the bar include/dfwfm_optim.h states."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import lazy_optim_ref as ref
import optim_ref
from conftest import REPO

LAZY_OPTIM_API = ["dfwfm_lazy_optim_abi_version", "dfwfm_lazy_optim_step_dev", "dfwfm_lazy_optim_step_dev_sched"]
LAZY_ADAM_API = ["dfwfm_lazy_adam_abi_version", "dfwfm_lazy_adam_step_dev"]
OPTIM_API = ["dfwfm_optim_abi_version", "dfwfm_optim_elem_ref", "dfwfm_optim_step", "dfwfm_optim_step_dev",
             "dfwfm_optim_step_dev_sched"]
VARIANTS = [("sgd", 0.0), ("sgd", 0.9), ("adag", 0.0), ("rmsp", 0.0)]
IDS = ["sgd", "sgd-momentum", "adag", "rmsp"]
LR = 1e-3


@pytest.fixture(scope="module")
def built():
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.build()
    return _lib


def header_functions(name):
    src = open(os.path.join(REPO, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dfwfm_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_exactly_its_three_functions_and_states_the_contract():
    assert header_functions("dfwfm_lazy_optim.h") == LAZY_OPTIM_API
    raw = open(os.path.join(REPO, "include", "dfwfm_lazy_optim.h")).read()
    assert re.search(r"#define\s+DFWFM_LAZY_OPTIM_ABI_VERSION\s+1\b", raw)
    assert "dfwfm_lazy_optim_table" in raw and "DFWFM_LAZY_PLAIN" in raw
    assert not re.search(r"#define\s+DFWFM_LAZY_(PLAIN|QUOTIENT|REMAINDER)", raw)  # reused, not redefined
    src = " ".join(raw.replace("*", " ").split())
    for phrase in ("touched", "clamp", "step counter", "weight decay acts on touched rows only", "zeroed gradient",
                   "not a per-row count", "updated once", "2^32", "HIP graph", "bit-identical from run to run",
                   "STILL advances", "GLOBAL step", "at global step 1", "coincides bit for bit", "do NOT coincide",
                   "up to 60 tables per launch", "dfwfm_optim_elem_ref", "dfwfm_lr_schedule_eval(s)",
                   "may be NULL", "null state where the optimizer needs one"):
        assert phrase in src, phrase


def test_the_other_headers_are_untouched():
    assert header_functions("dfwfm_optim.h") == OPTIM_API
    assert header_functions("dfwfm_lazy_adam.h") == LAZY_ADAM_API
    main = header_functions("dfwfm.h")
    assert len(main) == 35 and not any("lazy" in f or "optim" in f for f in main)
    for name in ("dfwfm.h", "dfwfm_optim.h", "dfwfm_lazy_adam.h", "dfwfm_lr_schedule.h"):
        assert "lazy_optim" not in open(os.path.join(REPO, "include", name)).read(), name


def test_library_exports_the_symbols_and_the_binding_matches(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in LAZY_OPTIM_API:
        assert hasattr(L, name), name
    assert set(built.LAZY_OPTIM_SIGNATURES) == set(header_functions("dfwfm_lazy_optim.h"))
    for other in (built.SIGNATURES, built.SERVE_SIGNATURES, built.BF16_SIGNATURES, built.BF16_FUSED_SIGNATURES,
                  built.FOLD_SIGNATURES, built.BF16_FOLD_SIGNATURES, built.CPU_SIGNATURES, built.INGEST_SIGNATURES,
                  built.LAZY_ADAM_SIGNATURES, built.LR_SCHEDULE_SIGNATURES, built.OPTIM_SIGNATURES,
                  built.INT8_SIGNATURES, built.HALF_TABLES_SIGNATURES, built.INT8_TABLES_SIGNATURES):
        assert not set(built.LAZY_OPTIM_SIGNATURES) & set(other)
    assert any(h.endswith(os.path.join("include", "dfwfm_lazy_optim.h")) for h in built.HEADERS)
    assert "dfwfm_lazy_optim.h" in built.HEADERS and "dfwfm_lazy_optim.hip" in built.SOURCES
    assert built.lib().dfwfm_lazy_optim_abi_version() == 1
    # the descriptor's layout is the header's: four pointers, three int64, four int32
    assert ctypes.sizeof(built.dfwfm_lazy_optim_table) == 4 * 8 + 3 * 8 + 4 * 4
    assert [f[0] for f in built.dfwfm_lazy_optim_table._fields_] == [
        "param", "grad", "state", "stamp", "rows", "key_range", "c", "width", "column", "kind", "reserved"]
    assert (built.LAZY_PLAIN, built.LAZY_QUOTIENT, built.LAZY_REMAINDER) == (0, 1, 2)


# ------------------------------------------------------------------------------------------- invalid arguments
def _table(built, **kw):
    """A descriptor with fake non-null pointers: an invalid one is refused before anything is dereferenced."""
    d = dict(param=0x1000, grad=0x2000, state=0x3000, stamp=0x5000, rows=7, key_range=7, c=0, width=10, column=0,
             kind=0, reserved=0)
    d.update(kw)
    return (built.dfwfm_lazy_optim_table * 1)(built.dfwfm_lazy_optim_table(**d))


def test_abi_version_and_invalid_arguments(built):
    """Invalid arguments return DFWFM_ERR_INVALID_ARG (-1) with a message and never abort; no HIP call is reached
    (this process has no device: a launch would return DFWFM_ERR_HIP)."""
    L = built.lib()
    assert L.dfwfm_lazy_optim_abi_version() == 1
    nan, inf = float("nan"), float("inf")
    good = optim_ref.hyper("rmsp", LR, 3e-7)

    def calls(tabs, n=1, xi=0x6000, stride=1, batch=4, state=0x7000, h=good, block=0x8000):
        hp = None if h is None else ctypes.byref(h)
        x = ctypes.c_void_p(xi) if xi else None
        st = ctypes.c_void_p(state) if state else None
        return [("dev", lambda: L.dfwfm_lazy_optim_step_dev(tabs, n, x, stride, batch, hp, st, None)),
                ("sched", lambda: L.dfwfm_lazy_optim_step_dev_sched(tabs, n, x, stride, batch, hp,
                                                                    ctypes.c_void_p(block) if block else None, st,
                                                                    None))]

    def refused(word, *a, only=None, **kw):
        for name, call in calls(*a, **kw):
            if only is None or name in only:
                assert call() == -1, (name, word)
                assert word in L.dfwfm_last_error(), (name, word, L.dfwfm_last_error())

    ok = _table(built)
    refused(b"null state block", ok, state=0)
    refused(b"null table array", None)
    refused(b"null xi", ok, xi=0)
    refused(b"xi_stride", ok, stride=0)
    refused(b"negative table count", ok, n=-1)
    refused(b"negative batch", ok, batch=-1)
    refused(b"null hyper", ok, h=None)
    refused(b"null schedule", ok, block=0, only=("sched",))
    for field in ("param", "grad", "stamp"):
        refused(b"null pointer", _table(built, **{field: None}))
    # a null state where the kind needs one; plain SGD needs none (and then fails later, on something else)
    for kind, mom in (("adag", 0.0), ("rmsp", 0.0), ("sgd", 0.9)):
        refused(b"null state pointer", _table(built, state=None), h=optim_ref.hyper(kind, LR, 0.0, mom))
    refused(b"width", _table(built, state=None, width=0), h=optim_ref.hyper("sgd", LR))
    for bad, word in ((dict(width=0), b"width"), (dict(rows=0), b"rows"), (dict(key_range=0), b"key_range"),
                      (dict(kind=3), b"kind"), (dict(kind=-1), b"kind"), (dict(kind=1, c=0), b"c < 1"),
                      (dict(kind=2, c=0), b"c < 1"), (dict(column=-1), b"column"), (dict(column=1), b"column"),
                      (dict(key_range=8), b"reaches"),                    # plain: key 7 has no row
                      (dict(kind=1, c=4, key_range=29), b"reaches"),     # quotient: 28 / 4 = row 7 of 7
                      (dict(kind=2, c=8, key_range=23), b"reaches")):    # remainder: row 7 of 7
        refused(word, _table(built, **bad))
    # the largest key ranges that fit pass that check (and are refused for the width here: no device is reached)
    refused(b"width", _table(built, kind=1, c=4, key_range=28, width=0))
    # the hyper-parameters: dfwfm_optim_step_dev's checks
    for kind in (-1, 3, 77):
        refused(b"unknown optimizer kind", ok, h=optim_ref.hyper(kind, LR))
    for field in ("lr", "weight_decay", "momentum", "alpha", "eps"):
        for bad, word in ((nan, b"NaN"), (inf, b"infinite"), (-inf, b"negative"), (-1e-9, b"negative")):
            for kind in ("sgd", "adag", "rmsp"):
                h = optim_ref.hyper(kind, LR, 1e-2, 0.9)
                setattr(h, field, bad)
                # (a scheduled call does not read lr)
                refused(field.encode(), ok, h=h, only=("dev",) if field == "lr" else None)
                assert word in L.dfwfm_last_error()
    for alpha in (1.0, 1.5):
        h = optim_ref.hyper("rmsp", LR)
        h.alpha = alpha
        refused(b"alpha", ok, h=h)


# --------------------------------------------------------------------------------------------------- the switch
def _sizes():
    return [1] * 13 + [7] * 26


def test_cli_flag_parses_and_reaches_the_module():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    assert p.parse_args([]).lazy_tables == 0
    assert p.parse_args(["-lazy_tables", "1"]).lazy_tables == 1
    with pytest.raises(SystemExit):
        p.parse_args(["-lazy_tables", "2"])
    for flag in (0, 1):
        m = get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args(["-lazy_tables", str(flag)]))
        assert m.lazy_tables is bool(flag) and m.lazy_table_adam is False
        assert "lazy" not in "".join(m.state_dict())  # a training switch, not state
    assert get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args([])).lazy_tables is False
    assert DeepFMs(field_size=39, feature_sizes=_sizes(), numerical=13, use_cuda=False).lazy_tables is False


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_fit_refuses_the_switch_off_the_fused_step(opt):
    """A module on the CPU (autograd + torch.optim): fit() raises before the first batch instead of training with the
    dense update; with the switch off the same call trains, as before."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = _sizes()
    xi, xv = synth.synth_inputs(sizes, 13, 64, seed=2)
    y = (np.arange(64) % 2).astype(np.float32)
    m = DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1,
                h_depth=1, deep_nodes=16, n_epochs=1, batch_size=32, optimizer_type=opt, use_cuda=False)
    m.lazy_tables = True
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(ValueError, match="lazy_tables"):
        m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    m.lazy_tables = False
    m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    assert any(not torch.equal(before[k], v) for k, v in m.state_dict().items())


def test_fused_step_signature_has_the_switch_off_by_default():
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    pars = inspect.signature(FusedTrainStep.__init__).parameters
    assert pars["lazy_tables"].default is False
    assert pars["lazy_table_adam"].default is False and pars["optimizer"].default == "adam"


# ------------------------------------------------------------------------------------- the reference helper itself
def _state(rows, width, seed, opt, mom):
    r = np.random.default_rng(seed)
    p = r.standard_normal((rows, width)).astype(np.float32)
    g = (r.standard_normal((rows, width)) * 10.0 ** r.integers(-8, 1, (rows, width))).astype(np.float32)
    return p, g, (np.zeros_like(p) if optim_ref.has_state(opt, mom) else None)


@pytest.mark.parametrize("opt,mom", [("sgd", 0.9), ("rmsp", 0.0)], ids=["sgd-momentum", "rmsp"])
def test_reference_row_touched_at_steps_one_and_three_only(built, opt, mom):
    """Row 3 is touched at steps 1 and 3: step 2 leaves its parameters and state alone (no decay, no weight decay, no
    move by the momentum buffer), which is not what the dense optimizer does; step 3 is the element function at step 3
    on what step 1 left.  Rows nobody touched never change."""
    kw = dict(lr=LR, weight_decay=3e-7, momentum=mom)
    p0, g1, s0 = _state(9, 10, 1, opt, mom)
    g2, g3 = _state(9, 10, 2, opt, mom)[1], _state(9, 10, 3, opt, mom)[1]
    p, g, s = ref.lazy_optim_ref(opt, p0, g1, s0, [3, 7, 3], 9, 1, **kw)
    after1 = (p.copy(), s.copy())
    assert not g[[3, 7]].any() and np.array_equal(g[[0, 1, 2, 4, 5, 6, 8]], g1[[0, 1, 2, 4, 5, 6, 8]])
    assert not np.array_equal(p[[3, 7]], p0[[3, 7]]) and s[[3, 7]].any()
    p, g, s = ref.lazy_optim_ref(opt, p, g2, s, [1, 2], 9, 2, **kw)
    for a, b in zip((p, s), after1):  # step 2 does not touch rows 3 and 7
        assert np.array_equal(a[[3, 7]], b[[3, 7]])
    p, g, s = ref.lazy_optim_ref(opt, p, g3, s, [3, 4], 9, 3, **kw)
    h = optim_ref.hyper(opt, LR, 3e-7, mom)
    wp, ws = optim_ref.lib_step(h, 3, after1[0][3], g3[3], after1[1][3])
    assert optim_ref.same_bits(p[3], wp) and optim_ref.same_bits(s[3], ws)
    # ... which is NOT the dense optimizer's result (its step 2, on a zero gradient, decays row 3's state and moves it)
    dp, ds = optim_ref.lib_step(h, 2, after1[0][3], np.zeros(10, np.float32), after1[1][3])
    dp, ds = optim_ref.lib_step(h, 3, dp, g3[3], ds)
    assert not np.array_equal(s[3], ds) and not np.array_equal(p[3], dp)
    untouched = [0, 5, 6, 8]
    assert np.array_equal(p[untouched], p0[untouched]) and not s[untouched].any()


def test_reference_momentum_sgd_copies_the_gradient_at_global_step_one_only(built):
    """The copy rule is the GLOBAL step's: at step 1 the buffer's old contents are not read and a -0 gradient keeps its
    sign; a row first touched at step 3 gets round(0 * momentum) + g', where -0 becomes +0."""
    f = np.float32
    p0 = np.ones((4, 1), f)
    g = np.array([[-0.0], [0.25], [0.0], [0.0]], f)
    s = np.full((4, 1), 123.0, f)
    p1, g1, s1 = ref.lazy_optim_ref("sgd", p0, g, s, [0, 1], 4, 1, lr=LR, momentum=0.9)
    assert optim_ref.bits(s1[0])[0] == optim_ref.bits(f(-0.0)) and s1[1, 0] == f(0.25)  # copies
    assert s1[2, 0] == f(123.0) and not g1[[0, 1]].any()
    fresh = np.zeros((4, 1), f)
    p3, g3, s3 = ref.lazy_optim_ref("sgd", p0, g, fresh, [0, 1], 4, 3, lr=LR, momentum=0.9)
    assert optim_ref.bits(s3[0])[0] == optim_ref.bits(f(0.0)) and s3[1, 0] == f(0.25)   # 0 * 0.9 + -0 = +0
    p3b, _, s3b = ref.lazy_optim_ref("sgd", p0, g, s, [1], 4, 3, lr=LR, momentum=0.9)
    assert s3b[1, 0] == f(f(123.0) * f(0.9)) + f(0.25) and p3b[1, 0] != p1[1, 0]      # the buffer is read at step 3
    # the library's element function agrees on all of it
    for step, start in ((1, s), (3, fresh), (3, s)):
        a = ref.lazy_optim_ref("sgd", p0, g, start, [0, 1], 4, step, lr=LR, momentum=0.9)
        b = ref.lazy_optim_ref("sgd", p0, g, start, [0, 1], 4, step, lr=LR, momentum=0.9, elem="lib")
        assert optim_ref.same_bits(a[0], b[0]) and optim_ref.same_bits(a[2], b[2])


def test_reference_out_of_range_keys_update_row_zero_and_a_zero_gradient_row_is_updated(built):
    p0, g0, s0 = _state(7, 1, 4, "adag", 0.0)
    p, g, s = ref.lazy_optim_ref("adag", p0, g0, s0, [-1, 7, 100], 7, 1, lr=LR, weight_decay=3e-7)
    assert p[0] != p0[0] and g[0] == 0 and s[0] != 0
    assert np.array_equal(p[1:], p0[1:]) and np.array_equal(g[1:], g0[1:]) and not s[1:].any()
    assert ref.lazy_optim_ref("sgd", p0, g0, None, [1], 7, 1, lr=LR)[2] is None  # plain SGD has no state
    # a touched row with an exactly zero gradient is still updated: weight decay acts, the state moves
    g0[:] = 0
    p, g, s = ref.lazy_optim_ref("rmsp", p0, g0, s0, [2], 7, 1, lr=LR, weight_decay=0.5)
    assert p[2] != p0[2] and s[2] != 0 and np.array_equal(np.delete(p, 2, 0), np.delete(p0, 2, 0))


def _torch_rows(opt, mom, p, g, s, step, wd):
    """torch.optim on compact rows, its state preset to what the global step `step` starts from."""
    q = torch.from_numpy(p.copy()).requires_grad_(True)
    q.grad = torch.from_numpy(g.copy())
    o = optim_ref.torch_optimizer(opt, [q], LR, wd, mom)
    if opt == "sgd":
        if mom != 0.0 and step > 1:
            o.state[q]["momentum_buffer"] = torch.from_numpy(s.copy())
    else:
        o.state[q] = {"step": torch.tensor(float(step - 1)), optim_ref.TORCH_STATE[opt]: torch.from_numpy(s.copy())}
    o.step()
    st = o.state[q].get(optim_ref.TORCH_STATE[opt]) if optim_ref.has_state(opt, mom) else None
    return q.detach().numpy(), (None if st is None else st.numpy())


@pytest.mark.parametrize("wd", [0.0, 3e-7])
@pytest.mark.parametrize("opt,mom", VARIANTS, ids=IDS)
def test_reference_against_torch_optim_on_the_compacted_rows(built, opt, mom, wd):
    """A 7 x 10 table at global steps 1 and 3 (row 3 in both, rows 5 / 4 and 0 in one each; key 9 clamps to row 0):
    the helper's touched rows against torch.optim's single-tensor step on the compacted rows, from the helper's own
    state before each step; and the helper's two element functions (numpy, library) against one another."""
    p, _, s = _state(7, 10, 11, opt, mom)
    for step, keys in ((1, [3, 5, 3]), (3, [3, 4, 9])):
        g = _state(7, 10, 20 + step, opt, mom)[1]
        rows = ref.touched_rows(keys, 7)
        assert rows.tolist() == ([3, 5] if step == 1 else [0, 3, 4])
        np_, ng, ns = ref.lazy_optim_ref(opt, p, g, s, keys, 7, step, lr=LR, weight_decay=wd, momentum=mom)
        lp, lg, ls = ref.lazy_optim_ref(opt, p, g, s, keys, 7, step, lr=LR, weight_decay=wd, momentum=mom, elem="lib")
        assert optim_ref.same_bits(np_, lp) and np.array_equal(ng, lg)
        tp, ts = _torch_rows(opt, mom, p[rows], g[rows], None if s is None else s[rows], step, wd)
        rest = np.setdiff1d(np.arange(7), rows)
        assert np.array_equal(np_[rest], p[rest]) and np.array_equal(ng[rest], g[rest]) and not ng[rows].any()
        if ns is not None:
            assert np.array_equal(ns[rest], s[rest])
            assert np.array_equal(optim_ref.bits(ns[rows]), optim_ref.bits(ts)), (opt, step, "state")
            assert optim_ref.same_bits(ns, ls)
        if opt == "sgd":
            assert np.array_equal(optim_ref.bits(np_[rows]), optim_ref.bits(tp)), (opt, step, "p")
        else:  # within one rounding
            assert np.all(np.abs(np_[rows] - tp) <= np.spacing(np.maximum(np.abs(np_[rows]), np.abs(tp)))), (opt, step)
        assert not np.array_equal(np_[rows], p[rows])
        p, s = np_, ns
