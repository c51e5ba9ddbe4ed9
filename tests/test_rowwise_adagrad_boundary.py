"""CPU: the C boundary of the row-wise Adagrad step (include/dfwfm_rowwise_adagrad.h) -- its own header and ABI version
in the same libdfwfm.so, the other headers' function lists untouched --, every invalid argument, the host function
dfwfm_rowwise_adagrad_row_ref against an independent numpy statement of the header (tests/rowwise_adagrad_ref.py), the
corner in which the element-wise Adagrad coincides, a row on which the order of the chain is observable, and the
switch's plumbing (CLI, module, FusedTrainStep's and fit()'s refusals); no compute on the device without a GPU.

Every comparison is bit for bit."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import optim_ref
import rowwise_adagrad_ref as ref
from conftest import REPO

f32 = np.float32
ROWWISE_API = ["dfwfm_rowwise_adagrad_abi_version", "dfwfm_rowwise_adagrad_row_ref", "dfwfm_rowwise_adagrad_step_dev",
               "dfwfm_rowwise_adagrad_step_dev_sched"]
LAZY_OPTIM_API = ["dfwfm_lazy_optim_abi_version", "dfwfm_lazy_optim_step_dev", "dfwfm_lazy_optim_step_dev_sched"]
LAZY_ADAM_API = ["dfwfm_lazy_adam_abi_version", "dfwfm_lazy_adam_step_dev"]
LAZY_LISTS_API = ["dfwfm_lazy_adam_lists_step_dev", "dfwfm_lazy_adam_lists_step_dev_sched",
                  "dfwfm_lazy_lists_abi_version", "dfwfm_lazy_optim_lists_step_dev",
                  "dfwfm_lazy_optim_lists_step_dev_sched"]
OPTIM_API = ["dfwfm_optim_abi_version", "dfwfm_optim_elem_ref", "dfwfm_optim_step", "dfwfm_optim_step_dev",
             "dfwfm_optim_step_dev_sched"]
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


def test_header_declares_exactly_its_four_functions_and_states_the_contract():
    assert header_functions("dfwfm_rowwise_adagrad.h") == ROWWISE_API
    raw = open(os.path.join(REPO, "include", "dfwfm_rowwise_adagrad.h")).read()
    assert re.search(r"#define\s+DFWFM_ROWWISE_ADAGRAD_ABI_VERSION\s+1\b", raw)
    assert "dfwfm_rowwise_table" in raw and "DFWFM_LAZY_PLAIN" in raw and "dfwfm_optim_hyper" in raw
    assert not re.search(r"#define\s+DFWFM_LAZY_(PLAIN|QUOTIENT|REMAINDER)", raw)  # reused, not redefined
    assert "dfwfm_lazy_optim.h\"" not in raw  # the rules are restated, not left to the other header
    src = " ".join(raw.replace("*", " ").split())
    for phrase in ("touched", "clamp", "step counter", "weight decay acts on touched rows only", "zeroed gradient",
                   "updated once", "2^32", "HIP graph", "bit-identical from run to run", "STILL advances",
                   "up to 60 tables per launch", "dfwfm_lr_schedule_eval(s)", "never NULL", "one float per row",
                   "ss = fmaf(g'_e, g'_e, ss)", "The summation order IS the contract", "not a tree",
                   "not a per-lane partial sum", "contraction off", "eps == 0 is accepted", "0 / 0",
                   "NOT torch.optim.Adagrad", "There is no dense form", "power of two up to 16",
                   "neither read nor written", "no allocation", "a kind other than DFWFM_OPTIM_ADAGRAD"):
        assert phrase in src, phrase


def test_the_other_headers_are_untouched():
    assert header_functions("dfwfm_optim.h") == OPTIM_API
    assert header_functions("dfwfm_lazy_adam.h") == LAZY_ADAM_API
    assert header_functions("dfwfm_lazy_optim.h") == LAZY_OPTIM_API
    assert header_functions("dfwfm_lazy_lists.h") == LAZY_LISTS_API
    main = header_functions("dfwfm.h")
    assert len(main) == 35 and not any("lazy" in f or "optim" in f or "rowwise" in f for f in main)
    for name in sorted(os.listdir(os.path.join(REPO, "include"))):
        if name != "dfwfm_rowwise_adagrad.h":
            assert "rowwise" not in open(os.path.join(REPO, "include", name)).read(), name


def test_library_exports_the_symbols_and_the_binding_matches(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in ROWWISE_API:
        assert hasattr(L, name), name
    assert set(built.ROWWISE_ADAGRAD_SIGNATURES) == set(ROWWISE_API)
    for other in (built.SIGNATURES, built.SERVE_SIGNATURES, built.BF16_SIGNATURES, built.BF16_FUSED_SIGNATURES,
                  built.FOLD_SIGNATURES, built.BF16_FOLD_SIGNATURES, built.CPU_SIGNATURES, built.INGEST_SIGNATURES,
                  built.LAZY_ADAM_SIGNATURES, built.LR_SCHEDULE_SIGNATURES, built.OPTIM_SIGNATURES,
                  built.INT8_SIGNATURES, built.HALF_TABLES_SIGNATURES, built.INT8_TABLES_SIGNATURES,
                  built.LAZY_OPTIM_SIGNATURES, built.LAZY_LISTS_SIGNATURES):
        assert not set(built.ROWWISE_ADAGRAD_SIGNATURES) & set(other)
    assert any(h.endswith(os.path.join("include", "dfwfm_rowwise_adagrad.h")) for h in built.HEADERS)
    assert "dfwfm_rowwise_adagrad.h" in built.HEADERS and "dfwfm_rowwise_adagrad.hip" in built.SOURCES
    assert built.lib().dfwfm_rowwise_adagrad_abi_version() == 1
    # the descriptor's layout is the header's: four pointers, three int64, four int32
    assert ctypes.sizeof(built.dfwfm_rowwise_table) == 4 * 8 + 3 * 8 + 4 * 4
    assert [f[0] for f in built.dfwfm_rowwise_table._fields_] == [
        "param", "grad", "state", "stamp", "rows", "key_range", "c", "width", "column", "kind", "reserved"]


# ------------------------------------------------------------------------------------------- invalid arguments
def _table(built, **kw):
    """A descriptor with fake non-null pointers: an invalid one is refused before anything is dereferenced."""
    d = dict(param=0x1000, grad=0x2000, state=0x3000, stamp=0x5000, rows=7, key_range=7, c=0, width=10, column=0,
             kind=0, reserved=0)
    d.update(kw)
    return (built.dfwfm_rowwise_table * 1)(built.dfwfm_rowwise_table(**d))


def test_invalid_arguments_of_the_two_entry_points(built):
    """Invalid arguments return DFWFM_ERR_INVALID_ARG (-1) with a message and never abort; no HIP call is reached
    (this process has no device: a launch would return DFWFM_ERR_HIP)."""
    L = built.lib()
    nan, inf = float("nan"), float("inf")
    good = optim_ref.hyper("adag", LR, 3e-7)

    def calls(tabs, n=1, xi=0x6000, stride=1, batch=4, state=0x7000, h=good, block=0x8000):
        hp = None if h is None else ctypes.byref(h)
        x = ctypes.c_void_p(xi) if xi else None
        st = ctypes.c_void_p(state) if state else None
        return [("dev", lambda: L.dfwfm_rowwise_adagrad_step_dev(tabs, n, x, stride, batch, hp, st, None)),
                ("sched", lambda: L.dfwfm_rowwise_adagrad_step_dev_sched(tabs, n, x, stride, batch, hp,
                                                                         ctypes.c_void_p(block) if block else None,
                                                                         st, None))]

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
    refused(b"null state pointer", _table(built, state=None))  # the row's accumulator is never optional
    for bad, word in ((dict(width=0), b"width"), (dict(rows=0), b"rows"), (dict(key_range=0), b"key_range"),
                      (dict(kind=3), b"kind"), (dict(kind=-1), b"kind"), (dict(kind=1, c=0), b"c < 1"),
                      (dict(kind=2, c=0), b"c < 1"), (dict(column=-1), b"column"), (dict(column=1), b"column"),
                      (dict(key_range=8), b"reaches"),                    # plain: key 7 has no row
                      (dict(kind=1, c=4, key_range=29), b"reaches"),     # quotient: 28 / 4 = row 7 of 7
                      (dict(kind=2, c=8, key_range=23), b"reaches")):    # remainder: row 7 of 7
        refused(word, _table(built, **bad))
    # the largest key range that fits passes that check (and is refused for the width here: no device is reached)
    refused(b"width", _table(built, kind=1, c=4, key_range=28, width=0))
    # the kind must be Adagrad: the other kinds of include/dfwfm_optim.h are refused, as unknown ones are
    for kind in ("sgd", "rmsp"):
        refused(b"not DFWFM_OPTIM_ADAGRAD", ok, h=optim_ref.hyper(kind, LR))
    for kind in (-1, 3, 77):
        refused(b"unknown optimizer kind", ok, h=optim_ref.hyper(kind, LR))
    for field in ("lr", "weight_decay", "momentum", "alpha", "eps"):
        for bad, word in ((nan, b"NaN"), (inf, b"infinite"), (-inf, b"negative"), (-1e-9, b"negative")):
            h = optim_ref.hyper("adag", LR, 1e-2)
            setattr(h, field, bad)
            refused(field.encode(), ok, h=h, only=("dev",) if field == "lr" else None)  # (a schedule replaces lr)
            assert word in L.dfwfm_last_error()
    h = optim_ref.hyper("adag", LR)
    h.alpha = 1.0
    refused(b"alpha", ok, h=h)


def test_invalid_arguments_of_the_host_function(built):
    L = built.lib()
    p, g, acc = (ctypes.c_float * 4)(1, 2, 3, 4), (ctypes.c_float * 4)(1, 1, 1, 1), ctypes.c_float(0.5)
    good = optim_ref.hyper("adag", LR)
    F = ctypes.POINTER(ctypes.c_float)

    def call(h=good, width=4, p=p, g=g, acc=ctypes.byref(acc)):
        return L.dfwfm_rowwise_adagrad_row_ref(None if h is None else ctypes.byref(h), width,
                                               p if p is None else ctypes.cast(p, F),
                                               g if g is None else ctypes.cast(g, F),
                                               acc if acc is None else ctypes.cast(acc, F))
    for kw, word in ((dict(h=None), b"null hyper"), (dict(width=0), b"width"), (dict(width=-3), b"width"),
                     (dict(p=None), b"null"), (dict(g=None), b"null"), (dict(acc=None), b"null"),
                     (dict(h=optim_ref.hyper("sgd", LR)), b"not DFWFM_OPTIM_ADAGRAD"),
                     (dict(h=optim_ref.hyper("adag", float("nan"))), b"lr")):
        assert call(**kw) == -1 and word in L.dfwfm_last_error(), (kw, L.dfwfm_last_error())
        assert list(p) == [1, 2, 3, 4] and acc.value == 0.5  # a refused call writes nothing
    assert call() == 0 and list(g) == [1, 1, 1, 1] and acc.value == 1.5 and list(p) != [1, 2, 3, 4]


# ------------------------------------------------------------------------------------------- the host function
def _rows(width, seed, zero_acc, n=64):
    """Random rows: parameters ~ N(0, 1), gradient magnitudes 1e-8 .. 1, an accumulator zero or as after earlier
    steps."""
    r = np.random.default_rng(seed)
    p = r.standard_normal((n, width)).astype(f32)
    g = (r.standard_normal((n, width)) * 10.0 ** r.uniform(-8, 0, (n, width))).astype(f32)
    acc = np.zeros(n, f32) if zero_acc else np.abs(0.1 * r.standard_normal(n)).astype(f32)
    return p, g, acc


@pytest.mark.parametrize("zero_acc", [True, False], ids=["acc-zero", "acc-nonzero"])
@pytest.mark.parametrize("eps", [1e-10, 0.0])
@pytest.mark.parametrize("wd", [0.0, 3e-7])
@pytest.mark.parametrize("width", [1, 4, 10, 16, 17, 33])
def test_host_function_equals_the_numpy_statement_of_the_header(built, width, wd, eps, zero_acc):
    p, g, acc = _rows(width, 100 * width + int(zero_acc), zero_acc)
    g0 = g.copy()
    np_p, np_acc = ref.np_rows(p, g, acc, lr=LR, wd=wd, eps=eps)
    lib_p, lib_acc = ref.lib_rows(ref.hyper(LR, wd, eps), p, g, acc)
    assert optim_ref.same_bits(np_p, lib_p) and optim_ref.same_bits(np_acc, lib_acc)
    assert np.array_equal(g, g0)  # the gradient is only read
    assert not np.array_equal(lib_p, p) and np.all(lib_acc >= acc) and np.any(lib_acc > acc)
    assert not np.isnan(lib_p).any()


def test_host_function_with_eps_zero_gives_nan_on_a_zero_row_with_a_zero_accumulator(built):
    """0 / 0, as torch's Adagrad with eps == 0; with the default eps the same row keeps its bits."""
    p = np.array([[1.0, -2.0, 3.0]], f32)
    z = np.zeros((1, 3), f32)
    for elem in (lambda e: ref.lib_rows(ref.hyper(LR, 0.0, e), p, z, np.zeros(1, f32)),
                 lambda e: ref.np_rows(p, z, np.zeros(1, f32), lr=LR, eps=e)):
        q, acc = elem(0.0)
        assert np.isnan(q).all() and acc[0] == 0
        q, acc = elem(1e-10)
        assert np.array_equal(q, p) and acc[0] == 0


@pytest.mark.parametrize("width", [1, 2, 4, 8, 16])
def test_witness_corner_equals_the_elementwise_adagrad(built, width):
    """weight_decay == 0, a width that is a power of two up to 16 and every gradient of a row +-2^k for the row's k:
    ss / width is exactly 2^(2k), and acc + 2^(2k) rounded once is fmaf(g, g, acc) -- the element-wise Adagrad
    (optim_ref.np_step, and the library's dfwfm_optim_elem_ref) on a `sum` row that is the accumulator broadcast gives
    the same parameters, and a `sum` row that is the new accumulator in every element."""
    r = np.random.default_rng(width)
    n = 64
    k = r.integers(-12, 3, n)
    g = (np.ldexp(1.0, k)[:, None] * r.choice([-1.0, 1.0], (n, width))).astype(f32)
    p = r.standard_normal((n, width)).astype(f32)
    acc = np.abs(0.1 * r.standard_normal(n)).astype(f32)
    acc[::4] = 0
    s = np.repeat(acc[:, None], width, 1)
    want_p, want_s = optim_ref.np_step("adag", 1, p, g, s, lr=LR)
    lib_p, lib_s = optim_ref.lib_step(optim_ref.hyper("adag", LR), 1, p, g, s)
    assert optim_ref.same_bits(want_p, lib_p) and optim_ref.same_bits(want_s, lib_s)
    assert np.array_equal(want_s, np.repeat(want_s[:, :1], width, 1))
    for got_p, got_acc in (ref.lib_rows(ref.hyper(LR), p, g, acc), ref.np_rows(p, g, acc, lr=LR)):
        assert optim_ref.same_bits(got_p, want_p) and optim_ref.same_bits(got_acc, want_s[:, 0])
    assert not np.array_equal(want_p, p)


def test_witness_corner_does_not_extend_to_other_rows(built):
    """A width that is no power of two, or gradients of mixed magnitude: the row-wise update is another optimizer."""
    r = np.random.default_rng(3)
    p = r.standard_normal((8, 10)).astype(f32)
    g = r.standard_normal((8, 10)).astype(f32)
    acc = np.zeros(8, f32)
    want_p, _ = optim_ref.np_step("adag", 1, p, g, np.zeros_like(p), lr=LR)
    got_p, _ = ref.lib_rows(ref.hyper(LR), p, g, acc)
    assert not np.array_equal(got_p, want_p)


# a row of width 10 (found by a search over random rows) on which the sequential chain and a pairwise tree of the same
# squares differ: in ss, in the accumulator, and in the parameters
ORDER_G = np.array([0xbf49ace8, 0xbfbeae25, 0x3f39d84c, 0x3f217ce5, 0x3ee94664, 0xbf1325d6, 0x3f91a143, 0x40555884,
                    0x3dcd0329, 0x3eeda73b], np.uint32).view(f32)[None, :]
ORDER_SS_CHAIN, ORDER_SS_TREE = 0x41877aee, 0x41877aed
ORDER_ACC_CHAIN, ORDER_ACC_TREE = 0x3fd8c4b0, 0x3fd8c4ae


def test_the_order_of_the_chain_is_observable(built):
    bits = lambda a: int(np.asarray(a, f32).view(np.uint32).reshape(-1)[0])  # noqa: E731
    assert bits(ref.chain_ss(ORDER_G)) == ORDER_SS_CHAIN and bits(ref.tree_ss(ORDER_G)) == ORDER_SS_TREE
    p = np.ones((1, 10), f32)
    chain = ref.np_rows(p, ORDER_G, np.zeros(1, f32), lr=LR)
    tree = ref.np_rows(p, ORDER_G, np.zeros(1, f32), lr=LR, ss_of=ref.tree_ss)
    assert bits(chain[1]) == ORDER_ACC_CHAIN and bits(tree[1]) == ORDER_ACC_TREE
    assert not np.array_equal(chain[0], tree[0])
    lib = ref.lib_rows(ref.hyper(LR), p, ORDER_G, np.zeros(1, f32))
    assert bits(lib[1]) == ORDER_ACC_CHAIN and optim_ref.same_bits(lib[0], chain[0])  # the library runs the chain


def test_reference_helper_updates_touched_rows_only(built):
    """tests/rowwise_adagrad_ref.py's table form: the clamp, the QR kinds, untouched rows are copies, touched gradient
    rows are zero, and its two element functions agree."""
    p, g, acc = _rows(10, 5, False, n=7)
    for keys, key_range, kind, c, rows in (([3, 5, 3], 7, ref.PLAIN, 1, [3, 5]), ([-1, 7, 100], 7, ref.PLAIN, 1, [0]),
                                           ([22, 5, 23, 9], 23, ref.QUOTIENT, 4, [0, 1, 2, 5]),
                                           ([22, 5, 23, 9], 23, ref.REMAINDER, 4, [0, 1, 2])):
        a = ref.rowwise_ref(p, g, acc, keys, key_range, kind, c, lr=LR, weight_decay=3e-7)
        b = ref.rowwise_ref(p, g, acc, keys, key_range, kind, c, lr=LR, weight_decay=3e-7, elem="lib")
        for x, y in zip(a, b):
            assert optim_ref.same_bits(x, y)
        rest = np.setdiff1d(np.arange(7), rows)
        assert np.array_equal(a[0][rest], p[rest]) and np.array_equal(a[1][rest], g[rest])
        assert np.array_equal(a[2][rest], acc[rest]) and not a[1][rows].any()
        assert np.all(a[2][rows] > acc[rows]) and not np.array_equal(a[0][rows], p[rows])


# --------------------------------------------------------------------------------------------------- the switch
def _sizes():
    return [1] * 13 + [7] * 26


def test_cli_flag_parses_and_reaches_the_module():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    assert p.parse_args([]).rowwise_adagrad == 0
    assert p.parse_args(["-rowwise_adagrad", "1"]).rowwise_adagrad == 1
    with pytest.raises(SystemExit):
        p.parse_args(["-rowwise_adagrad", "2"])
    for flag in (0, 1):
        m = get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args(["-rowwise_adagrad", str(flag)]))
        assert m.rowwise_adagrad is bool(flag) and m.lazy_tables is False and m.lazy_table_adam is False
        assert "rowwise" not in "".join(m.state_dict())  # a training switch, not state
    assert get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args([])).rowwise_adagrad is False
    assert DeepFMs(field_size=39, feature_sizes=_sizes(), numerical=13, use_cuda=False).rowwise_adagrad is False


@pytest.mark.parametrize("opt,fused_optimizer", [("adag", True), ("adag", False), ("adam", True), ("sgd", True)])
def test_fit_refuses_the_switch_off_the_fused_adagrad_step(opt, fused_optimizer):
    """A module on the CPU (autograd + torch.optim), whatever its optimizer_type and fused_optimizer: fit() raises
    before the first batch instead of training with another update; with the switch off the same call trains."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = _sizes()
    xi, xv = synth.synth_inputs(sizes, 13, 64, seed=2)
    y = (np.arange(64) % 2).astype(np.float32)
    m = DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1,
                h_depth=1, deep_nodes=16, n_epochs=1, batch_size=32, optimizer_type=opt, use_cuda=False)
    m.rowwise_adagrad = True
    m.fused_optimizer = fused_optimizer
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(ValueError, match="rowwise_adagrad"):
        m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    m.rowwise_adagrad = False
    m.fused_optimizer = False
    m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    assert any(not torch.equal(before[k], v) for k, v in m.state_dict().items())


def test_fused_step_has_the_switch_off_by_default_and_its_refusals():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd import _lib
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep, check_rowwise
    pars = inspect.signature(FusedTrainStep.__init__).parameters
    assert pars["rowwise_tables"].default is False and pars["lazy_tables"].default is False
    assert pars["optimizer"].default == "adam"
    check_rowwise("adag", False, None)  # the one accepted combination
    for opt in ("adam", "sgd", "rmsp"):
        with pytest.raises(ValueError, match="optimizer='adag'"):
            check_rowwise(opt, False, None)
    for opt in ("adam", "adag"):
        with pytest.raises(ValueError, match="lazy_table_adam"):
            check_rowwise(opt, True, None)
    with pytest.raises(NotImplementedError, match="dfwfm_lazy_lists_span") as e:
        check_rowwise("adag", False, object())
    assert "ONE offset" in str(e.value) and "state pointer per span" in str(e.value)
    # the constructor itself needs a device, with the switch as without
    m = DeepFMs(field_size=39, feature_sizes=_sizes(), numerical=13, use_cuda=False)
    with pytest.raises(_lib.DfwfmError, match="HIP device"):
        FusedTrainStep(m, 8, optimizer="adag", rowwise_tables=True)


def test_bench_tool_refuses_the_flag_without_fused_adagrad():
    """tools/bench_train.py --rowwise-tables needs --mode fused and --optimizer adag: refused while parsing, before any
    device call."""
    import subprocess
    import sys
    tool = os.path.join(REPO, "tools", "bench_train.py")
    for extra in (["--optimizer", "rmsp"], ["--optimizer", "adag", "--mode", "autograd"]):
        r = subprocess.run([sys.executable, tool, "--rowwise-tables"] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "--rowwise-tables needs" in r.stderr, r.stderr
