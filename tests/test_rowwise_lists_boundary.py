"""CPU: the C boundary of the list-driven row-wise Adagrad step (include_dp/dfwfm_rowwise_lists.h) -- its own header and
ABI version in the same libdfwfm.so --, every invalid argument, the switch's plumbing (FusedTrainStep's keyword and
refusals, module, CLI, fit(), the bench tool's parse-time refusal), and a host emulation of the step (the union of the
lists' rows, then the row's arithmetic) against the key-driven reference on keys that touch the same rows; no compute
on the device without a GPU.

Every comparison is bit for bit."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import optim_ref
import rowwise_adagrad_ref as rw
import rowwise_lists_ref as ref
from conftest import REPO

f32 = np.float32
API = ["dfwfm_rowwise_adagrad_lists_step_dev", "dfwfm_rowwise_adagrad_lists_step_dev_sched",
       "dfwfm_rowwise_lists_abi_version"]
LR = 1e-3


@pytest.fixture(scope="module")
def built():
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.build()
    return _lib


def header_functions(name):
    src = open(os.path.join(REPO, "include_dp", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dfwfm_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_exactly_its_three_functions_and_states_the_contract():
    assert header_functions("dfwfm_rowwise_lists.h") == API
    raw = open(os.path.join(REPO, "include_dp", "dfwfm_rowwise_lists.h")).read()
    assert re.search(r"#define\s+DFWFM_ROWWISE_LISTS_ABI_VERSION\s+1\b", raw)
    assert re.search(r"#define\s+DFWFM_ROWWISE_LISTS_SPANS_PER_LAUNCH\s+\d+\b", raw)
    assert re.search(r"#define\s+DFWFM_ROWWISE_LISTS_LISTS_PER_LAUNCH\s+\d+\b", raw)
    assert "dfwfm_rowwise_lists_span" in raw and "dfwfm_lazy_lists_list" in raw
    assert "} dfwfm_lazy_lists_list;" not in raw  # the existing list type, not a second one
    src = " ".join(raw.replace("*", " ").split())
    for phrase in ("touched", "at least one list names its destination", "is skipped", "no address is formed",
                   "updated once", "STILL advances", "device-scope look", "atomic exchange", "2^32", "HIP graph",
                   "several launches", "no allocation", "bit-identical from run to run", "indexes the gradient ONLY",
                   "never NULL", "ss = fmaf(g'_e, g'_e, ss)", "The summation order IS the contract", "not a tree",
                   "not a per-lane partial sum", "contraction off", "dfwfm_rowwise_adagrad_row_ref",
                   "weight decay acts on touched rows only", "zeroed gradient", "eps == 0 is accepted",
                   "dfwfm_lr_schedule_eval(s)", "a kind other than DFWFM_OPTIM_ADAGRAD", "a null param, state or stamp",
                   "overlaps", "matches no span", "cap < 0", "cap / 256 above 2^30", "No call aborts"):
        assert phrase in src, phrase


def test_library_exports_the_symbols_and_the_binding_matches(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in API:
        assert hasattr(L, name), name
    assert set(built.ROWWISE_LISTS_SIGNATURES) == set(API)
    for other in (built.SIGNATURES, built.LAZY_ADAM_SIGNATURES, built.OPTIM_SIGNATURES, built.LAZY_OPTIM_SIGNATURES,
                  built.LAZY_LISTS_SIGNATURES, built.ROWWISE_ADAGRAD_SIGNATURES):
        assert not set(built.ROWWISE_LISTS_SIGNATURES) & set(other)
    assert any(h.endswith(os.path.join("include_dp", "dfwfm_rowwise_lists.h")) for h in built.HEADERS)
    assert "dfwfm_rowwise_lists.h" in built.HEADERS and "dfwfm_rowwise_lists.hip" in built.SOURCES
    assert built.lib().dfwfm_rowwise_lists_abi_version() == 1
    # the span's layout is the header's: three pointers, two int64, two int32; the list is the lazy lists' own
    assert ctypes.sizeof(built.dfwfm_rowwise_lists_span) == 3 * 8 + 2 * 8 + 2 * 4
    assert [f[0] for f in built.dfwfm_rowwise_lists_span._fields_] == ["param", "state", "stamp", "offset", "rows",
                                                                         "width", "reserved"]
    raw = open(os.path.join(REPO, "include_dp", "dfwfm_rowwise_lists.h")).read()
    for field in ("param", "state", "stamp", "offset", "rows", "width"):
        assert re.search(r"\b%s;" % field, raw), field
    limits = {k: int(v) for k, v in re.findall(r"#define\s+DFWFM_ROWWISE_LISTS_(\w+)_PER_LAUNCH\s+(\d+)", raw)}
    assert limits == {"SPANS": built.ROWWISE_LISTS_SPANS_PER_LAUNCH, "LISTS": built.ROWWISE_LISTS_LISTS_PER_LAUNCH}
    assert 1 <= limits["SPANS"] <= 64 and 1 <= limits["LISTS"] <= 32
    # the two row functions exist once: in the shared csrc header, called by both kernels
    csrc = os.path.join(REPO, "xsdeepfwfm_deprecated_amd", "csrc")
    text = {n: open(os.path.join(csrc, n)).read() for n in ("dfwfm_rowwise_adagrad.h", "dfwfm_rowwise_adagrad.hip",
                                                            "dfwfm_rowwise_lists.hip")}
    for fn in ("rowwise_update_one", "rowwise_update_group"):
        defined = {n: len(re.findall(r"void\s+%s\s*\(" % fn, t)) for n, t in text.items()}
        assert defined == {"dfwfm_rowwise_adagrad.h": 1, "dfwfm_rowwise_adagrad.hip": 0, "dfwfm_rowwise_lists.hip": 0}
        assert fn + "(c, " in text["dfwfm_rowwise_adagrad.hip"] and fn + "(c, " in text["dfwfm_rowwise_lists.hip"]


# ------------------------------------------------------------------------------------------- invalid arguments
def _spans(built, *descs):
    """Span descriptors with fake non-null pointers: an invalid one is refused before anything is dereferenced."""
    arr = (built.dfwfm_rowwise_lists_span * max(len(descs), 1))()
    for i, kw in enumerate(descs):
        d = dict(param=0x1000 + 0x100 * i, state=0x3000 + 0x100 * i, stamp=0x5000 + 0x100 * i, offset=80 * i, rows=7,
                 width=10, reserved=0)
        d.update(kw)
        arr[i] = built.dfwfm_rowwise_lists_span(**d)
    return arr, len(descs)


def _lists(built, *descs):
    arr = (built.dfwfm_lazy_lists_list * max(len(descs), 1))()
    for i, kw in enumerate(descs):
        d = dict(dest=0x9000, count=0xa000, cap=16, width=10, reserved=0)
        d.update(kw)
        arr[i] = built.dfwfm_lazy_lists_list(**d)
    return arr, len(descs)


def test_invalid_arguments_of_the_two_entry_points(built):
    """Invalid arguments return DFWFM_ERR_INVALID_ARG (-1) with a message and never abort; no HIP call is reached (this
    process has no device: a launch would return DFWFM_ERR_HIP)."""
    L = built.lib()
    P = ctypes.c_void_p
    nan, inf = float("nan"), float("inf")
    good = optim_ref.hyper("adag", LR, 3e-7)
    ok_s, ok_l = _spans(built, {}), _lists(built, {})

    def calls(sp=ok_s, ls=ok_l, grad=0x2000, state=0x7000, h=good, block=0x8000, null_spans=False, null_lists=False):
        (sa, ns), (la, nl) = sp, ls
        sa, la = (None if null_spans else sa), (None if null_lists else la)
        g, st, bl = (P(x) if x else None for x in (grad, state, block))
        hp = None if h is None else ctypes.byref(h)
        return [("dev", lambda: L.dfwfm_rowwise_adagrad_lists_step_dev(sa, ns, la, nl, g, hp, st, None)),
                ("sched", lambda: L.dfwfm_rowwise_adagrad_lists_step_dev_sched(sa, ns, la, nl, g, hp, bl, st, None))]

    def refused(word, only=None, rc=-1, **kw):
        for name, call in calls(**kw):
            if only is None or name in only:
                assert call() == rc, (name, word)
                assert word in L.dfwfm_last_error(), (name, word, L.dfwfm_last_error())

    refused(b"null state block", state=0)
    refused(b"null schedule", block=0, only=("sched",))
    refused(b"null grad", grad=0)
    refused(b"null span array", null_spans=True)
    refused(b"null list array", null_lists=True)
    refused(b"negative span count", sp=(ok_s[0], -1))
    refused(b"negative list count", ls=(ok_l[0], -1))
    refused(b"null hyper", h=None)
    # spans
    for bad, word in ((dict(param=None), b"null pointer"), (dict(stamp=None), b"null pointer"),
                      (dict(state=None), b"null state pointer"),  # the rows' accumulators are never optional
                      (dict(rows=0), b"rows"), (dict(rows=-3), b"rows"), (dict(width=0), b"width"),
                      (dict(width=-1), b"width"), (dict(offset=-4), b"negative offset"),
                      (dict(offset=2 ** 62, rows=2 ** 60), b"63 bits")):
        refused(word, sp=_spans(built, bad))
    refused(b"overlapping", sp=_spans(built, {}, dict(offset=69)))       # rows 0..6 of width 10 end at 70
    refused(b"overlapping", sp=_spans(built, dict(offset=69), dict(offset=0)))  # in any order
    refused(b"overlapping", sp=_spans(built, {}, dict(offset=0)))
    refused(b"cap < 0", sp=_spans(built, {}, dict(offset=70)), ls=_lists(built, dict(cap=-1)))  # adjacent spans pass
    # lists
    refused(b"cap < 0", ls=_lists(built, {}, dict(cap=-1)))
    refused(b"null pointer", ls=_lists(built, dict(dest=None)))
    refused(b"null pointer", ls=_lists(built, dict(count=None)))
    refused(b"matches no span", ls=_lists(built, dict(width=1)))
    refused(b"matches no span", ls=_lists(built, dict(width=0)))
    refused(b"matches no span", sp=(ok_s[0], 0))                          # no span at all: no list matches
    refused(b"too long", ls=_lists(built, dict(cap=256 * (2 ** 30 + 1))), rc=-2)  # DFWFM_ERR_UNSUPPORTED
    # the hyper-parameters: dfwfm_optim_step_dev's checks, and the kind is Adagrad
    for kind in ("sgd", "rmsp"):
        refused(b"not DFWFM_OPTIM_ADAGRAD", h=optim_ref.hyper(kind, LR))
    for kind in (-1, 3, 77):
        refused(b"unknown optimizer kind", h=optim_ref.hyper(kind, LR))
    for field in ("lr", "weight_decay", "momentum", "alpha", "eps"):
        for bad, word in ((nan, b"NaN"), (inf, b"infinite"), (-inf, b"negative"), (-1e-9, b"negative")):
            h = optim_ref.hyper("adag", LR, 1e-2)
            setattr(h, field, bad)
            refused(field.encode(), h=h, only=("dev",) if field == "lr" else None)  # (a schedule replaces lr)
            assert word in L.dfwfm_last_error()
    h = optim_ref.hyper("adag", LR)
    h.alpha = 1.0
    refused(b"alpha", h=h)


# --------------------------------------------------------------------------------------------------- the switch
def _sizes():
    return [1] * 13 + [7] * 26


def test_fused_step_has_the_switch_off_by_default_and_its_refusals():
    from xsdeepfwfm_deprecated_amd import DeepFMs, _lib
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep, check_rowwise, check_rowwise_exchange
    pars = inspect.signature(FusedTrainStep.__init__).parameters
    assert pars["rowwise_exchange"].default is False and pars["rowwise_tables"].default is False
    assert pars["lazy_exchange"].default is False and pars["sparse_exchange"].default is True
    assert "unless rowwise_exchange is on" in " ".join(FusedTrainStep.__doc__.split())
    # the three-argument form is what it was: the very NotImplementedError under dist
    sig = inspect.signature(check_rowwise).parameters
    assert list(sig)[:3] == ["optimizer", "lazy_table_adam", "dist"] and list(sig.values())[3].default is False
    for args in (("adag", False, object()), ("adag", False, object(), False)):
        with pytest.raises(NotImplementedError, match="dfwfm_lazy_lists_span") as e:
            check_rowwise(*args)
        assert "ONE offset" in str(e.value) and "state pointer per span" in str(e.value)
    check_rowwise("adag", False, object(), True)  # with the switch: accepted
    check_rowwise("adag", False, None, True)
    with pytest.raises(ValueError, match="optimizer='adag'"):
        check_rowwise("rmsp", False, object(), True)
    with pytest.raises(ValueError, match="lazy_table_adam"):
        check_rowwise("adag", True, object(), True)
    check_rowwise_exchange(True, object(), True)  # the one accepted combination
    with pytest.raises(ValueError, match="needs dist"):
        check_rowwise_exchange(True, None, True)
    with pytest.raises(ValueError, match="needs rowwise_tables"):
        check_rowwise_exchange(False, object(), True)
    with pytest.raises(ValueError, match="needs sparse_exchange"):
        check_rowwise_exchange(True, object(), False)
    # the constructor itself needs a device, with the switch as without
    m = DeepFMs(field_size=39, feature_sizes=_sizes(), numerical=13, use_cuda=False)
    with pytest.raises(_lib.DfwfmError, match="HIP device"):
        FusedTrainStep(m, 8, optimizer="adag", rowwise_tables=True, rowwise_exchange=True, dist=object())


def test_cli_flag_parses_and_reaches_the_module():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    assert p.parse_args([]).rowwise_exchange == 0
    assert p.parse_args(["-rowwise_exchange", "1"]).rowwise_exchange == 1
    with pytest.raises(SystemExit):
        p.parse_args(["-rowwise_exchange", "2"])
    for flag in (0, 1):
        m = get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args(["-rowwise_exchange", str(flag)]))
        assert m.rowwise_exchange is bool(flag) and m.rowwise_adagrad is False and m.lazy_exchange is False
        assert "rowwise" not in "".join(m.state_dict())  # a training switch, not state
    assert DeepFMs(field_size=39, feature_sizes=_sizes(), numerical=13, use_cuda=False).rowwise_exchange is False


@pytest.mark.parametrize("rowwise_adagrad", [False, True])
def test_fit_refuses_the_switch_off_the_fused_step(rowwise_adagrad):
    """A module on the CPU (autograd + torch.optim): fit() raises before the first batch instead of training through
    another path -- for the switch itself, or, with rowwise_adagrad set as well, for that."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = _sizes()
    xi, xv = synth.synth_inputs(sizes, 13, 64, seed=2)
    y = (np.arange(64) % 2).astype(np.float32)
    m = DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1,
                h_depth=1, deep_nodes=16, n_epochs=1, batch_size=32, optimizer_type="adag", use_cuda=False)
    m.rowwise_exchange = True
    m.rowwise_adagrad = rowwise_adagrad
    m.fused_optimizer = rowwise_adagrad
    with pytest.raises(ValueError, match="rowwise_adagrad" if rowwise_adagrad else "rowwise_exchange"):
        m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])


def test_bench_tool_refuses_the_flag_while_parsing():
    """tools/bench_train.py --rowwise-exchange needs --rowwise-tables and one of --exchange-world1 / --gpus N: refused
    while parsing, before any device call; the --rowwise-tables refusal keeps its words."""
    tool = os.path.join(REPO, "tools", "bench_train.py")
    for extra in (["--exchange-world1", "--optimizer", "adag"],       # no --rowwise-tables
                  ["--rowwise-tables", "--optimizer", "adag"]):      # no ranks
        r = subprocess.run([sys.executable, tool, "--rowwise-exchange"] + extra, capture_output=True, text=True,
                           env=dict(os.environ, WORLD_SIZE="1"))
        assert r.returncode == 2 and "--rowwise-exchange needs --rowwise-tables" in r.stderr, r.stderr
    r = subprocess.run([sys.executable, tool, "--rowwise-exchange", "--rowwise-tables", "--exchange-world1"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--rowwise-tables needs --mode fused and --optimizer adag" in r.stderr, r.stderr


# ------------------------------------------------------------------------------------- the host emulation
SPANS = [(0, 1, 10), (12, 7, 10), (84, 7, 1), (92, 5, 10), (144, 6, 17)]
TOTAL = 248


@pytest.mark.parametrize("elem", ["np", "lib"])
@pytest.mark.parametrize("wd", [0.0, 3e-7])
def test_host_emulation_equals_the_key_driven_reference_on_keys_that_touch_the_same_rows(built, elem, wd):
    """The union of the lists' rows, then the row's arithmetic on them: per span the result is rowwise_ref's (the
    key-driven step's reference) on keys that touch exactly those rows -- a row two lists name updated once --, the
    other rows, the other accumulators and the pads keep every bit, touched gradient rows are zero; np_rows and the
    library's host function agree."""
    r = np.random.default_rng(5)
    params = [r.standard_normal((rows, w)).astype(f32) for _, rows, w in SPANS]
    accs = [np.abs(0.1 * r.standard_normal(rows)).astype(f32) for _, rows, _ in SPANS]
    grad = (r.standard_normal(TOTAL) * 10.0 ** r.uniform(-8, 0, TOTAL)).astype(f32)
    lists = [(np.array([12, 32, 92, 999], np.int64), 3, 4, 10),       # the 4th entry lies behind the count
             (np.array([32, 122, 0, 17, 84, 144], np.int64), 9, 6, 10),  # 17: mid-row; 84, 144: spans of other widths
             (np.array([86, 84, 91], np.int64), 3, 3, 1),             # 91: the pad
             (np.array([86], np.int64), 1, 2, 1), (np.array([85], np.int64), -3, 1, 1),
             (np.array([144 + 17 * 5, 144 + 17, 150, 246], np.int64), 4, 4, 17)]  # 150: mid-row; 246: the end
    want_rows = [[0], [0, 2], [0, 2], [0, 3], [1, 5]]
    gp, gg, ga, union = ref.rowwise_lists_ref(params, grad, accs, SPANS, lists, lr=LR, weight_decay=wd, elem=elem)
    assert [u.tolist() for u in union] == want_rows
    keep = np.ones(TOTAL, bool)
    for i, (span, rows) in enumerate(zip(SPANS, want_rows)):
        wp, wg, wa = rw.rowwise_ref(params[i], ref.grad_rows(grad, span), accs[i], rows + rows[:1], span[1],
                                    lr=LR, weight_decay=wd, elem="lib" if elem == "np" else "np")
        assert optim_ref.same_bits(gp[i], wp) and optim_ref.same_bits(ga[i], wa)
        assert optim_ref.same_bits(ref.grad_rows(gg, span), wg) and not ref.grad_rows(gg, span)[rows].any()
        rest = np.setdiff1d(np.arange(span[1]), rows)
        assert np.array_equal(gp[i][rest], params[i][rest]) and np.array_equal(ga[i][rest], accs[i][rest])
        assert not np.array_equal(gp[i][rows], params[i][rows]) and np.all(ga[i][rows] >= accs[i][rows])
        ref.grad_rows(keep, span)[rows] = False
    assert np.array_equal(gg[keep], grad[keep])  # untouched gradient rows and the pads
    keys, index = ref.keys_for(union)
    assert index == [0, 1, 2, 3, 4] and keys.shape == (2, 5)
    assert [sorted(set(keys[:, j].tolist())) for j in range(5)] == want_rows
