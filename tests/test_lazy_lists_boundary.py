"""CPU: the C boundary of the list-driven row-lazy steps (include/dfwfm_lazy_lists.h) -- its own header and ABI version
in the same libdfwfm.so, the other headers' function lists untouched --, every invalid argument (fake non-null
pointers: nothing is dereferenced, no launch is reached), the lazy_exchange switch's plumbing (CLI, module, the fused
step's keyword) and the reference helper's own bookkeeping (tests/lazy_lists_ref.py); no compute on the device without
a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import lazy_lists_ref as ref
import optim_ref
from conftest import REPO

LAZY_LISTS_API = ["dfwfm_lazy_adam_lists_step_dev", "dfwfm_lazy_adam_lists_step_dev_sched",
                  "dfwfm_lazy_lists_abi_version", "dfwfm_lazy_optim_lists_step_dev",
                  "dfwfm_lazy_optim_lists_step_dev_sched"]
LAZY_OPTIM_API = ["dfwfm_lazy_optim_abi_version", "dfwfm_lazy_optim_step_dev", "dfwfm_lazy_optim_step_dev_sched"]
LAZY_ADAM_API = ["dfwfm_lazy_adam_abi_version", "dfwfm_lazy_adam_step_dev"]
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


def test_header_declares_exactly_its_five_functions_and_states_the_contract():
    assert header_functions("dfwfm_lazy_lists.h") == LAZY_LISTS_API
    raw = open(os.path.join(REPO, "include", "dfwfm_lazy_lists.h")).read()
    assert re.search(r"#define\s+DFWFM_LAZY_LISTS_ABI_VERSION\s+1\b", raw)
    assert "dfwfm_lazy_lists_span" in raw and "dfwfm_lazy_lists_list" in raw
    src = " ".join(raw.replace("*", " ").split())
    for phrase in ("touched", "at least one list names its destination", "the same bits", "GLOBAL step",
                   "weight decay acts on touched rows only", "zeroed gradient", "updated once", "2^32",
                   "device-scope look", "atomic exchange", "STILL advances", "is skipped", "no address is formed",
                   "HIP graph", "64) spans", "32) lists", "several launches", "min( count, cap)",
                   "bit-identical from run to run", "dfwfm_lr_schedule_eval(s)", "may be NULL",
                   "null opt_state where the optimizer needs one", "overlaps", "matches no span", "cap < 0",
                   "No call aborts"):
        assert phrase in src, phrase


def test_the_other_headers_are_untouched():
    assert header_functions("dfwfm_optim.h") == OPTIM_API
    assert header_functions("dfwfm_lazy_adam.h") == LAZY_ADAM_API
    assert header_functions("dfwfm_lazy_optim.h") == LAZY_OPTIM_API
    main = header_functions("dfwfm.h")
    assert len(main) == 35 and not any("lazy" in f or "optim" in f for f in main)
    for name in sorted(os.listdir(os.path.join(REPO, "include"))):
        if name != "dfwfm_lazy_lists.h":
            assert "lazy_lists" not in open(os.path.join(REPO, "include", name)).read(), name
    for name, macro in (("dfwfm_lazy_adam.h", "DFWFM_LAZY_ADAM_ABI_VERSION"),
                        ("dfwfm_lazy_optim.h", "DFWFM_LAZY_OPTIM_ABI_VERSION"),
                        ("dfwfm_optim.h", "DFWFM_OPTIM_ABI_VERSION")):
        assert re.search(r"#define\s+%s\s+1\b" % macro, open(os.path.join(REPO, "include", name)).read()), name


def test_library_exports_the_symbols_and_the_binding_matches(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in LAZY_LISTS_API:
        assert hasattr(L, name), name
    assert set(built.LAZY_LISTS_SIGNATURES) == set(header_functions("dfwfm_lazy_lists.h"))
    for other in (built.SIGNATURES, built.SERVE_SIGNATURES, built.BF16_SIGNATURES, built.BF16_FUSED_SIGNATURES,
                  built.FOLD_SIGNATURES, built.BF16_FOLD_SIGNATURES, built.CPU_SIGNATURES, built.INGEST_SIGNATURES,
                  built.LAZY_ADAM_SIGNATURES, built.LR_SCHEDULE_SIGNATURES, built.OPTIM_SIGNATURES,
                  built.INT8_SIGNATURES, built.HALF_TABLES_SIGNATURES, built.INT8_TABLES_SIGNATURES,
                  built.LAZY_OPTIM_SIGNATURES):
        assert not set(built.LAZY_LISTS_SIGNATURES) & set(other)
    assert any(h.endswith(os.path.join("include", "dfwfm_lazy_lists.h")) for h in built.HEADERS)
    assert "dfwfm_lazy_lists.h" in built.HEADERS and "dfwfm_lazy_lists.hip" in built.SOURCES
    assert built.lib().dfwfm_lazy_lists_abi_version() == 1
    # the descriptors' layouts are the header's
    assert ctypes.sizeof(built.dfwfm_lazy_lists_span) == 2 * 8 + 2 * 8 + 2 * 4
    assert [f[0] for f in built.dfwfm_lazy_lists_span._fields_] == ["param", "stamp", "offset", "rows", "width",
                                                                      "reserved"]
    assert ctypes.sizeof(built.dfwfm_lazy_lists_list) == 2 * 8 + 8 + 2 * 4
    assert [f[0] for f in built.dfwfm_lazy_lists_list._fields_] == ["dest", "count", "cap", "width", "reserved"]
    raw = open(os.path.join(REPO, "include", "dfwfm_lazy_lists.h")).read()
    for field in ("param", "stamp", "offset", "rows", "width", "dest", "count", "cap"):
        assert re.search(r"\b%s;" % field, raw), field


# ------------------------------------------------------------------------------------------- invalid arguments
def _spans(built, *descs):
    """Span descriptors with fake non-null pointers: an invalid one is refused before anything is dereferenced."""
    arr = (built.dfwfm_lazy_lists_span * max(len(descs), 1))()
    for i, kw in enumerate(descs):
        d = dict(param=0x1000 + 0x100 * i, stamp=0x5000 + 0x100 * i, offset=80 * i, rows=7, width=10, reserved=0)
        d.update(kw)
        arr[i] = built.dfwfm_lazy_lists_span(**d)
    return arr, len(descs)


def _lists(built, *descs):
    arr = (built.dfwfm_lazy_lists_list * max(len(descs), 1))()
    for i, kw in enumerate(descs):
        d = dict(dest=0x9000, count=0xa000, cap=16, width=10, reserved=0)
        d.update(kw)
        arr[i] = built.dfwfm_lazy_lists_list(**d)
    return arr, len(descs)


def test_abi_version_and_invalid_arguments(built):
    """Invalid arguments return DFWFM_ERR_INVALID_ARG (-1) with a message and never abort; no HIP call is reached (this
    process has no device: a launch would return DFWFM_ERR_HIP)."""
    L = built.lib()
    P = ctypes.c_void_p
    assert L.dfwfm_lazy_lists_abi_version() == 1
    nan, inf = float("nan"), float("inf")
    good = optim_ref.hyper("rmsp", LR, 3e-7)
    ok_s, ok_l = _spans(built, {}), _lists(built, {})

    def calls(sp=ok_s, ls=ok_l, grad=0x2000, m=0x3000, v=0x4000, state=0x7000, h=good, block=0x8000,
              null_spans=False, null_lists=False):
        (sa, ns), (la, nl) = sp, ls
        sa, la = (None if null_spans else sa), (None if null_lists else la)
        g, mm, vv = (P(x) if x else None for x in (grad, m, v))
        st, bl = (P(state) if state else None), (P(block) if block else None)
        hp = None if h is None else ctypes.byref(h)
        return [("adam", lambda: L.dfwfm_lazy_adam_lists_step_dev(sa, ns, la, nl, g, mm, vv, LR, 0.9, 0.999, 1e-8,
                                                                   0.0, st, None)),
                ("adam_sched", lambda: L.dfwfm_lazy_adam_lists_step_dev_sched(sa, ns, la, nl, g, mm, vv, bl, 0.9,
                                                                               0.999, 1e-8, 0.0, st, None)),
                ("optim", lambda: L.dfwfm_lazy_optim_lists_step_dev(sa, ns, la, nl, g, mm, hp, st, None)),
                ("optim_sched", lambda: L.dfwfm_lazy_optim_lists_step_dev_sched(sa, ns, la, nl, g, mm, hp, bl, st,
                                                                                 None))]

    def refused(word, only=None, **kw):
        for name, call in calls(**kw):
            if only is None or name in only:
                assert call() == -1, (name, word)
                assert word in L.dfwfm_last_error(), (name, word, L.dfwfm_last_error())

    refused(b"null state block", state=0)
    refused(b"null schedule", block=0, only=("adam_sched", "optim_sched"))
    refused(b"null grad", grad=0)
    refused(b"null exp_avg", m=0, only=("adam", "adam_sched"))
    refused(b"null exp_avg", v=0, only=("adam", "adam_sched"))
    refused(b"null span array", null_spans=True)
    refused(b"null list array", null_lists=True)
    refused(b"negative span count", sp=(ok_s[0], -1))
    refused(b"negative list count", ls=(ok_l[0], -1))
    refused(b"null hyper", h=None, only=("optim", "optim_sched"))
    # a null state array where the kind needs one; plain SGD needs none (and is then refused for something else)
    for kind, mom in (("adag", 0.0), ("rmsp", 0.0), ("sgd", 0.9)):
        refused(b"null state array", m=0, h=optim_ref.hyper(kind, LR, 0.0, mom), only=("optim", "optim_sched"))
    refused(b"cap < 0", m=0, h=optim_ref.hyper("sgd", LR), ls=_lists(built, dict(cap=-1)), only=("optim", "optim_sched"))
    # spans
    for bad, word in ((dict(param=None), b"null pointer"), (dict(stamp=None), b"null pointer"),
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
    refused(b"cap < 0", sp=_spans(built, {}, dict(offset=80, width=1)), ls=_lists(built, dict(width=1), dict(cap=-1)))
    # the hyper-parameters: dfwfm_optim_step_dev's checks
    for kind in (-1, 3, 77):
        refused(b"unknown optimizer kind", h=optim_ref.hyper(kind, LR), only=("optim", "optim_sched"))
    for field in ("lr", "weight_decay", "momentum", "alpha", "eps"):
        for bad, word in ((nan, b"NaN"), (inf, b"infinite"), (-inf, b"negative"), (-1e-9, b"negative")):
            h = optim_ref.hyper("rmsp", LR, 1e-2, 0.9)
            setattr(h, field, bad)
            # (a scheduled call does not read lr)
            refused(field.encode(), h=h, only=("optim",) if field == "lr" else ("optim", "optim_sched"))
            assert word in L.dfwfm_last_error()
    h = optim_ref.hyper("rmsp", LR)
    h.alpha = 1.0
    refused(b"alpha", h=h, only=("optim", "optim_sched"))


# --------------------------------------------------------------------------------------------------- the switch
def _sizes():
    return [1] * 13 + [7] * 26


def test_cli_flag_parses_and_reaches_the_module():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    assert p.parse_args([]).lazy_exchange == 0
    assert p.parse_args(["-lazy_exchange", "1"]).lazy_exchange == 1
    with pytest.raises(SystemExit):
        p.parse_args(["-lazy_exchange", "2"])
    for flag in (0, 1):
        m = get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args(["-lazy_exchange", str(flag)]))
        assert m.lazy_exchange is bool(flag) and m.lazy_tables is False and m.lazy_table_adam is False
        assert "lazy" not in "".join(m.state_dict())  # a training switch, not state
    assert get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args([])).lazy_exchange is False
    assert DeepFMs(field_size=39, feature_sizes=_sizes(), numerical=13, use_cuda=False).lazy_exchange is False


def test_fit_refuses_the_switch_off_the_fused_step():
    """A module on the CPU (autograd + torch.optim): fit() raises before the first batch instead of training through
    another path."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = _sizes()
    xi, xv = synth.synth_inputs(sizes, 13, 64, seed=2)
    y = (np.arange(64) % 2).astype(np.float32)
    m = DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1,
                h_depth=1, deep_nodes=16, n_epochs=1, batch_size=32, optimizer_type="adam", use_cuda=False)
    m.lazy_exchange = True
    with pytest.raises(ValueError, match="lazy_exchange"):
        m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])


def test_fused_step_signature_has_the_switch_off_by_default():
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    pars = inspect.signature(FusedTrainStep.__init__).parameters
    assert pars["lazy_exchange"].default is False
    assert pars["lazy_tables"].default is False and pars["lazy_table_adam"].default is False
    assert pars["sparse_exchange"].default is True


# ------------------------------------------------------------------------------------- the reference helper itself
SPANS = [(0, 1, 10), (12, 7, 10), (84, 7, 1), (92, 5, 10)]


def test_reference_union_of_destinations_per_span():
    """Destinations map to rows per span of the list's width; the count is clamped to [0, cap]; a destination between
    two rows, in a span of another width, in a pad or past the end is skipped."""
    lists = [(np.array([0, 12, 72, 92, 999], np.int64), 4, 5, 10),    # the 5th entry lies behind the count
             (np.array([72, 22, 17, 84, 142], np.int64), 9, 5, 10),   # count > cap; 17: mid-row; 84: width-1 span; 142: end
             (np.array([84, 90, 91, 12], np.int64), 4, 4, 1),         # 91: the pad; 12: a width-10 span
             (np.array([85], np.int64), -3, 1, 1),                    # a negative count reads nothing
             (np.array([132], np.int64), 1, 1, 10)]
    rows = ref.union_rows(SPANS, lists)
    assert [r.tolist() for r in rows] == [[0], [0, 1, 6], [0, 6], [0, 4]]
    assert [r.tolist() for r in ref.union_rows(SPANS, [])] == [[], [], [], []]


@pytest.mark.parametrize("opt,mom", [("adam", 0.0), ("sgd", 0.0), ("sgd", 0.9), ("adag", 0.0), ("rmsp", 0.0)],
                         ids=["adam", "sgd", "sgd-momentum", "adag", "rmsp"])
def test_reference_updates_the_union_rows_once_and_nothing_else(built, opt, mom):
    """Two lists that share rows: the result is the key-driven reference's on each span's union rows (a shared row
    updated once), the other rows keep every bit, touched gradient rows are zero."""
    import lazy_adam_ref
    import lazy_optim_ref
    r = np.random.default_rng(5)
    total = 144
    params = [r.standard_normal((rows, w)).astype(np.float32) for _, rows, w in SPANS]
    grad = r.standard_normal(total).astype(np.float32)
    m = (0.1 * r.standard_normal(total)).astype(np.float32)
    v = (0.01 * r.random(total)).astype(np.float32)
    lists = [(np.array([12, 32, 92], np.int64), 3, 4, 10), (np.array([32, 122, 0], np.int64), 3, 3, 10),
             (np.array([86, 84], np.int64), 2, 2, 1), (np.array([86], np.int64), 1, 2, 1)]
    want_rows = [[0], [0, 2], [0, 2], [0, 3]]
    assert [x.tolist() for x in ref.union_rows(SPANS, lists)] == want_rows
    if opt == "adam":
        gp, gg, gm, gv = ref.lazy_adam_lists_ref(params, grad, m, v, SPANS, lists, 3, lr=LR, weight_decay=3e-7)
    else:
        m = np.abs(m)  # a sum / square_avg is never negative
        st = m if optim_ref.has_state(opt, mom) else None
        gp, gg, gm = ref.lazy_optim_lists_ref(opt, params, grad, st, SPANS, lists, 3, lr=LR, weight_decay=3e-7,
                                              momentum=mom)
        assert (gm is None) == (st is None)
    for i, ((off, rows, w), touched) in enumerate(zip(SPANS, want_rows)):
        sl = slice(off, off + rows * w)
        view = lambda a: a[sl].reshape(rows, w)  # noqa: E731
        if opt == "adam":
            wp, wg, wm, wv = lazy_adam_ref.lazy_adam_ref(params[i], view(grad), view(m), view(v), touched, rows, 3,
                                                         lr=LR, weight_decay=3e-7)
            assert np.array_equal(view(gv), wv)
        else:
            wp, wg, wm = lazy_optim_ref.lazy_optim_ref(opt, params[i], view(grad), None if gm is None else view(m),
                                                       touched, rows, 3, lr=LR, weight_decay=3e-7, momentum=mom)
        assert np.array_equal(gp[i], wp) and np.array_equal(view(gg), wg)
        if gm is not None:
            assert np.array_equal(view(gm), wm)
        rest = np.setdiff1d(np.arange(rows), touched)
        assert np.array_equal(gp[i][rest], params[i][rest]) and np.array_equal(view(gg)[rest], view(grad)[rest])
        assert not view(gg)[touched].any() and not np.array_equal(gp[i][touched], params[i][touched])
    pads = np.r_[10:12, 82:84, 91:92, 142:144]
    assert np.array_equal(gg[pads], grad[pads])  # the pads between the spans are nobody's
