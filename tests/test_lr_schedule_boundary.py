"""CPU: the C boundary of the device-resident learning-rate schedules (include/dfwfm_lr_schedule.h) -- its own header
and ABI version in the same libdfwfm.so, the other headers' function lists untouched --, the host evaluation
dfwfm_lr_schedule_eval against exact rational arithmetic (tests/lr_schedule_ref.py) bit for bit, every invalid
argument, and the lr_schedule switch's plumbing (CLI, module, fit's refusal to train at another rate); no compute on the
device without a GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import lr_schedule_ref as ref
from conftest import REPO

LR_API = ["dfwfm_adam_step_dev_sched", "dfwfm_lazy_adam_step_dev_sched", "dfwfm_lr_schedule_abi_version",
          "dfwfm_lr_schedule_eval", "dfwfm_lr_schedule_write"]
LAZY_API = ["dfwfm_lazy_adam_abi_version", "dfwfm_lazy_adam_step_dev"]
FOLD_API = ["dfwfm_bf16_fold_abi_version", "dfwfm_model_fold_bf16"]
FUSED_API = ["dfwfm_bf16_fused_abi_version", "dfwfm_bf16_fused_forward", "dfwfm_bf16_fused_forward_batches",
             "dfwfm_bf16_fused_supported"]
BF16_API = ["dfwfm_bf16_abi_version", "dfwfm_bf16_forward", "dfwfm_bf16_workspace_bytes", "dfwfm_model_pack_bf16"]
F32_FOLD_API = ["dfwfm_fold_abi_version", "dfwfm_model_fold_numerical"]
SERVE_API = ["dfwfm_serve_abi_version", "dfwfm_serve_forward", "dfwfm_serve_workspace_bytes"]
INT8_API = ["dfwfm_int8_abi_version", "dfwfm_int8_forward", "dfwfm_int8_forward_batches", "dfwfm_int8_supported",
            "dfwfm_model_pack_int8"]
HALF_TABLES_API = ["dfwfm_half_tables_abi_version", "dfwfm_model_pack_tables_half", "dfwfm_model_serving_copy_bytes"]
INT8_TABLES_API = ["dfwfm_int8_tables_abi_version", "dfwfm_model_pack_tables_int8"]


@pytest.fixture(scope="module")
def built():
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.build()
    return _lib


def header_functions(name):
    src = open(os.path.join(REPO, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dfwfm_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_exactly_its_five_functions():
    assert header_functions("dfwfm_lr_schedule.h") == LR_API
    src = open(os.path.join(REPO, "include", "dfwfm_lr_schedule.h")).read()
    assert re.search(r"#define\s+DFWFM_LR_SCHEDULE_ABI_VERSION\s+1\b", src)
    assert re.search(r"#define\s+DFWFM_LR_MAX_KNOTS\s+64\b", src)


def test_header_states_the_contract():
    src = " ".join(open(os.path.join(REPO, "include", "dfwfm_lr_schedule.h")).read().replace("*", " ").split())
    for phrase in ("strictly increasing", "fma", "counter + 1", "no recapture", "lane k loads knot k",
                   "the same 64 bits", "0 is allowed"):
        assert phrase in src, phrase


def test_the_other_headers_are_untouched():
    assert header_functions("dfwfm_lazy_adam.h") == LAZY_API
    assert header_functions("dfwfm_bf16_fold.h") == FOLD_API
    assert header_functions("dfwfm_bf16_fused.h") == FUSED_API
    assert header_functions("dfwfm_bf16.h") == BF16_API
    assert header_functions("dfwfm_fold.h") == F32_FOLD_API
    assert header_functions("dfwfm_serve.h") == SERVE_API
    assert header_functions("dfwfm_int8.h") == INT8_API
    assert header_functions("dfwfm_half_tables.h") == HALF_TABLES_API
    assert header_functions("dfwfm_int8_tables.h") == INT8_TABLES_API
    main = header_functions("dfwfm.h")
    assert len(main) == 35 and not any("sched" in f for f in main)
    assert not any("sched" in f for f in header_functions("dfwfm_cpu.h"))


def test_library_exports_the_symbols_and_the_binding_matches(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in LR_API:
        assert hasattr(L, name), name
    assert set(built.LR_SCHEDULE_SIGNATURES) == set(LR_API)
    for other in (built.SIGNATURES, built.SERVE_SIGNATURES, built.BF16_SIGNATURES, built.BF16_FUSED_SIGNATURES,
                  built.FOLD_SIGNATURES, built.BF16_FOLD_SIGNATURES, built.LAZY_ADAM_SIGNATURES, built.INT8_SIGNATURES,
                  built.HALF_TABLES_SIGNATURES, built.INT8_TABLES_SIGNATURES, built.CPU_SIGNATURES,
                  built.INGEST_SIGNATURES):
        assert not set(built.LR_SCHEDULE_SIGNATURES) & set(other)
    assert set(built.SIGNATURES) == set(header_functions("dfwfm.h"))
    assert set(built.LAZY_ADAM_SIGNATURES) == set(LAZY_API)
    assert any(h.endswith("dfwfm_lr_schedule.h") for h in built.HEADERS)  # a changed header rebuilds the library
    # the knot's and the block's layout are the header's
    assert ctypes.sizeof(built.dfwfm_lr_knot) == 16
    assert [f[0] for f in built.dfwfm_lr_knot._fields_] == ["step", "lr"]
    assert built.LR_MAX_KNOTS == 64 and built.LR_SCHEDULE_BYTES == 16 + 64 * 16 and built.LR_SCHEDULE_BYTES % 16 == 0
    # the scheduled steps' argument lists are their twins' with the rate replaced by the block's pointer
    dense, lazy = built.SIGNATURES["dfwfm_adam_step_dev"][1], built.LAZY_ADAM_SIGNATURES["dfwfm_lazy_adam_step_dev"][1]
    assert built.LR_SCHEDULE_SIGNATURES["dfwfm_adam_step_dev_sched"][1] == dense[:2] + [ctypes.c_void_p] + dense[3:]
    assert built.LR_SCHEDULE_SIGNATURES["dfwfm_lazy_adam_step_dev_sched"][1] == \
        lazy[:5] + [ctypes.c_void_p] + lazy[6:]


# ------------------------------------------------------------------------------------------- the host evaluation
def _eval(built, knots, s):
    return built.lr_schedule_eval(knots, s)


def _check(built, knots, steps):
    for s in steps:
        got, want = _eval(built, knots, s), ref.lr_at(knots, s)
        assert ref.bits(got) == ref.bits(want), (knots, s, got, want)


UP = float(np.nextafter(1e-3, 1.0))
CASES = {
    "one knot": ([(5, 1e-3)], [1, 4, 5, 6, 10 ** 12]),
    "warm-up and decay": ([(1, 1e-4), (2000, 1e-3), (200000, 1e-4)],
                          [-3, 0, 1, 2, 3, 7, 999, 1000, 1999, 2000, 2001, 77777, 199999, 200000, 200001, 2 ** 62]),
    "first knot late": ([(10, 3e-4), (17, 1e-3)], [1, 9, 10, 11, 13, 16, 17, 18]),
    "adjacent steps": ([(3, 1e-4), (4, 1e-3), (5, 2e-4), (9, 7e-4)], [2, 3, 4, 5, 6, 7, 8, 9, 10]),
    "descending": ([(1, 1e-2), (1000, 1e-5)], [1, 2, 3, 333, 500, 998, 999, 1000, 1001]),
    "one ulp apart": ([(1, 1e-3), (1001, UP), (2001, 1e-3)], [1, 2, 250, 500, 501, 502, 750, 1000, 1001, 1500, 2000]),
    "zero rate": ([(1, 0.0), (100, 1e-3), (300, 0.0), (400, 0.0)], [1, 2, 50, 99, 100, 101, 200, 299, 300, 350, 400, 401]),
    "near 2^40": ([(2 ** 40 - 5, 1e-3), (2 ** 40 + 3, 1e-4), (2 ** 40 + 2 ** 20 + 1, 5e-4)],
                  [2 ** 40 - 6, 2 ** 40 - 5, 2 ** 40 - 4, 2 ** 40, 2 ** 40 + 2, 2 ** 40 + 3, 2 ** 40 + 4,
                   2 ** 40 + 2 ** 19, 2 ** 40 + 2 ** 20, 2 ** 40 + 2 ** 20 + 1, 2 ** 41]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_eval_equals_the_rational_reference_bit_for_bit(built, name):
    knots, steps = CASES[name]
    _check(built, knots, steps)
    _check(built, knots, [k[0] for k in knots])  # at every knot: exactly that knot's rate
    for (s, lr) in knots:
        assert ref.bits(_eval(built, knots, s)) == ref.bits(lr)


def test_eval_with_64_knots(built):
    r = np.random.default_rng(64)
    steps = np.cumsum(r.integers(1, 50, 64)).tolist()
    knots = list(zip(steps, (10.0 ** r.uniform(-6, -1, 64)).tolist()))
    _check(built, knots, range(0, steps[-1] + 3))


def test_eval_on_random_schedules(built):
    """A few thousand (knots, s) draws from a fixed seed: 1..64 knots, gaps from 1 to 2^33, rates over eight decades
    (some exactly zero), s inside, at and outside the table."""
    r = np.random.default_rng(20240607)
    for _ in range(400):
        n = int(r.integers(1, 65))
        gaps = np.where(r.random(n) < 0.3, 1, (2.0 ** r.uniform(0, 33, n)).astype(np.int64))
        steps = np.cumsum(gaps).tolist()
        lrs = (10.0 ** r.uniform(-9, -1, n)) * (r.random(n) > 0.1)
        knots = list(zip(steps, lrs.tolist()))
        inside = r.integers(steps[0], steps[-1] + 1, 6).tolist()
        picks = r.choice(n, 2).tolist()
        _check(built, knots, inside + [steps[picks[0]], steps[picks[1]] + 1, steps[0] - 1, steps[-1] + 1])


# ------------------------------------------------------------------------------------------- invalid arguments
def _knots(built, pairs):
    return built.lr_knots(pairs)[0]


def _bad_tables():
    nan, inf = float("nan"), float("inf")
    return [([(0, 1e-3)], b"below 1"), ([(-4, 1e-3), (5, 1e-3)], b"below 1"),
            ([(1, 1e-3), (1, 2e-3)], b"strictly increasing"), ([(1, 1e-3), (9, 2e-3), (8, 1e-3)], b"strictly increasing"),
            ([(1, nan)], b"NaN"), ([(1, 1e-3), (2, inf)], b"infinite"), ([(1, 1e-3), (2, -inf)], b"negative"),
            ([(1, -1e-9)], b"negative")]


def test_abi_version_and_invalid_arguments(built):
    """Invalid arguments return DFWFM_ERR_INVALID_ARG (-1) with a message and never abort; no HIP call is reached
    (this process has no device: one would return DFWFM_ERR_HIP)."""
    L = built.lib()
    assert L.dfwfm_lr_schedule_abi_version() == 1
    out = ctypes.c_double(-7.0)
    ok = _knots(built, [(1, 1e-4), (10, 1e-3)])
    block, state, fake = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
    tens = (built.dfwfm_adam_tensor * 1)(built.dfwfm_adam_tensor(0x4000, 0x5000, 0x6000, 0x7000, 8))
    tabs = (built.dfwfm_lazy_adam_table * 1)(built.dfwfm_lazy_adam_table(
        param=0x4000, grad=0x5000, exp_avg=0x6000, exp_avg_sq=0x7000, stamp=0x8000, rows=7, key_range=7, c=0, width=10,
        column=0, kind=0, reserved=0))

    def evaluate(k, n):
        return L.dfwfm_lr_schedule_eval(k, n, 3, ctypes.byref(out))

    def write(k, n):
        return L.dfwfm_lr_schedule_write(block, k, n, None)

    assert evaluate(ok, 2) == 0 and out.value == ref.lr_at([(1, 1e-4), (10, 1e-3)], 3)
    # null pointers
    assert evaluate(None, 2) == -1 and b"null" in L.dfwfm_last_error()
    assert L.dfwfm_lr_schedule_eval(ok, 2, 3, None) == -1 and b"null" in L.dfwfm_last_error()
    assert write(None, 2) == -1 and b"null" in L.dfwfm_last_error()
    assert L.dfwfm_lr_schedule_write(None, ok, 2, None) == -1 and b"null" in L.dfwfm_last_error()
    # the knot count
    big = _knots(built, [(i + 1, 1e-3) for i in range(65)])
    for call in (evaluate, write):
        for k, n in ((ok, 0), (ok, -1), (big, 65)):
            assert call(k, n) == -1 and b"knots" in L.dfwfm_last_error(), (call.__name__, n)
        for pairs, word in _bad_tables():
            assert call(_knots(built, pairs), len(pairs)) == -1, pairs
            assert word in L.dfwfm_last_error(), (pairs, L.dfwfm_last_error())
    assert evaluate(_knots(built, [(1, 0.0)]), 1) == 0 and out.value == 0.0  # a zero rate is allowed
    assert evaluate(big, 64) == 0
    # the scheduled steps: a null block, and every check of their twins
    adam = lambda t, n, sch, st: L.dfwfm_adam_step_dev_sched(t, n, sch, 0.9, 0.999, 1e-8, 3e-7, st, None)  # noqa: E731
    assert adam(tens, 1, None, state) == -1 and b"null schedule" in L.dfwfm_last_error()
    assert adam(tens, 1, block, None) == -1 and b"null" in L.dfwfm_last_error()
    assert adam(None, 1, block, state) == -1 and b"null" in L.dfwfm_last_error()
    assert adam(tens, -1, block, state) == -1 and b"negative" in L.dfwfm_last_error()
    lazy = lambda t, n, xi, stride, batch, sch, st: L.dfwfm_lazy_adam_step_dev_sched(  # noqa: E731
        t, n, xi, stride, batch, sch, 0.9, 0.999, 1e-8, 3e-7, st, None)
    assert lazy(tabs, 1, fake, 1, 4, None, state) == -1 and b"null schedule" in L.dfwfm_last_error()
    assert lazy(tabs, 1, fake, 1, 4, block, None) == -1 and b"null" in L.dfwfm_last_error()
    assert lazy(None, 1, fake, 1, 4, block, state) == -1 and b"null" in L.dfwfm_last_error()
    assert lazy(tabs, 1, None, 1, 4, block, state) == -1 and b"null" in L.dfwfm_last_error()
    assert lazy(tabs, -1, fake, 1, 4, block, state) == -1 and b"negative" in L.dfwfm_last_error()
    assert lazy(tabs, 1, fake, 1, -1, block, state) == -1 and b"negative" in L.dfwfm_last_error()
    tabs[0].width = 0
    assert lazy(tabs, 1, fake, 1, 4, block, state) == -1 and b"width" in L.dfwfm_last_error()
    tabs[0].width, tabs[0].key_range = 10, 8
    assert lazy(tabs, 1, fake, 1, 4, block, state) == -1 and b"reaches" in L.dfwfm_last_error()


# --------------------------------------------------------------------------------------------------- the switch
def _sizes():
    return [1] * 13 + [7] * 26


def test_cli_spec_parses_and_reaches_the_module():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    assert p.parse_args([]).lr_schedule is None
    want = [(1, 1e-4), (2000, 1e-3), (200000, 1e-4)]
    assert p.parse_args(["-lr_schedule", "1:1e-4,2000:1e-3,200000:1e-4"]).lr_schedule == want
    assert p.parse_args(["-lr_schedule", "7:0"]).lr_schedule == [(7, 0.0)]
    m = get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args(["-lr_schedule", "1:1e-4,2000:1e-3"]))
    assert m.lr_schedule == [(1, 1e-4), (2000, 1e-3)]
    assert "lr_schedule" not in "".join(m.state_dict())  # a training switch, not state
    assert get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args([])).lr_schedule is None
    assert DeepFMs(field_size=39, feature_sizes=_sizes(), numerical=13, use_cuda=False).lr_schedule is None


@pytest.mark.parametrize("spec", ["", "1", "1:", ":1e-3", "a:1e-3", "1.5:1e-3", "1:x", "1:1e-3,", "1:1e-3;2:1e-3",
                                  "0:1e-3", "2:1e-3,2:1e-4", "5:1e-3,3:1e-4", "1:-1e-3", "1:nan", "1:inf", "1:2:3",
                                  ",".join(f"{i + 1}:1e-3" for i in range(65))])
def test_malformed_cli_spec_is_an_argparse_error(spec, capsys):
    from xsdeepfwfm_deprecated_amd.cli import get_parser
    with pytest.raises(SystemExit) as e:
        get_parser().parse_args(["-lr_schedule", spec])
    assert e.value.code == 2
    assert "lr_schedule" in capsys.readouterr().err


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_fit_refuses_the_schedule_off_the_fused_step(opt):
    """A module on the CPU (torch.optim.Adam through autograd), or any optimizer but Adam: fit() raises before the
    first batch instead of training at the fixed learning_rate."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = _sizes()
    xi, xv = synth.synth_inputs(sizes, 13, 64, seed=2)
    y = (np.arange(64) % 2).astype(np.float32)
    m = DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1,
                h_depth=1, deep_nodes=16, n_epochs=1, batch_size=32, optimizer_type=opt, use_cuda=False)
    m.lr_schedule = [(1, 1e-4), (3, 1e-3)]
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(ValueError, match="lr_schedule"):
        m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    m.lr_schedule = None  # the same call trains without the switch
    m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    assert any(not torch.equal(before[k], v) for k, v in m.state_dict().items())


def test_fused_step_signature_has_the_schedule_off_by_default():
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    assert inspect.signature(FusedTrainStep.__init__).parameters["lr_schedule"].default is None
    for name in ("set_lr", "set_lr_schedule", "lr_at"):
        assert callable(getattr(FusedTrainStep, name))


# ------------------------------------------------------------------------------------- the reference helper itself
def test_reference_rounds_where_the_contract_rounds():
    """Midpoints and exact cases whose value is known without it; and one case where a product rounded on its own
    (no fma) would give another double, so that the reference is seen to fuse."""
    assert ref.lr_at([(1, 1.0), (3, 2.0)], 2) == 1.5
    assert ref.lr_at([(1, 1.0), (5, 0.0)], 4) == 0.25
    assert ref.lr_at([(2, 1e-3)], -5) == 1e-3 and ref.lr_at([(2, 1e-3)], 2 ** 50) == 1e-3
    assert ref.bits(ref.lr_at([(1, 0.0), (9, 0.0)], 4)) == ref.bits(0.0)
    r = np.random.default_rng(3)
    split = 0
    for _ in range(2000):
        a, b = (10.0 ** r.uniform(-6, -1, 2)).tolist()
        n = int(r.integers(3, 5000))
        s = int(r.integers(2, n))
        t = (s - 1) / (n - 1)
        split += ref.lr_at([(1, a), (n, b)], s) != (b - a) * t + a  # Python rounds the product, then the sum
    assert 0 < split < 2000
