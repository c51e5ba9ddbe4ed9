"""CPU: the C boundary of the SGD / Adagrad / RMSprop steps (include/dfwfm_optim.h) -- its own header and ABI version
in the same libdfwfm.so --, the host function dfwfm_optim_elem_ref against the numpy restatement of the header's forms
(tests/optim_ref.py) bit for bit and against torch.optim.{SGD, Adagrad, RMSprop} on the CPU, every invalid argument, and
the fused_optimizer switch's plumbing (CLI, module, fit's refusal to train through another path); no compute on the
device without a GPU.

Against torch.optim 2.10 (foreach=False, the reference's arguments; n in {3, 8, 16, 37, 1031}, wd in {0, 6e-7, 1e-2},
four steps, the state carried by the library function): SGD's parameters and momentum buffer, Adagrad's sum and
RMSprop's square_avg are bit-identical in every case; Adagrad's and RMSprop's parameters differ in at most 3 of 1031
elements (ATen's vector path forms the quotient another way), within rtol 2.4e-7, atol 2e-9."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as ref
from conftest import REPO

OPTIM_API = ["dfwfm_optim_abi_version", "dfwfm_optim_elem_ref", "dfwfm_optim_step", "dfwfm_optim_step_dev",
             "dfwfm_optim_step_dev_sched"]
NS = [3, 8, 16, 37, 1031]
WDS = [0.0, 6e-7, 1e-2]
LR = 1e-3
# kind, momentum
VARIANTS = [("sgd", 0.0), ("sgd", 0.9), ("adag", 0.0), ("rmsp", 0.0)]


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
    assert header_functions("dfwfm_optim.h") == OPTIM_API
    raw = open(os.path.join(REPO, "include", "dfwfm_optim.h")).read()
    assert re.search(r"#define\s+DFWFM_OPTIM_ABI_VERSION\s+1\b", raw)
    for name in ("DFWFM_OPTIM_SGD", "DFWFM_OPTIM_ADAGRAD", "DFWFM_OPTIM_RMSPROP"):
        assert name in raw
    src = " ".join(raw.replace("*", " ").split())  # (the comment's leading stars, and its products' ones, are blanks)
    for phrase in ("fmaf(wd, p, g)", "fmaf(d, -lr, p)", "fmaf(g', g', sum)", "round((1 - alpha) g')",
                   "round(sq alpha)", "counter + 1", "the same 32 bits", "dfwfm_lr_schedule_eval(s)", "at step 1"):
        assert phrase in src, phrase
    assert "dfwfm_optim" not in open(os.path.join(REPO, "include", "dfwfm.h")).read()


def test_library_exports_the_symbols_and_the_binding_matches(built):
    L = ctypes.CDLL(built.LIB_PATH)
    for name in OPTIM_API:
        assert hasattr(L, name), name
    assert set(built.OPTIM_SIGNATURES) == set(OPTIM_API)
    for other in (built.SIGNATURES, built.LAZY_ADAM_SIGNATURES, built.LR_SCHEDULE_SIGNATURES):
        assert not set(built.OPTIM_SIGNATURES) & set(other)
    assert any(h.endswith(os.path.join("include", "dfwfm_optim.h")) for h in built.HEADERS)
    assert "dfwfm_optim.h" in built.HEADERS and "dfwfm_optim.hip" in built.SOURCES
    assert built.lib().dfwfm_optim_abi_version() == 1
    # the structs' layouts are the header's: a 32-byte tensor entry, the hyper-parameters' doubles behind the kind
    assert ctypes.sizeof(built.dfwfm_optim_tensor) == 32
    assert [f[0] for f in built.dfwfm_optim_tensor._fields_] == ["param", "grad", "state", "numel"]
    assert ctypes.sizeof(built.dfwfm_optim_hyper) == 48 and built.dfwfm_optim_hyper.lr.offset == 8
    assert [f[0] for f in built.dfwfm_optim_hyper._fields_] == ["kind", "reserved", "lr", "weight_decay", "momentum",
                                                               "alpha", "eps"]
    assert (built.OPTIM_SGD, built.OPTIM_ADAGRAD, built.OPTIM_RMSPROP) == (0, 1, 2)
    assert {k: v[0] for k, v in built.OPTIM_KINDS.items()} == ref.KINDS
    assert {k: v[1] for k, v in built.OPTIM_KINDS.items()} == ref.DEFAULT_EPS


# ------------------------------------------------------------------------------------------- the host function
def _draw(n, seed):
    r = np.random.default_rng(seed)
    p0 = (0.1 * r.standard_normal(n)).astype(np.float32)
    gs = [(0.01 * r.standard_normal(n)).astype(np.float32) for _ in range(4)]
    return p0, gs


@pytest.fixture(scope="module")
def lib_runs(built):
    """Four steps of every (variant, n, wd) through dfwfm_optim_elem_ref, the state carried: computed once, shared by
    the numpy and the torch comparison, never written.  {(kind, momentum, n, wd): [(p, s) after each step]}"""
    runs = {}
    for kind, mom in VARIANTS:
        for n in NS:
            for wd in WDS:
                p, gs = _draw(n, 1000 + n)
                s = np.zeros(n, np.float32) if ref.has_state(kind, mom) else None
                h = ref.hyper(kind, LR, wd, mom)
                out = []
                for k, g in enumerate(gs, 1):
                    p, s = ref.lib_step(h, k, p, g, s)
                    out.append((p.copy(), None if s is None else s.copy()))
                runs[(kind, mom, n, wd)] = out
    return runs


@pytest.mark.parametrize("kind,mom", VARIANTS)
def test_elem_ref_equals_the_numpy_restatement_bit_for_bit(lib_runs, kind, mom):
    for n in NS:
        for wd in WDS:
            p, gs = _draw(n, 1000 + n)
            s = np.zeros(n, np.float32) if ref.has_state(kind, mom) else None
            for k, g in enumerate(gs, 1):
                p, s = ref.np_step(kind, k, p, g, s, lr=LR, wd=wd, momentum=mom)
                lp, ls = lib_runs[(kind, mom, n, wd)][k - 1]
                assert np.array_equal(ref.bits(p), ref.bits(lp)), (kind, mom, n, wd, k, "p")
                assert (s is None) == (ls is None)
                if s is not None:
                    assert np.array_equal(ref.bits(s), ref.bits(ls)), (kind, mom, n, wd, k, "state")
    assert not np.array_equal(lib_runs[(kind, mom, 37, 0.0)][0][0], lib_runs[(kind, mom, 37, 0.0)][3][0])


def test_elem_ref_equals_the_numpy_restatement_on_special_values(built):
    """Zeros of both signs, subnormals, gradients whose square underflows or overflows, huge and tiny parameters, at
    steps 1 and 2, with and without weight decay: finite or not, the same bits (a NaN equals a NaN)."""
    vals = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, 1e-30, -1e-30, 1e-20, 3e-5, -0.37, 1.0, 7.5, 1e10, -1e19, 1e20,
                     3e38, -3e38, np.inf, -np.inf, np.nan], np.float32)
    g, p = (a.reshape(-1) for a in np.meshgrid(vals, vals[:17]))
    r = np.random.default_rng(5)
    for kind, mom in VARIANTS:
        for wd in (0.0, 1e-2):
            for step in (1, 2):
                s = np.abs(r.standard_normal(p.size)).astype(np.float32) * (step > 1) if ref.has_state(kind, mom) else None
                if kind == "sgd" and s is not None:
                    s = s * np.where(r.random(p.size) < 0.5, -1, 1).astype(np.float32)
                np_p, np_s = ref.np_step(kind, step, p, g, s, lr=LR, wd=wd, momentum=mom)
                lp, ls = ref.lib_step(ref.hyper(kind, LR, wd, mom), step, p, g, s)
                assert ref.same_bits(np_p, lp), (kind, mom, wd, step, "p")
                if s is not None:
                    assert ref.same_bits(np_s, ls), (kind, mom, wd, step, "state")


def test_momentum_sgd_copies_the_gradient_at_step_one_and_keeps_a_negative_zero(built):
    h = ref.hyper("sgd", LR, 0.0, 0.9)
    p, s = ref.elem_ref(h, 1, -0.0, -0.0, 123.0)  # the buffer's old contents are not read at step 1
    assert ref.bits(s) == ref.bits(np.float32(-0.0))     # a copy: g * 1 + 0 would have been +0 ...
    assert ref.bits(p) == ref.bits(np.float32(0.0))      # ... and p = fmaf(-0, -lr, -0) = +0 + -0 = +0, as torch's
    p, s = ref.elem_ref(h, 2, 1.0, -0.0, -0.0)    # step 2: (-0 * 0.9) + -0 = -0
    assert ref.bits(s) == ref.bits(np.float32(-0.0)) and p == np.float32(1.0)
    p, s = ref.elem_ref(h, 2, 1.0, 0.25, 0.5)
    assert s == np.float32(np.float32(0.5) * np.float32(0.9)) + np.float32(0.25)
    p1, s1 = ref.elem_ref(h, 1, 1.0, 0.25, 0.5)
    assert s1 == np.float32(0.25) and p1 != p


@pytest.mark.parametrize("kind,mom", VARIANTS)
def test_elem_ref_against_torch_optim_on_the_cpu(lib_runs, kind, mom):
    """torch.optim's single-tensor step, built as the reference builds it.  The state and SGD's parameters bit for bit;
    Adagrad's and RMSprop's parameters within the project's bar for Adam against torch (rtol 2.4e-7, atol 2e-9), at most
    1 % of the elements differing at all: counted over all elements the kind compares, and per tensor where a tensor
    has the hundred elements that make 1 % of it a count (n = 1031: at most 10; the header's forms themselves, in
    numpy, differ from torch in up to 3 of those and in 1 of 16 at n = 16, so no count per 3- to 37-element tensor
    could be held).  Each step starts from the library's own previous parameters and state (put
    into torch's tensors), so one step's rounding difference does not feed the next comparison."""
    worst = total = differing = 0
    for n in NS:
        for wd in WDS:
            p0, gs = _draw(n, 1000 + n)
            t = torch.tensor(p0.copy(), requires_grad=True)
            opt = ref.torch_optimizer(kind, [t], LR, wd, mom)
            for k, g in enumerate(gs, 1):
                t.grad = torch.tensor(g.copy())
                opt.step()
                lp, ls = lib_runs[(kind, mom, n, wd)][k - 1]
                tp = t.detach().numpy()
                if ls is not None:
                    ts = opt.state[t][ref.TORCH_STATE[kind]].numpy()
                    assert np.array_equal(ref.bits(ts), ref.bits(ls)), (kind, mom, n, wd, k, "state")
                if kind == "sgd":
                    assert np.array_equal(ref.bits(tp), ref.bits(lp)), (kind, mom, n, wd, k, "p")
                else:
                    differ = int((ref.bits(tp) != ref.bits(lp)).sum())
                    worst = max(worst, differ)
                    total, differing = total + n, differing + differ
                    assert n < 100 or differ <= 0.01 * n, (kind, n, wd, k, differ)
                    assert np.all(np.abs(tp - lp) <= 2.4e-7 * np.abs(tp) + 2e-9), (kind, n, wd, k)
                    with torch.no_grad():
                        t.copy_(torch.from_numpy(lp))  # the next step from the library's parameters
    print(f"{kind} momentum {mom}: at most {worst} elements of a tensor differ from torch, {differing} of {total}")
    assert differing <= 0.01 * total, (kind, differing, total)


# ------------------------------------------------------------------------------------------- invalid arguments
def test_abi_version_and_invalid_arguments(built):
    """Invalid arguments return DFWFM_ERR_INVALID_ARG (-1) with a message and never abort; no HIP call is reached
    (this process has no device: a launch would return DFWFM_ERR_HIP)."""
    L = built.lib()
    assert L.dfwfm_optim_abi_version() == 1
    nan, inf = float("nan"), float("inf")
    state, block = ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)

    def tens(param=0x4000, grad=0x5000, st=0x6000, n=8):
        return (built.dfwfm_optim_tensor * 1)(built.dfwfm_optim_tensor(param, grad, st, n))

    def calls(t, n, h):
        hp = None if h is None else ctypes.byref(h)
        return [("step", lambda: L.dfwfm_optim_step(t, n, hp, 3, None)),
                ("step_dev", lambda: L.dfwfm_optim_step_dev(t, n, hp, state, None)),
                ("step_dev_sched", lambda: L.dfwfm_optim_step_dev_sched(t, n, hp, block, state, None))]

    def refused(t, n, h, word, only=None):
        for name, call in calls(t, n, h):
            if only is None or name in only:
                assert call() == -1, (name, word)
                assert word in L.dfwfm_last_error(), (name, word, L.dfwfm_last_error())

    ok = ref.hyper("rmsp", LR, 1e-2)
    refused(tens(), 1, None, b"null hyper")
    refused(None, 1, ok, b"null tensor array")
    refused(tens(), -1, ok, b"negative tensor count")
    refused(tens(param=None), 1, ok, b"null param")
    for kind, mom in (("adag", 0.0), ("rmsp", 0.0), ("sgd", 0.9)):
        refused(tens(st=None), 1, ref.hyper(kind, LR, 0.0, mom), b"null state pointer")
    for kind in (-1, 3, 77):
        refused(tens(), 1, ref.hyper(kind, LR), b"unknown optimizer kind")
    for field in ("lr", "weight_decay", "momentum", "alpha", "eps"):
        for bad, word in ((nan, b"NaN"), (inf, b"infinite"), (-inf, b"negative"), (-1e-9, b"negative")):
            for kind in ("sgd", "adag", "rmsp"):
                h = ref.hyper(kind, LR, 1e-2, 0.9)
                setattr(h, field, bad)
                # (a scheduled call does not read lr)
                refused(tens(), 1, h, field.encode(), only=("step", "step_dev") if field == "lr" else None)
                assert word in L.dfwfm_last_error()
    for alpha in (1.0, 1.5):
        h = ref.hyper("rmsp", LR)
        h.alpha = alpha
        refused(tens(), 1, h, b"alpha")
    assert L.dfwfm_optim_step_dev(tens(), 1, ctypes.byref(ok), None, None) == -1 and b"null state block" in \
        L.dfwfm_last_error()
    assert L.dfwfm_optim_step_dev_sched(tens(), 1, ctypes.byref(ok), block, None, None) == -1 and \
        b"null state block" in L.dfwfm_last_error()
    assert L.dfwfm_optim_step_dev_sched(tens(), 1, ctypes.byref(ok), None, state, None) == -1 and \
        b"null schedule" in L.dfwfm_last_error()
    for step in (0, -5):
        assert L.dfwfm_optim_step(tens(), 1, ctypes.byref(ok), step, None) == -1 and b"below 1" in L.dfwfm_last_error()
    # the host function
    p, s = ctypes.c_float(1.0), ctypes.c_float(0.0)
    g = ctypes.c_float(0.5)
    elem = L.dfwfm_optim_elem_ref
    assert elem(None, 1, ctypes.byref(p), g, ctypes.byref(s)) == -1 and b"null hyper" in L.dfwfm_last_error()
    assert elem(ctypes.byref(ok), 1, None, g, ctypes.byref(s)) == -1 and b"null param" in L.dfwfm_last_error()
    assert elem(ctypes.byref(ok), 1, ctypes.byref(p), g, None) == -1 and b"null state" in L.dfwfm_last_error()
    assert elem(ctypes.byref(ok), 0, ctypes.byref(p), g, ctypes.byref(s)) == -1 and b"below 1" in L.dfwfm_last_error()
    assert elem(ctypes.byref(ref.hyper(9, LR)), 1, ctypes.byref(p), g, ctypes.byref(s)) == -1
    assert p.value == 1.0 and s.value == 0.0  # a refused call writes nothing
    # plain SGD needs no state; zero hyper-parameters are allowed
    assert elem(ctypes.byref(ref.hyper("sgd", 0.0)), 1, ctypes.byref(p), g, None) == 0 and p.value == 1.0
    assert elem(ctypes.byref(ref.hyper("sgd", 0.5)), 1, ctypes.byref(p), g, None) == 0 and p.value == 0.75
    # a stepless list on the host-step call launches nothing and is fine without a device
    assert L.dfwfm_optim_step(None, 0, ctypes.byref(ok), 1, None) == 0
    assert L.dfwfm_optim_step(tens(grad=None), 1, ctypes.byref(ok), 1, None) == 0
    assert L.dfwfm_optim_step(tens(n=0), 1, ctypes.byref(ok), 1, None) == 0


# --------------------------------------------------------------------------------------------------- the switch
def _sizes():
    return [1] * 13 + [7] * 26


def test_fused_step_signature_has_adam_as_its_default():
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    pars = inspect.signature(FusedTrainStep.__init__).parameters
    assert pars["optimizer"].default == "adam"
    assert pars["momentum"].default == 0.0 and pars["alpha"].default == 0.99
    assert pars["lazy_table_adam"].default is False and pars["lr_schedule"].default is None


def test_cli_flag_parses_and_reaches_the_module():
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd.cli import get_model, get_parser
    p = get_parser()
    assert p.parse_args([]).fused_optimizer == 0
    assert p.parse_args(["-fused_optimizer", "1"]).fused_optimizer == 1
    with pytest.raises(SystemExit):
        p.parse_args(["-fused_optimizer", "2"])
    m = get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args(["-fused_optimizer", "1"]))
    assert m.fused_optimizer is True
    assert "fused_optimizer" not in "".join(m.state_dict())  # a training switch, not state
    assert get_model(cuda=False, feature_sizes=_sizes(), pars=p.parse_args([])).fused_optimizer is False
    assert DeepFMs(field_size=39, feature_sizes=_sizes(), numerical=13, use_cuda=False).fused_optimizer is False


@pytest.mark.parametrize("opt", ["sgd", "adag", "rmsp"])
def test_fit_refuses_the_switch_off_the_fused_step(opt):
    """A module on the CPU: fit() raises before the first batch instead of training through autograd + torch.optim;
    with the switch off the same call trains, as before."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = _sizes()
    xi, xv = synth.synth_inputs(sizes, 13, 64, seed=2)
    y = (np.arange(64) % 2).astype(np.float32)
    m = DeepFMs(field_size=39, feature_sizes=sizes, numerical=13, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1,
                h_depth=1, deep_nodes=16, n_epochs=1, batch_size=32, optimizer_type=opt, momentum=0.9,
                use_cuda=False)
    m.fused_optimizer = True
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(ValueError, match="fused_optimizer"):
        m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    m.fused_optimizer = False
    m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    assert any(not torch.equal(before[k], v) for k, v in m.state_dict().items())


# ------------------------------------------------------------------------------------- the reference helper itself
def _exact_fma(a, b, c):
    """fmaf by exact rational arithmetic: the float32 nearest to a * b + c, ties to the even mantissa."""
    from fractions import Fraction
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    r = np.float32(float(exact))
    cands = {float(r), float(np.nextafter(r, np.float32(np.inf))), float(np.nextafter(r, np.float32(-np.inf)))}
    best = min(cands, key=lambda x: (abs(Fraction(x) - exact), int(np.float32(x).view(np.int32)) & 1))
    return np.float32(best)


def test_fma32_rounds_once():
    """fma32 against exact rational arithmetic: on a case where the float64 sum lands on a float32 tie although the
    exact sum lies below it (two roundings would go up to the even neighbour), and on random draws."""
    f = np.float32
    a, b, c = f(2.0 ** -12 + 2.0 ** -35), f(2.0 ** -12 - 2.0 ** -35), np.nextafter(f(1), f(2))
    twice = f(np.float64(a) * np.float64(b) + np.float64(c))
    assert twice == f(1 + 2.0 ** -22) and _exact_fma(a, b, c) == c  # the double rounding is real here
    assert ref.fma32(a, b, c) == c
    assert ref.fma32(-a, b, -c) == -c
    r = np.random.default_rng(11)
    x, y, z = ((r.standard_normal(300) * 10.0 ** r.uniform(-6, 6, 300)).astype(f) for _ in range(3))
    got = ref.fma32(x, y, z)
    for i in range(300):
        assert got[i] == _exact_fma(x[i], y[i], z[i]), i
    # cancellation: the product against its own rounded value leaves the rounding error, exactly
    assert ref.fma32(f(1 + 2.0 ** -12), f(1 + 2.0 ** -12), -f(1 + 2.0 ** -11)) == f(2.0 ** -24)
