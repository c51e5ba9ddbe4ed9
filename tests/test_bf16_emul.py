"""CPU: the numpy statement of the bf16 deep tower's numeric contract (tests/bf16_emul.py, include/dfwfm_bf16.h) --
its rounding is torch's, its exact case is exact and not degenerate, and the tolerance conditions of the GPU tests
hold between two summation orders of the reference itself."""
import numpy as np
import pytest
import torch

import bf16_emul
from oracle import dfwfm_oracle
from xsdeepfwfm_deprecated_amd import _lib

K_ORDERS = [(11, 32), (23, 16), (37, 50)]  # (shuffle seed, chunk): three other summation orders


@pytest.fixture(autouse=True)
def contract_has_a_path():
    """The emulation states the contract of a path the library has (include/dfwfm_bf16.h); without it these tests
    would describe nothing."""
    assert "dfwfm_bf16_forward" in _lib.BF16_SIGNATURES


def test_bf16_rne_is_torch_rounding():
    rs = np.random.RandomState(0)
    x = np.concatenate([
        rs.standard_normal(20000).astype(np.float32)
        * np.float32(10.0) ** rs.randint(-20, 20, 20000).astype(np.float32),
        rs.randint(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32),  # any bit pattern
        # exact ties: the dropped half is 0x8000, kept mantissa even (rounds down) and odd (rounds up), both signs
        np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F80FFFF, 0x3F808001, 0x3F807FFF,
                  0x00008000, 0x00018000, 0x7F7F8000, 0x7F7E8000], dtype=np.uint32).view(np.float32),
        np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, 0.0, -0.0, np.inf, -np.inf, np.nan],
                 dtype=np.float32),
        np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)])  # NaNs
    got = bf16_emul.bf16_rne(x)
    ref = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    nan = np.isnan(x)
    assert np.isnan(got[nan]).all() and np.isnan(ref[nan]).all()
    assert np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32))  # bits: -0 stays -0
    assert np.isinf(got[np.abs(x) == np.finfo(np.float32).max]).all()  # the largest finite values round to Inf
    assert (got.view(np.uint32)[~nan] & 0xFFFF == 0).all()


def test_exact_case_is_exact():
    cfg, params, xi, xv = bf16_emul.exact_case()
    assert xi.shape[0] == 96
    ref = dfwfm_oracle.forward(cfg, params, xi, xv).astype(np.float32)
    assert np.array_equal(bf16_emul.forward(cfg, params, xi, xv).astype(np.float32), ref)
    for ko in K_ORDERS:
        got = bf16_emul.forward(cfg, params, xi, xv, acc=np.float32, k_order=ko).astype(np.float32)
        assert np.array_equal(got, ref), ko


def test_exact_case_is_not_degenerate():
    cfg, params, xi, xv = bf16_emul.exact_case()
    total, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    assert (parts["deep"] != 0).mean() >= 0.5
    assert len(np.unique(total.astype(np.float32))) >= 0.9 * len(total)
    # the placement the case promises: first and last K index and every 32-wide K chunk carry weights
    for l in (1, 2, 3):
        W = params[f"net_1_linear_{l}.weight"]
        used = np.abs(W).sum(0) > 0
        assert used[0] and used[-1]
        assert all(used[c:c + 32].any() for c in range(0, W.shape[1], 32))


def _reference_alone(cfg, params, xi, xv, r, e, what):
    s = np.maximum(1.0, np.abs(r))
    fmt = (np.abs(e - r) / s).max()
    for ko in K_ORDERS:
        o = bf16_emul.forward(cfg, params, xi, xv, acc=np.float32, k_order=ko)
        d = np.abs(o - e) / s
        print(what, ko, dict(fmt=float(fmt), outside=float((d > 1e-5).mean()), worst_over_fmt=float(d.max() / fmt)))
        assert (d <= 1e-5).mean() >= 0.97, (what, ko)
        assert d.max() <= 0.5 * fmt, (what, ko)


@pytest.mark.parametrize("name", bf16_emul.DEEP_GOLDENS)
def test_gpu_conditions_hold_for_the_reference_alone_goldens(name):
    """A condition on the inputs, not a measurement: another float32 summation order of the same contract stays
    inside the bounds the GPU tests put on the kernel (at most 1.6 % of rows outside 1e-5, worst 0.09 of the format
    error, when this was written)."""
    cfg, params, xi, xv, y, r, e = bf16_emul.golden_case(name)
    _reference_alone(cfg, params, xi, xv, r, e, name)


@pytest.mark.parametrize("i", range(len(bf16_emul.SWEEP)))
def test_gpu_conditions_hold_for_the_reference_alone_sweep(i):
    cfg, params, xi, xv, r, e = bf16_emul.sweep_ref(i)
    _reference_alone(cfg, params, xi, xv, r, e, bf16_emul.SWEEP[i])
