"""GPU: the rounding points of the bf16 and int8 contracts on exact ties (tests/rounding_witness.py; its conditions
are checked on the CPU by test_rounding_witness.py).  On these cases every rounding site rounds, on ties of both
directions, and everything else is exact, so the contract's emulation cast to float32 is the only right answer: no
tolerance.  A kernel that rounds half away from zero, or truncates, at any one site gives other bits in at least a
quarter of the rows."""
import numpy as np
import pytest
import torch

import rounding_witness as rw
from conftest import model_kwargs

pytestmark = pytest.mark.gpu


def make_model(case, device):
    from xsdeepfwfm_deprecated_amd import DeepFMs
    cfg, params, xi, xv = case
    m = DeepFMs(**model_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    return m.to(device).eval()


def run(m, xi, xv, device):
    with torch.no_grad():
        out = m(torch.from_numpy(np.array(xi)).to(device), torch.from_numpy(np.array(xv)).to(device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_bits(m, case, want, device, what):
    """The whole batch, 33 rows (one more than a 32-row tile) and one ordinary row alone (not int8's ZERO_ROW)."""
    cfg, params, xi, xv = case
    assert rw.ZERO_ROW != 58
    for rows in (slice(0, 96), slice(0, 33), slice(58, 59)):
        got = run(m, xi[rows], xv[rows], device)
        assert got.dtype == np.float32
        assert np.array_equal(got, want[rows]), (what, rows, np.flatnonzero(got != want[rows]).tolist())


@pytest.fixture(scope="module")
def bf16_model(gpu):
    return make_model(rw.bf16_case(), gpu)


@pytest.fixture(scope="module")
def bf16_want():
    case = rw.bf16_case()
    return rw.as_f32(rw.bf16_logits(case)), rw.as_f32(rw.bf16_logits(case, fold=True))


def test_bf16_per_layer_forward_rounds_ties_to_even(gpu, bf16_model, bf16_want):
    m = bf16_model
    m.mlp_dtype, m.bf16_fused, m.bf16_fold = "bf16", False, False
    check_bits(m, rw.bf16_case(), bf16_want[0], gpu, "per-layer bf16")
    assert m._engine.bf16 and not m._engine.bf16_fused


@pytest.mark.parametrize("tile", ["", "bf16rows=16", "bf16rows=32", "bf16rows=64"])
@pytest.mark.parametrize("fold", [False, True])
def test_bf16_fused_forward_rounds_ties_to_even(gpu, monkeypatch, bf16_model, bf16_want, fold, tile):
    """x_0, x_l and the weight pack of the one-launch forward; with the fold, bf16(Xv) and bf16(P)."""
    if tile:
        monkeypatch.setenv("DFWFM_DIAG", tile)
    m = bf16_model
    m.mlp_dtype, m.bf16_fused, m.bf16_fold = "bf16", True, fold
    check_bits(m, rw.bf16_case(), bf16_want[int(fold)], gpu, ("fused bf16", fold, tile))
    assert m._engine.bf16_fused and m._engine._bf16_fold_on is fold


@pytest.mark.parametrize("tile", ["", "int8rows=16", "int8rows=32"])
def test_int8_forward_rounds_ties_to_even(gpu, monkeypatch, tile):
    """q and qW on half-integers at both layers; the all-zero input row and the all-zero weight rows."""
    if tile:
        monkeypatch.setenv("DFWFM_DIAG", tile)
    case = rw.int8_case()
    m = make_model(case, gpu)
    m.mlp_dtype = "int8"
    check_bits(m, case, rw.as_f32(rw.int8_logits(case)), gpu, ("int8", tile))
    assert m._engine.int8
    z = rw.ZERO_ROW  # the zero row alone: a = 0, h_1 = relu(b_1)
    cfg, params, xi, xv = case
    assert np.array_equal(run(m, xi[z:z + 1], xv[z:z + 1], gpu), rw.as_f32(rw.int8_logits(case))[z:z + 1])
