"""CPU: the host kernels (libdfwfm_cpu.so) on the table zoo (tests/table_cases.py) -- tables at the row counts where the
device kernels change path, QR collision counts from 1 to past n -- against the float64 oracle, and the index-range rule
per field: a plain table accepts [0, n), a QR field [0, ceil(n / c) c).  One training step of the zoo's cases runs with
the other variants (tests/test_train_variants.py, train_cases.CASES)."""
import numpy as np
import pytest

import table_cases as zc
import train_cases as tc
from conftest import logit_close
from oracle import dfwfm_oracle
from test_cpu_kernel import cpu_model, run


@pytest.mark.parametrize("op", zc.OPS)
@pytest.mark.parametrize("c", zc.C_ALL)
def test_cpu_forward_zoo_matches_oracle(c, op):
    cfg, params, xi, xv = zc.zoo(1, op, c)
    got = run(cpu_model(cfg, params), xi, xv)
    assert logit_close(got, dfwfm_oracle.forward(cfg, params, xi, xv)) < 1e-5


@pytest.mark.parametrize("qr,deep", [(0, 1), (0, 0), (1, 0)])
def test_cpu_forward_zoo_plain_and_mlp_free(qr, deep):
    cfg, params, xi, xv = zc.zoo(qr, "mult", 7, deep=deep)
    got = run(cpu_model(cfg, params), xi, xv)
    assert logit_close(got, dfwfm_oracle.forward(cfg, params, xi, xv)) < 1e-5


@pytest.mark.parametrize("op", zc.OPS)
@pytest.mark.parametrize("c", zc.C_ALL)
def test_cpu_index_range_per_field(c, op):
    """Per categorical field: the first invalid index (n, or ceil(n / c) c for a QR field), -1 and 2^32 + 3 (valid low
    32 bits: a range check after truncation would pass it) raise IndexError, in the host kernels and in the oracle;
    the last valid index (forced row 2) does not, and a clean batch afterwards passes."""
    cfg, params, xi, xv = zc.zoo(1, op, c)
    m = cpu_model(cfg, params)
    xi, xv = xi[:8], xv[:8]
    for j in range(xi.shape[1]):
        for bad in (zc.valid_end(cfg, j), -1, 2 ** 32 + 3):
            x = xi.copy()
            x[5, j] = bad
            with pytest.raises(IndexError):
                run(m, x, xv)
            with pytest.raises(IndexError):
                dfwfm_oracle.forward(cfg, params, x, xv)
    run(m, xi, xv)


@pytest.mark.parametrize("name,c,op", [("zoo_qr_mult_c1", 1, "mult"), ("zoo_qr_add_c7", 7, "add"),
                                       ("zoo_qr_mult_c5000", 5000, "mult")])
def test_zoo_goldens_hold_the_wide_zoo_and_the_edge_rows(name, c, op):
    """The reference's goldens at c = 1, c = 7 and c > n (tests/test_oracle.py pins the oracle to them): the 39-field
    zoo's tables, 256 rows, the three forced rows in the stored Xi."""
    from conftest import load_golden
    cfg, params, xi, xv, y, l32, l64, _ = load_golden(name)
    assert cfg["feature_sizes"] == [1] * 13 + zc.ROWS_WIDE and max(zc.ROWS_WIDE) < 2500
    assert (cfg["qr_collisions"], cfg["qr_operation"], cfg["qr_flag"], len(xi)) == (c, op, 1, 256)
    zc.check_inputs(cfg, xi)
    assert logit_close(dfwfm_oracle.forward(cfg, params, xi[:3], xv[:3]), l64[:3]) < 1e-11


def test_zoo_cases_are_registered_with_their_edge_rows():
    """Every (c, op) of the zoo trains with the other variants (CASES), on inputs that hold the three forced rows."""
    for op in zc.OPS:
        for c in zc.C_ALL:
            cfg, params, xi, xv, y = tc.case(zc.name(op, c))
            assert cfg["qr_collisions"] == c and cfg["qr_operation"] == op and cfg["qr_threshold"] == zc.THRESHOLD
            assert cfg["feature_sizes"] == [1] * zc.NUM + zc.ROWS and len(xi) == zc.B_TRAIN
            zc.check_inputs(cfg, xi)
            assert params[f"fm_2nd_embeddings.{zc.NUM + 8}.weight"].shape == (200, zc.D)  # 200: still a plain bag
            assert params[f"fm_2nd_embeddings.{zc.NUM + 9}.weight_q"].shape == (-(-201 // c), zc.D)
            assert params[f"fm_2nd_embeddings.{zc.NUM + 9}.weight_r"].shape == (c, zc.D)
