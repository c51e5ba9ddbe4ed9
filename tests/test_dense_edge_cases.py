"""CPU: the references of tests/dense_edge_cases.py alone meet every bar the GPU legs hold the kernels to
(tests/test_gpu_dense_edges.py, tests/test_gpu_adam_edges.py), and the split-K case table is what dw_plan's arithmetic
gives.  No kernel runs here: a bar that float32 arithmetic on the CPU misses would say nothing about a kernel.

Measured here (PyTorch's CPU kernels in float32 against float64):
  split-K cases, fp32 port: gradients within 2.9e-7 .. 2.4e-6 of each tensor's largest entry (bar 2e-5, a quarter of
    it 5e-6); per touched table row 3.8e-6 .. 1.3e-5 (bar 2e-5: kept), but 2.6e-2 on d8n320 at 1100 (per-tensor bar
    alone there); logits within 1.9e-6, the loss within 1.1e-6.
  BCE: |(sigmoid(z) - y) - float64| <= 8.9e-8 (bar 2^-22 = 2.4e-7); every prefix's loss within 1e-7 of the mean.
  Adam: p at 0.25 of its bar, exp_avg within 1.0e-7 and exp_avg_sq within 1.6e-7 (bar 2.4e-7), every betas pair.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_edge_cases as dc
import train_cases as tc


# ---------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("key", list(dc.DW_CASES), ids=lambda k: f"{k[0]}-{k[1]}")
def test_dw_plan_reproduces_the_case_table(key):
    """dw_plan's and dwr_xcd_plan's arithmetic, restated, puts every case on the edge its table entry names."""
    shape, B = key
    splits, rows, last, waves, groups, _ = dc.DW_CASES[key]
    D, N, H = dc.DW_SHAPES[shape]
    ps, nnb, nkb, got_splits, got_rows = dc.dw_plan(D, N, H, B)
    assert (got_splits, got_rows) == (splits, rows)
    assert B - (splits - 1) * rows == last and 0 < last <= rows
    assert dc.dw_waves(B, splits, rows) == waves and sum(waves) == last
    assert dc.dw_groups(D, N, H, B) == groups
    assert splits > 1 and last < rows  # a split batch with a ragged last split
    assert N % dc.DW_EDGE or (dc.F * D) % dc.DW_EDGE  # columns past N or F D in the last block of a row


def test_dw_case_table_covers_every_edge():
    """The edges the table exists for, each met by at least one case."""
    cases = dc.DW_CASES
    assert any(w[1:] == (0, 0, 0) and w[0] % 4 for _, _, _, w, _, _ in cases.values())  # three empty waves, rows % 4
    assert any(0 in w and w[0] % 4 == 0 for _, _, _, w, _, _ in cases.values())
    assert any(g is None for *_, g, _ in cases.values())                     # non-uniform layers: blockIdx order
    assert any(g is not None and g % 8 == 0 and g >= 16 for *_, g, _ in cases.values())  # whole rounds only
    assert any(g is not None and g > 8 and g % 8 for *_, g, _ in cases.values())         # rounds and leftovers
    D, N, H = dc.DW_SHAPES["d16n400"]
    ps, nnb, nkb, _, _ = dc.dw_plan(D, N, H, 131)
    assert nnb * nkb[0] > 32
    (s0, b0), (s1, b1) = dc.DW_PAIR
    assert s0 == s1 and b1 < b0 and cases[(s1, b1)][0] > cases[(s0, b0)][0]  # a smaller batch with more splits
    assert -(-2617 // 16) == 164 and 164 // 4 == 32 + 8 + 1  # reduce_final_block's three loops, per wave


@pytest.mark.parametrize("key", list(dc.DW_CASES), ids=lambda k: f"{k[0]}-{k[1]}")
def test_dw_last_split_rows_carry_gradient(key):
    """Not vacuous: every row of the last split has |sigmoid(z) - y| >= 0.5, and without the last split's rows every
    MLP weight and bias gradient is off by far more than the bar (here: by 100 times G_TOL of its largest entry)."""
    cfg, params, xi, xv, y = dc.dw_case(*key)
    if key == dc.DW_PAIR[1]:
        params = dc.dw_reference(*dc.DW_PAIR[0])[1][3]
    z, _, g = tc.ref_step64(cfg, params, xi, xv, y)
    lo = (dc.DW_CASES[key][0] - 1) * dc.DW_CASES[key][1]
    assert np.all(np.abs(1 / (1 + np.exp(-z[lo:])) - y[lo:]) >= 0.5)
    _, _, head = tc.ref_step64(cfg, params, xi[:lo], xv[:lo], y[:lo])  # mean over lo rows: rescale to the batch's
    for k in g:
        if k.startswith("net_1_linear_"):
            miss = np.abs(g[k] - head[k] * lo / len(xi)).max() / np.abs(g[k]).max()
            assert miss > 100 * tc.G_TOL, (k, miss)


@pytest.mark.parametrize("key", list(dc.DW_CASES), ids=lambda k: f"{k[0]}-{k[1]}")
def test_fp32_port_meets_every_bar_dw(key):
    """The fp32 port against float64 on every case: check_step's bars (logits, loss, per tensor; per row where the
    table keeps it, which is wherever the port meets it), and under a quarter of the per-tensor gradient bar -- the
    precondition that a kernel outside it is wrong and not merely rounding differently."""
    cfg, params, xi, xv, y = dc.dw_case(*key)
    ref, port = dc.dw_reference(*key)
    if key == dc.DW_PAIR[1]:  # the second step of the pair starts from the parameters after the first
        params = dc.dw_reference(*dc.DW_PAIR[0])[1][3]
        ref, port = tc.ref_step64(cfg, params, xi, xv, y), tc.port_step(cfg, params, xi, xv, y, dc.LR, dc.L2)
    wt, wr, kt, kr = tc.grad_stats(cfg, xi, port[2], ref[2])
    print(f"{key}: fp32 port, gradient error over the tensor's max {wt:.2e} ({kt}), over the row's max {wr:.2e}")
    dc.check_dw_step(key, cfg, params, xi, xv, port[0], port[1], port[2], ref)
    assert wt < tc.G_TOL / 4, (kt, wt)
    assert dc.DW_CASES[key][5] == (wr <= tc.G_TOL), (kr, wr)  # the table's flag is the measured fact


# ---------------------------------------------------------------------------------------------------------- B
def test_bce_fixture_holds_every_special_pair():
    z, y = dc.bce_fixture()
    pairs = set(zip(z[:63].tolist(), y[:63].tolist()))
    assert all((np.float32(a), np.float32(b)) in {(np.float32(p), np.float32(q)) for p, q in pairs}
               for a in dc.BCE_SPECIAL for b in dc.BCE_LABELS)
    assert not np.any((z > -89) & (z < -87)) and np.all(np.isfinite(z))
    assert z[dc.BCE_BAD] not in dc.BCE_SPECIAL and set(np.unique(y).tolist()) == {0.0, 1.0, np.float32(0.3).item()}


def test_torch_bce32_meets_the_bars():
    """float32 torch (sigmoid(z) - y, binary_cross_entropy_with_logits) against the float64 reference, at the bars
    of the GPU leg: 2^-22 on the gradient, the project's loss bar on every prefix, the saturated values exact."""
    z, y = dc.bce_fixture()
    d64, l64 = dc.bce_ref64(z, y)
    zt, yt = torch.from_numpy(z.copy()), torch.from_numpy(y.copy())
    d32 = (torch.sigmoid(zt) - yt).numpy()
    err = float(np.abs(d32.astype(np.float64) - d64).max())
    print(f"float32 torch: |dz n - (sigmoid - y)| <= {err:.2e} (bar {dc.DZ_TOL:.2e})")
    assert err <= dc.DZ_TOL
    for n in dc.BCE_N:
        l32 = float(F.binary_cross_entropy_with_logits(zt[:n], yt[:n], reduction="sum"))
        assert dc.loss_close(l32, float(l64[:n].sum()), n), n
        for denom in (n, 3 * n):
            hi, lo, val = dc.bce_saturated32(z[:n], y[:n], denom)
            got = (d32[:n] / np.float32(denom)).astype(np.float32)
            assert np.array_equal(got[hi | lo], val[hi | lo])
            assert np.abs(got.astype(np.float64) * denom - d64[:n]).max() <= dc.DZ_TOL


# ---------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("betas", dc.ADAM_BETAS, ids=str)
def test_torch_adam32_meets_the_bar(betas):
    """torch.optim.Adam in float32 against the float64 restatement over the whole grid: p within rtol 2.4e-7 and
    atol 2e-9, exp_avg and exp_avg_sq within MV_RTOL -- for beta1 <= 0.5 (lerp's other form) as well."""
    worst = [0.0, 0.0, 0.0]
    for step, b, wd, eps, gmin in dc.adam_grid():
        if b != betas:
            continue
        _, r64, t32 = dc.adam_grid_case(step, b, wd, eps, gmin)
        e = (dc.p_err(t32[0], r64[0]), dc.rel_err(t32[1], r64[1]), dc.rel_err(t32[2], r64[2]))
        assert e[0] <= 1.0 and e[1] <= dc.MV_RTOL[b] and e[2] <= dc.MV_RTOL[b], (step, b, wd, eps, e)
        worst = [max(a, c) for a, c in zip(worst, e)]
    print(f"betas {betas}: torch float32, p at {worst[0]:.2f} of its bar, exp_avg {worst[1]:.2e}, "
          f"exp_avg_sq {worst[2]:.2e}")


def test_adam_grid_fixture_is_well_conditioned():
    """What the bars rest on: v normal after the step everywhere (the eps = 0 case included), no cancellation in
    g + wd p or in exp_avg's update, and a quarter of the parameters 0."""
    tiny = float(np.finfo(np.float32).tiny)
    for step, b, wd, eps, gmin in dc.adam_grid():
        (p, g, m, v), r64, _ = dc.adam_grid_case(step, b, wd, eps, gmin)
        assert np.all(r64[2] >= tiny) and np.all(np.isfinite(r64[0]))
        assert np.all(g * p >= 0) and np.all(m.astype(np.float64) * (g + wd * p.astype(np.float64)) > 0)
        assert np.count_nonzero(p == 0) >= len(p) // 4


def test_adam_special_fixture_and_torch_classes():
    """The special-value tensor: every kind at every lane of a float4, in a p = 0 and a p != 0 float4, beside ordinary
    neighbours; and torch's classes on it (1e25: v = inf and p unchanged; NaN and inf: NaN)."""
    p, g, m, v, mask, plain = dc.adam_special_values()
    blk = dc.ADAM_SPECIAL_BLOCK
    for k, (name, val) in enumerate(dc.ADAM_SPECIAL):
        idx = np.flatnonzero(mask[k * blk:(k + 1) * blk])
        assert sorted(set(idx % 4)) == [0, 1, 2, 3] and len(idx) == 8
        assert np.count_nonzero(p[k * blk + idx] == 0) == 4
        for i in idx:  # the other three lanes of its float4 are ordinary
            assert mask[k * blk + i // 4 * 4:k * blk + i // 4 * 4 + 4].sum() == 1
    assert np.all(np.isfinite(plain)) and np.array_equal(plain[~mask], g[~mask])
    tp, tm, tv = dc.adam_torch32(p, g, m, v, *dc.ADAM_SPECIAL_HYPER)
    kind = {name: slice(k * blk, (k + 1) * blk) for k, (name, _) in enumerate(dc.ADAM_SPECIAL)}
    for name in ("huge+", "huge-"):  # ((1 - b2) g) g = 1e37: finite in torch's evaluation order
        s = kind[name]
        assert np.all(np.isfinite(tv[s][mask[s]])) and np.all(tv[s][mask[s]] > 1e36)
    for name in ("over+", "over-"):
        s = kind[name]
        assert np.all(np.isinf(tv[s][mask[s]])) and np.array_equal(tp[s][mask[s]], p[s][mask[s]])
    for name in ("nan", "inf+", "inf-"):
        s = kind[name]
        assert np.all(np.isnan(tp[s][mask[s]]))
    s = kind["zero"]
    assert np.array_equal(tp[s][mask[s]], p[s][mask[s]]) and not np.any(tv[s][mask[s]])
    for name in ("tiny+", "sub+"):
        s = kind[name]
        zero = mask[s] & (p[s] == 0)
        assert np.all(tp[s][zero] < 0) and np.all(np.isfinite(tp[s][mask[s]]))  # the tiny update shows at p = 0
    assert np.all(np.isfinite(tp[~mask]))
