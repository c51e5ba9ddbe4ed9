"""The dense half of the training step at its edges: the cases, fixtures and float64 references that the CPU leg
(tests/test_dense_edge_cases.py: the references alone meet every bar) and the GPU legs (tests/test_gpu_dense_edges.py:
split-K weight gradients and the BCE kernels; tests/test_gpu_adam_edges.py: Adam) share.

A. Split-K weight gradients (dwr_kernel, dwr_reduce_kernel, dw_sum_kernel; planned by dw_plan).  DW_CASES crosses a
   split batch with a ragged last split, empty waves, row counts that are no multiple of 4, N and F D that are no
   multiple of the 80-wide block, and every grouping of dwr_xcd_plan.  dw_plan / dw_groups restate the host planning,
   so a later change of the plan that moves a case off its edge fails test_dw_plan_reproduces_the_case_table.
B. bce_fixture: logits from saturated to denormal-free extremes against every label, taken as prefixes.
C. Adam: one value vector for the position / alignment tests, the (step, betas, weight_decay, eps) grid with its
   float64 reference (adam_ref64) and torch's own float32 step (adam_torch32), and the special-value tensor.
"""
import functools
import math

import numpy as np
import torch

import train_cases as tc

# ----------------------------------------------------------------------------------------------------------
# A. split-K weight gradients
DW_EDGE, DW_QUANTUM, DW_WAVES = 80, 64, 4  # kDwEdge, kDwRows, dwr_kernel<4, 4>'s waves
F, NUM = 39, 13
LR, L2 = 1e-3, 3e-7

DW_SHAPES = {  # name: (D, N, H)
    "d4n96": (4, 96, 2),      # uniform nkb [2, 2], nnb nkb = 4 <= 32: groups of 4
    "d10n96": (10, 96, 2),    # nkb [5, 2]: non-uniform, blockIdx order
    "d16n400": (16, 400, 1),  # nnb nkb = 40 > 32: groups of nkb = 8
    "d8n320": (8, 320, 2),    # uniform [4, 4]: groups of 16
    "criteo": (10, 400, 3),   # the Criteo MLP, uniform [5, 5, 5]: groups of 25
}
# (shape, B): (splits, rows per split, rows of the last split, rows of its four waves, block groups or None,
#              per-row bar kept).
# Per-row bar: check_step's bar on every touched table row (G_TOL of the row's largest entry) is kept where the fp32
# port itself meets it on that case (test_fp32_port_meets_every_bar_dw measures it: 3.8e-6 .. 1.3e-5); the d8n320 pair's
# first step (1100 rows) has the per-tensor bar alone: there a table row is read only by samples whose
# (sigmoid(z) - y) is ill-conditioned in fp32 (train_cases.SEEDS's comment) and the port itself is 2.6e-2 of that row
# off.  After that step's update the 1000-row step is well conditioned again (port 8.3e-6) and keeps the per-row bar.
DW_CASES = {
    ("d4n96", 129): (2, 128, 1, (1, 0, 0, 0), 4, True),
    ("d4n96", 131): (2, 128, 3, (3, 0, 0, 0), 4, True),
    ("d4n96", 200): (2, 128, 72, (32, 32, 8, 0), 4, True),
    ("d4n96", 257): (3, 128, 1, (1, 0, 0, 0), 6, True),
    ("d4n96", 500): (4, 128, 116, (32, 32, 32, 20), 8, True),
    ("d4n96", 1000): (8, 128, 104, (32, 32, 32, 8), 16, True),   # two whole rounds of eight groups
    ("d4n96", 1100): (9, 128, 76, (32, 32, 12, 0), 18, True),    # two rounds + 2
    ("d4n96", 2617): (21, 128, 57, (32, 25, 0, 0), 42, True),    # 164 tiles: 41 = 32 + 8 + 1 per wave (final sums)
    ("d10n96", 131): (2, 128, 3, (3, 0, 0, 0), None, True),
    ("d10n96", 500): (4, 128, 116, (32, 32, 32, 20), None, True),
    ("d16n400", 131): (2, 128, 3, (3, 0, 0, 0), 10, True),
    ("d16n400", 500): (4, 128, 116, (32, 32, 32, 20), 20, True),
    ("d16n400", 1000): (6, 192, 40, (40, 0, 0, 0), 30, True),
    ("d8n320", 1100): (6, 192, 140, (48, 48, 44, 0), 12, False),
    ("d8n320", 1000): (8, 128, 104, (32, 32, 32, 8), 16, True),   # after 1100 on the same model: more splits
    ("criteo", 257): (3, 128, 1, (1, 0, 0, 0), 9, True),         # one round + 1
    ("criteo", 500): (3, 192, 116, (48, 48, 20, 0), 9, True),
}
DW_PAIR = (("d8n320", 1100), ("d8n320", 1000))  # run in this order on one model
DW_SINGLE = [k for k in DW_CASES if k not in DW_PAIR]
DW_FUSED = [("d4n96", 131), ("criteo", 500)]     # FusedTrainStep: dwr_reduce_kernel


def dw_plan(D, N, H, B):
    """dw_plan (csrc/dfwfm_capi.hip): (blocks per split, nkb per layer, splits, rows per split) for a batch of B."""
    nnb = -(-N // DW_EDGE)
    nkb = [-(-(F * D if l == 1 else N) // DW_EDGE) for l in range(1, H + 1)]
    ps = nnb * sum(nkb)
    sp = max(1, min(256 // ps, (B + 127) // 128))
    rows = -(-(-(-B // sp)) // DW_QUANTUM) * DW_QUANTUM
    return ps, nnb, nkb, -(-B // rows), rows


def dw_groups(D, N, H, B):
    """dwr_xcd_plan (csrc/dfwfm_train.hip): the number of XCD-local block groups, None for blockIdx order."""
    ps, nnb, nkb, splits, _ = dw_plan(D, N, H, B)
    total = ps * splits
    if any(k != nkb[0] for k in nkb) or total % nkb[0]:
        return None
    sg = nnb * nkb[0]
    return total // (sg if sg <= 32 else nkb[0])


def dw_waves(B, splits, rows):
    """Rows of the last split's four waves (dwr_block: a contiguous quarter of the split each, clamped to the batch)."""
    q, lo = rows // DW_WAVES, (splits - 1) * rows
    return tuple(max(0, min(lo + (w + 1) * q, B) - (lo + w * q)) for w in range(DW_WAVES))


def dw_last_split(key):
    """The first row of the case's last split (of the pair: of the earlier of its two batches' last splits)."""
    if key in DW_PAIR:
        return min((DW_CASES[k][0] - 1) * DW_CASES[k][1] for k in DW_PAIR)
    return (DW_CASES[key][0] - 1) * DW_CASES[key][1]


@functools.lru_cache(maxsize=None)
def dw_case(shape, B):
    """(cfg, params, xi, xv, y) of a DW_CASES entry; the pair's second batch is the first's leading rows.
    train_case's logits reach 60 and most of its samples are classified right, with sigmoid(z) - y ~ 0: a last split
    of one such row adds nothing to any gradient, and a kernel that dropped it would pass.  So every row of the last
    split is labelled against its (float64) logit: |sigmoid(z) - y| >= 0.5 there, well conditioned, and each of those
    rows weighs at least as much as any other row of the batch (test_dw_last_split_rows_carry_gradient)."""
    D, N, H = DW_SHAPES[shape]
    if (shape, B) == DW_PAIR[1]:
        cfg, params, xi, xv, y = dw_case(*DW_PAIR[0])
        return cfg, params, xi[:B], xv[:B], y[:B]
    cfg, params, xi, xv, y = tc.train_case(F, NUM, D, N, H, B=B)
    from oracle import torch_port
    with torch.no_grad():
        z = torch_port.forward_graph(cfg, {k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()},
                                     torch.as_tensor(tc.port_xi(xi)), torch.as_tensor(xv, dtype=torch.float64)).numpy()
    lo = dw_last_split((shape, B))
    y = y.copy()
    y[lo:] = z[lo:] < 0
    return cfg, params, xi, xv, y


@functools.lru_cache(maxsize=None)
def dw_reference(shape, B):
    """(ref_step64, port_step) of a case from its initial parameters, computed once; read, never written."""
    cfg, params, xi, xv, y = dw_case(shape, B)
    return tc.ref_step64(cfg, params, xi, xv, y), tc.port_step(cfg, params, xi, xv, y, LR, L2)


def check_dw_step(key, cfg, params, xi, xv, out, loss, grads, ref):
    """train_cases.check_step at the case's bars: logits 1e-5, the loss, G_TOL per tensor, and per touched row where
    DW_CASES keeps it.  Returns the worst (per-tensor, per-row) ratios."""
    return tc.check_step(cfg, params, xi, xv, out, loss, grads, ref, per_row=DW_CASES[key][5])


# ----------------------------------------------------------------------------------------------------------
# B. BCE gradient and loss
BCE_SPECIAL = (0.0, 1e-8, -1e-8, 1.0, -1.0, 17.0, -17.0, 30.0, -30.0, 60.0, -60.0, 90.0, -90.0, 104.0, -104.0, 120.0,
               -120.0)
BCE_LABELS = (0.0, 1.0, 0.3)
BCE_N = (1, 63, 64, 65, 255, 256, 257, 4097)
BCE_BAD = 60  # the index that takes the NaN / +-inf logit: an ordinary element, inside every prefix from 63 on
DZ_TOL = 2.0 ** -22  # |dz denom - (sigmoid(z) - y)|: 4 ulp of 1 (expf within 2 ulp, an add, a reciprocal and a
#                      subtraction on values <= 1, one correctly rounded division)


@functools.lru_cache(maxsize=None)
def bce_fixture():
    """(z, y), 4097 float32 each: every special logit against every label first (51 pairs, so the prefix of 63 holds
    them all), then N(0, 3) logits with labels drawn from the three.  No logit lies in (-89, -87), where sigmoid is
    denormal or flushed depending on the implementation."""
    rng = np.random.default_rng(2024)
    zs = np.repeat(np.asarray(BCE_SPECIAL, np.float32), len(BCE_LABELS))
    ys = np.tile(np.asarray(BCE_LABELS, np.float32), len(BCE_SPECIAL))
    n = max(BCE_N) - len(zs)
    z = np.concatenate([zs, (3.0 * rng.standard_normal(n)).astype(np.float32)])
    y = np.concatenate([ys, np.asarray(BCE_LABELS, np.float32)[rng.integers(0, 3, n)]])
    assert not np.any((z > -89) & (z < -87)) and len(z) == max(BCE_N)
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y


def bce_ref64(z, y):
    """(sigmoid(z) - y, per-sample loss) in float64: max(z, 0) - z y + log1p(exp(-|z|))."""
    z, y = z.astype(np.float64), y.astype(np.float64)
    e = np.exp(-np.abs(z))
    sg = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return sg - y, np.maximum(z, 0.0) - z * y + np.log1p(e)


def bce_saturated32(z, y, denom):
    """The exact dz of a saturated logit, in the kernels' float32 operations: z >= 30 (sigmoid rounds to 1):
    fl(fl(1 - y) / denom); z <= -90 (expf overflows, sigmoid 0): fl(-y / denom).  (hi mask, lo mask, value)."""
    d = np.float32(denom)
    hi, lo = z >= 30, z <= -90
    val = np.where(hi, (np.float32(1.0) - y) / d, (np.float32(0.0) - y) / d).astype(np.float32)
    return hi, lo, val


def loss_close(got_sum, ref_sum, n):
    """The project's loss bar on the mean: |got / n - ref / n| <= 1e-5 max(1, |ref / n|)."""
    return abs(got_sum / n - ref_sum / n) <= 1e-5 * max(1.0, abs(ref_sum / n))


# ----------------------------------------------------------------------------------------------------------
# C. Adam
ADAM_N = 8193
ADAM_NUMELS = (1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
ADAM_SLOTS = (0, 45, 90, 91, 92, 182)  # of a 183-tensor list: kAdamList = 91 tensors per launch
ADAM_LIVE = 183
ADAM_BLOCK, ADAM_GRID = 4096, 2048     # kAdamBlock, kAdamGrid
ADAM_STATE_BYTES = 48                  # {int64 step; 7 float scalars; int32 ticket; pad}

ADAM_STEPS = (1, 2, 10, 1000, 10 ** 6, 2 ** 31)
ADAM_BETAS = ((0.9, 0.999), (0.5, 0.9), (0.3, 0.999), (0.0, 0.5))
ADAM_WD = (0.0, 3e-7, 0.1)
ADAM_EPS = (1e-8, 1e-3)
ADAM_LR = 1e-3
P_RTOL, P_ATOL = 2.4e-7, 2e-9  # test_gpu_train.test_adam_matches_torch_over_steps's bar on p
# rtol on exp_avg and exp_avg_sq against float64, per betas: 2.4e-7 for all four.  torch's own float32 step meets it
# for beta1 <= 0.5 too, where its lerp takes the weight >= 0.5 form and the kernel does not (measured worst over the
# grid, exp_avg / exp_avg_sq: (0.9, 0.999) 6.4e-8 / 1.2e-7, (0.5, 0.9) 9.9e-8 / 1.2e-7, (0.3, 0.999) 1.0e-7 / 1.2e-7,
# (0.0, 0.5) 9.2e-8 / 1.6e-7; p at 0.25 of its bar: test_torch_adam32_meets_the_bar), so no combination is widened.
MV_RTOL = {b: 2.4e-7 for b in ADAM_BETAS}


def adam_values(n=ADAM_N, seed=7):
    """(p, g, m, v) float32 with v != 0: gradients over eight decades, m and v of the gradients' scale."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 1, n)).astype(np.float32)
    m = (g * rng.uniform(-1.5, 1.5, n)).astype(np.float32)
    v = (g.astype(np.float64) ** 2 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    assert np.all(v > 0)
    return p, g, m, v


def adam_grid_values(wd, n=4099, seed=19, gmin=0.0):
    """(p, g, m, v) for the hyper-parameter grid.  g has p's sign and exp_avg the sign of the effective gradient
    g + wd p, so that neither g + wd p nor exp_avg's update cancels: where one does, the result's relative error is
    unbounded in any float32 implementation and says nothing about the kernel.  A quarter of the parameters are 0.
    gmin: |g| >= gmin (the eps = 0 case: v stays normal)."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    p[: n // 4] = 0.0
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 1, n)).astype(np.float32)
    g = np.where(p < 0, -np.abs(g), np.where(p > 0, np.abs(g), g)).astype(np.float32)
    if gmin:
        g = np.where(np.abs(g) < gmin, np.copysign(np.float32(gmin), g), g).astype(np.float32)
    ge = g.astype(np.float64) + wd * p.astype(np.float64)
    m = (ge * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    v = (ge ** 2 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    return p, g, m, v


def adam_ref64(p, g, m, v, step, lr, b1, b2, eps, wd):
    """torch.optim.Adam's single-tensor step (torch/optim/adam.py, _single_tensor_adam) in float64."""
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        g = g + wd * p
        m = m + (g - m) * (1.0 - b1)
        v = v * b2 + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        p = p - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v


def adam_torch32(p, g, m, v, step, lr, b1, b2, eps, wd):
    """torch.optim.Adam(foreach=False) on the CPU in float32, its state preset to step - 1."""
    q = torch.from_numpy(p.copy()).requires_grad_(True)
    q.grad = torch.from_numpy(g.copy())
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m.copy()),
                    "exp_avg_sq": torch.from_numpy(v.copy())}
    opt.step()
    st = opt.state[q]
    return q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def adam_grid():
    """Every (step, betas, wd, eps) of the grid, and the eps = 0 case on gradients with |g| >= 1e-15."""
    combos = [(s, b, wd, eps, 0.0) for s in ADAM_STEPS for b in ADAM_BETAS for wd in ADAM_WD for eps in ADAM_EPS]
    return combos + [(10, (0.9, 0.999), 0.0, 0.0, 1e-15)]


@functools.lru_cache(maxsize=None)
def adam_grid_case(step, betas, wd, eps, gmin):
    """((p, g, m, v), float64 result, torch float32 result) of one grid entry, computed once."""
    vals = adam_grid_values(wd, gmin=gmin)
    args = (step, ADAM_LR, betas[0], betas[1], eps, wd)
    return vals, adam_ref64(*vals, *args), adam_torch32(*vals, *args)


def rel_err(got, ref):
    """max |got - ref| / |ref| over ref != 0 (0 where ref is 0 and got is too, inf where only ref is)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        e = np.where(ref != 0, np.abs(got - ref) / np.abs(ref), np.where(got != 0, np.inf, 0.0))
    return float(e.max(initial=0.0))


def p_err(got, ref):
    """max of |got - ref| / (P_ATOL + P_RTOL |ref|): <= 1 is numpy's assert_allclose at the bar on p."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (P_ATOL + P_RTOL * np.abs(ref))).max(initial=0.0))


# the special-value tensor: twelve kinds of gradient, each in its own 64-float block, at a different lane of eight
# float4 of the block, beside ordinary neighbours; the first half of every block has p = 0 (tiny updates show)
ADAM_SPECIAL = (("zero", 0.0), ("tiny+", 1e-30), ("tiny-", -1e-30), ("sub+", 1e-20), ("sub-", -1e-20),
                ("huge+", 1e20), ("huge-", -1e20), ("over+", 1e25), ("over-", -1e25), ("nan", float("nan")),
                ("inf+", float("inf")), ("inf-", float("-inf")))
ADAM_SPECIAL_BLOCK = 64
ADAM_SPECIAL_HYPER = (3, ADAM_LR, 0.9, 0.999, 1e-8, 0.0)  # step, lr, betas, eps; no weight decay: g is what it says


def adam_special_values(seed=23):
    """(p, g, m, v, special mask, g with the specials replaced by ordinary gradients).  zero / tiny / sub kinds sit on
    m = v = 0 (g = 0: nothing moves; 1e-30: g g underflows, v stays 0; 1e-20: v becomes subnormal); the huge, over, NaN
    and inf kinds on ordinary m and v.  1e20: g g overflows, but torch's addcmul_ and the kernel both form
    ((1 - b2) g) g = 1e37, so v stays finite there; 1e25 is the gradient at which that product overflows too
    (v = inf, p does not move)."""
    n = ADAM_SPECIAL_BLOCK * len(ADAM_SPECIAL)
    p, g, m, v = adam_grid_values(0.0, n=n, seed=seed)
    p = np.where(np.arange(n) % ADAM_SPECIAL_BLOCK < ADAM_SPECIAL_BLOCK // 2, np.float32(0), np.abs(p) + 0.5)
    p = p.astype(np.float32)
    plain = g.copy()
    mask = np.zeros(n, bool)
    for k, (name, val) in enumerate(ADAM_SPECIAL):
        for j in range(0, 8, 2):  # float4 0, 2, 4, 6 of each half of the block, at lanes 0, 1, 2, 3
            i = k * ADAM_SPECIAL_BLOCK + 4 * j + j // 2
            i2 = i + ADAM_SPECIAL_BLOCK // 2
            for t in (i, i2):
                g[t] = val
                mask[t] = True
                if name in ("zero", "tiny+", "tiny-", "sub+", "sub-"):
                    m[t] = v[t] = 0.0
    return p, g, m, v, mask, plain
