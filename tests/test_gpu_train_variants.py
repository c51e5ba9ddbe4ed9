"""GPU: one HIP training step (dfwfm_train_forward / dfwfm_backward / HIP Adam) on the model variants and shapes no
golden trains (train_cases.CASES), against a float64 autograd reference of the same step -- the sorted per-row-owner
scatter (deterministic) and the atomic scatter both -- plus ragged batches, dropout rates other than 0.5 and the
fused graph step on four of the variants.  tests/test_train_variants.py runs the same cases on the host kernels.

Worst gradient error measured on an MI355X, as |g - g64|.max() over the float64 reference's largest entry of the
tensor / of the touched table row (bar: G_TOL = 2e-5 for both; the numbers are evidence of margin, not thresholds).
The sorted and the atomic scatter gave the same figures on every case (at B = 37 a row is read by one or two
samples).  "port" is the yardstick: oracle/torch_port.train_step, fp32 on PyTorch's CPU kernels; "host" the host
kernels (tests/test_train_variants.py).

    case              port tensor / row    host tensor / row    HIP sorted = atomic, tensor / row
    fm_deep           2.0e-7 / 3.0e-7      3.6e-7 / 3.7e-7      2.9e-7 / 4.1e-7
    fm_deep_nolw      2.2e-7 / 2.7e-7      3.7e-7 / 4.2e-7      3.3e-7 / 4.7e-7
    fm_shallow        1.6e-7 / 2.7e-7      2.8e-7 / 3.5e-7      2.8e-7 / 3.9e-7
    logit             1.4e-7 / 4.7e-8      1.4e-7 / 4.7e-8      1.1e-7 / 4.7e-8
    fwfm_shallow_lw   2.4e-7 / 3.6e-7      3.5e-7 / 5.5e-7      3.8e-7 / 4.7e-7
    fwlw_lw           3.4e-7 / 5.5e-7      3.4e-7 / 1.3e-6      4.4e-7 / 1.6e-6
    qr_add            2.2e-7 / 3.4e-7      3.6e-7 / 6.3e-7      4.0e-7 / 5.1e-7
    qr_add_fwlw       2.2e-7 / 4.6e-7      5.3e-7 / 1.2e-6      2.2e-7 / 5.7e-7
    embbag            3.0e-7 / 3.6e-7      3.7e-7 / 6.3e-7      3.8e-7 / 4.7e-7
    num0              3.3e-7 / 1.2e-6      4.5e-7 / 1.6e-6      6.2e-7 / 1.3e-6
    allnum            2.1e-7 / -           3.5e-7 / -           1.8e-7 / -        (no categorical table)
    num20             2.4e-7 / 2.6e-7      2.5e-7 / 3.2e-7      2.0e-7 / 2.9e-7
    f64               2.7e-7 / 2.0e-6      5.5e-7 / 1.6e-6      6.9e-7 / 2.1e-6
    logit_num20       1.4e-7 / 2.4e-8      1.4e-7 / 2.4e-8      1.1e-7 / 2.4e-8
    dropout p = 0.1   3.7e-7 / 4.5e-7      3.7e-7 / 5.0e-7      3.3e-7 / 6.4e-7
    dropout p = 0.9   3.5e-7 / 1.4e-6      9.3e-7 / 1.9e-6      1.0e-6 / 2.3e-6

The table zoo's cases (zoo_*, zoo39_*: tests/table_cases.py) run here too; their figures are in the table of
tests/test_gpu_train_tables.py.

The per-row figure only means something on well-conditioned samples (train_cases.SEEDS): a table row read by one
sample carries that sample's (sigmoid(z) - y) / B, and with logits of size 1e2 the fp32 port itself is off by 1e-5 to
100 % of such a row on most seeds.
"""
import numpy as np
import pytest
import torch

import train_cases as tc
from conftest import logit_close
from oracle import torch_port
from test_gpu_train import DP_TOL, G_TOL, build, check_dp, hip_step

pytestmark = pytest.mark.gpu

LR, L2 = 1e-3, 3e-7
assert tc.G_TOL == G_TOL  # one bar for the host and the HIP legs


@pytest.mark.parametrize("det", [True, False], ids=["sorted", "atomic"])
@pytest.mark.parametrize("name", list(tc.CASES))
def test_train_variant_matches_float64(gpu, name, det):
    """Logits, loss, every gradient (per tensor; per touched table row; untouched rows exactly 0) and the Adam
    update.  f64: F = 64, num = 16, D = 10, N = 256 needs 37 972 floats = 148.3 KiB of backward LDS (bwd_layout:
    lw 64 + fwlw 640 + rsk 4096 + E 16 x 644 + dE 16 x 644 + G / Gram 8192 + dl 16 + fc 260 + tail 2048 + fo 1024 +
    xv 1024), under the 160 KiB refusal; its 136 tensors take Adam's 91-tensor launches (kAdamList) twice."""
    cfg, params, xi, xv, y = tc.case(name)
    ref, (_, _, og, onew) = tc.reference(name)
    m = build(cfg, params, gpu, is_deep_dropout=False)
    m.deterministic = det
    out, loss, grads, newp = hip_step(m, xi, xv, y, gpu, LR, L2)
    wt, wr, kt, kr = tc.grad_stats(cfg, xi, grads, ref[2])
    print(f"{name} {'sorted' if det else 'atomic'}: HIP, gradient error over the tensor's max {wt:.2e} ({kt}), "
          f"over the row's max {wr:.2e} ({kr})")
    tc.check_step(cfg, params, xi, xv, out, loss, grads, ref)
    assert check_dp(cfg, params, grads, newp, og, onew, LR, L2) <= DP_TOL


@pytest.mark.parametrize("name,B", tc.RAGGED)
def test_train_variant_ragged(gpu, name, B):
    """One row, one full tile, one full tile and a row: the layouts without numerical / categorical fields and the
    model without a per-tile backward."""
    cfg, params, xi, xv, y = tc.ragged_case(name, B)
    m = build(cfg, params, gpu, is_deep_dropout=False)
    out, loss, grads, _ = hip_step(m, xi, xv, y, gpu, LR, L2)
    tc.check_step(cfg, params, xi, xv, out, loss, grads, tc.reference(name, B)[0])


@pytest.mark.parametrize("p", tc.DROPOUT_RATES)
def test_train_dropout_rates(gpu, p):
    """Deep-tower dropout away from p = 0.5: drop_scale = 1 / (1 - p) is 1.11 and 10, not 2."""
    cfg, params, xi, xv, y, _ = tc.dropout_case(0, p)
    m = build(cfg, params, gpu, is_deep_dropout=True)
    m.dropout_deep = [p] * (cfg["h_depth"] + 1)
    seed = tc.dropout_seed()  # what train_forward draws next (after the constructor, which seeds torch itself)
    masks = tc.dropout_case(seed, p)[5]
    out, loss, grads, _ = hip_step(m, xi, xv, y, gpu, LR, 0.0)
    wt, wr = tc.check_step(cfg, params, xi, xv, out, loss, grads, tc.ref_step64(cfg, params, xi, xv, y, masks, p))
    print(f"dropout p={p}: HIP, gradient error over the tensor's max {wt:.2e}, over the row's max {wr:.2e}")
    if p == 0.9:  # not vacuous: some hidden units survive
        assert any(np.any(grads[f"net_1_linear_{i}.weight"]) for i in range(1, cfg["h_depth"] + 1))


@pytest.mark.parametrize("name", tc.FUSED)
def test_fused_step_variants(gpu, name):
    """FusedTrainStep (step 1 eager, steps 2 and 3 replayed from the captured graph) at the bars of
    test_gpu_train.test_fused_graph_steps_match_oracle.  Every parameter of these variants is in the kernels'
    gradient layout, so none is refused."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    B, K = 32, 3
    cfg, params, xi, xv, y = tc.case(name, B * K)
    bats = [(xi[k * B:(k + 1) * B], xv[k * B:(k + 1) * B], y[k * B:(k + 1) * B]) for k in range(K)]
    m = build(cfg, params, gpu, is_deep_dropout=False)
    t = FusedTrainStep(m, B, lr=LR, weight_decay=L2)
    logits = []
    for xb, vb, yb in bats:
        t.step(torch.from_numpy(xb).to(gpu), torch.from_numpy(vb).to(gpu), torch.from_numpy(yb).to(gpu))
        logits.append(t.out[:B].detach().cpu().numpy().copy())
    torch.cuda.synchronize()
    assert t.graphs is not None  # steps 2.. replayed
    outs, onew = torch_port.train_steps(cfg, params, [(tc.port_xi(a), b, c) for a, b, c in bats], LR, L2)
    for k in range(K):
        assert logit_close(logits[k], outs[k]) < 1e-4, k
    e = np.concatenate([np.abs(p.detach().cpu().numpy() - onew[k]).reshape(-1) / LR for k, p in m.named_parameters()])
    assert np.median(e) < 1e-3 and np.quantile(e, 0.999) < 0.05, (np.median(e), np.quantile(e, 0.999))
    ref_loss = sum(float(torch.nn.functional.binary_cross_entropy_with_logits(
        torch.from_numpy(o), torch.from_numpy(yb), reduction="sum")) for o, (_, _, yb) in zip(outs, bats))
    assert abs(t.loss_sum.item() - ref_loss) <= 1e-4 * abs(ref_loss)
    t.close()
