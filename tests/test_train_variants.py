"""CPU: one training step of the host kernels (libdfwfm_cpu.so) on every case of train_cases.CASES -- the model
variants and shapes no golden trains -- against a float64 autograd reference; and the yardstick for the bars:
the fp32 port's own error against that reference, on every input the CPU and GPU legs use.

Worst gradient error over the reference's largest entry (per tensor / per touched table row), bar 2e-5:
the table in tests/test_gpu_train_variants.py (host kernels and fp32 port beside the HIP legs)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_cases as tc
from test_cpu_kernel import cpu_model


def cpu_step(cfg, params, xi, xv, y, **kw):
    m = cpu_model(cfg, params, **kw).train()
    out = m(torch.from_numpy(xi), torch.from_numpy(xv))
    loss = F.binary_cross_entropy_with_logits(out, torch.from_numpy(y))
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().numpy().copy()) for k, p in m.named_parameters()}
    return out.detach().numpy(), float(loss.item()), grads


def port_within_quarter_bar(what, cfg, xi, port_grads, g64):
    wt, wr, kt, kr = tc.grad_stats(cfg, xi, port_grads, g64)
    print(f"{what}: fp32 port, gradient error over the tensor's max {wt:.2e}, over the row's max {wr:.2e}")
    assert wt < tc.G_TOL / 4, (kt, wt)
    assert wr < tc.G_TOL / 4, (kr, wr)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_cpu_train_variant_matches_float64(name):
    cfg, params, xi, xv, y = tc.case(name)
    out, loss, grads = cpu_step(cfg, params, xi, xv, y, is_deep_dropout=False)
    wt, wr = tc.check_step(cfg, params, xi, xv, out, loss, grads, tc.reference(name)[0])
    print(f"{name}: host kernels, gradient error over the tensor's max {wt:.2e}, over the row's max {wr:.2e}")


@pytest.mark.parametrize("name,B", tc.RAGGED)
def test_cpu_train_variant_ragged(name, B):
    cfg, params, xi, xv, y = tc.ragged_case(name, B)
    out, loss, grads = cpu_step(cfg, params, xi, xv, y, is_deep_dropout=False)
    tc.check_step(cfg, params, xi, xv, out, loss, grads, tc.reference(name, B)[0])


@pytest.mark.parametrize("name", list(tc.CASES))
def test_fp32_port_within_quarter_bar(name):
    """The precondition of check_step's bars: fp32 arithmetic alone (oracle/torch_port.train_step, PyTorch's CPU
    kernels) stays under G_TOL / 4 of each tensor's and of each touched table row's largest gradient entry, so a
    kernel outside G_TOL is wrong and not merely rounding differently.  A case that misses gets another seed
    (train_cases.SEEDS), never another bar."""
    ref, port = tc.reference(name)
    port_within_quarter_bar(name, tc.case(name)[0], tc.case(name)[2], port[2], ref[2])


@pytest.mark.parametrize("name,B", tc.RAGGED)
def test_fp32_port_within_quarter_bar_ragged(name, B):
    ref, port = tc.reference(name, B)
    cfg, _, xi, _, _ = tc.ragged_case(name, B)
    port_within_quarter_bar(f"{name}/B={B}", cfg, xi, port[2], ref[2])


@pytest.mark.parametrize("p", tc.DROPOUT_RATES)
def test_fp32_port_within_quarter_bar_dropout(p):
    cfg, params, xi, xv, y, masks = tc.dropout_case(tc.dropout_seed(), p)
    _, _, og, _ = tc.port_step(cfg, params, xi, xv, y, 1e-3, 0.0, masks, p)
    port_within_quarter_bar(f"dropout p={p}", cfg, xi, og, tc.ref_step64(cfg, params, xi, xv, y, masks, p)[2])


@pytest.mark.parametrize("p", tc.DROPOUT_RATES)
def test_cpu_train_dropout_rates(p):
    """Deep-tower dropout away from p = 0.5 (drop_scale 1 / (1 - p) = 1.11 and 10): the host kernels' masks and
    scale against the float64 reference with the oracle's rebuilt masks."""
    cfg, params, xi, xv, y, _ = tc.dropout_case(0, p)
    m = cpu_model(cfg, params, is_deep_dropout=True).train()
    m.dropout_deep = [p] * (cfg["h_depth"] + 1)
    seed = tc.dropout_seed()  # after the constructor, which seeds torch itself
    masks = tc.dropout_case(seed, p)[5]
    out = m(torch.from_numpy(xi), torch.from_numpy(xv))
    loss = F.binary_cross_entropy_with_logits(out, torch.from_numpy(y))
    loss.backward()
    grads = {k: q.grad.detach().numpy().copy() for k, q in m.named_parameters()}
    wt, wr = tc.check_step(cfg, params, xi, xv, out.detach().numpy(), float(loss.item()), grads,
                           tc.ref_step64(cfg, params, xi, xv, y, masks, p))
    print(f"dropout p={p}: host kernels, gradient error over the tensor's max {wt:.2e}, over the row's max {wr:.2e}")
    assert any(np.any(grads[f"net_1_linear_{i}.weight"]) for i in range(1, cfg["h_depth"] + 1))  # not vacuous


def test_check_step_catches_a_gradient_in_an_untouched_row():
    """The harness itself: the smallest value in one row the batch did not read is refused."""
    cfg, params, xi, xv, y = tc.case("qr_add")
    ref = tc.reference("qr_add")[0]
    k = f"fm_2nd_embeddings.{cfg['numerical']}.weight"
    row = int(np.flatnonzero(~tc.table_rows(cfg, xi)[k])[0])
    grads = {n: g.astype(np.float32) for n, g in ref[2].items()}
    tc.check_step(cfg, params, xi, xv, ref[0], ref[1], grads, ref)
    grads[k][row, 0] = 1e-12
    with pytest.raises(AssertionError, match="did not touch"):
        tc.check_step(cfg, params, xi, xv, ref[0], ref[1], grads, ref)
