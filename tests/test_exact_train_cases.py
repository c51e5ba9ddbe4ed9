"""CPU: the exact-arithmetic witness of the training step (tests/exact_train_cases.py) stands on its own -- the
certificate holds on every case, float32 arithmetic alone (oracle/torch_port on PyTorch's CPU kernels, the batch
forwards and reversed) returns the float64 reference's bits, no case is degenerate, every listed slip of the reference
changes a gradient bit -- and the host kernels (libdfwfm_cpu.so) return those bits too, at 1 and at 4 threads.
tests/test_gpu_exact_train.py holds every HIP route to the same reference."""
import numpy as np
import pytest
import torch

import exact_train_cases as xc
import train_cases as tc
from test_cpu_kernel import cpu_model

NAMES = list(xc.all_cases())
# models with a part nobody reads: the parameter exists, the forward ignores it and its gradient is exactly zero
UNUSED = {"fwlw_lw-37": ("fm_1st_embeddings",)}


def _assert_bits(what, got_logits, got_grads, case):
    z, g = xc.ref32(case)
    assert np.array_equal(np.asarray(got_logits, np.float32), z), (what, "logits")
    assert set(got_grads) == set(g), what
    for k in g:
        got = got_grads[k]
        got = np.zeros_like(g[k]) if got is None else np.asarray(got, np.float32)
        assert np.array_equal(got, g[k]), (what, k, int(np.sum(got != g[k])), "elements differ")


@pytest.mark.parametrize("name", NAMES)
def test_certificate_holds(name):
    """bound / quantum < 2^24 on the logits and on every gradient tensor (the saturated case: on p - lr g and on the
    loss sum too)."""
    case = xc.all_cases()[name]
    cert = xc.saturated_certificate(xc.saturated()) if name == "sat-128" else xc.certificate(case)
    worst = max(cert, key=cert.get)
    grad = max((k for k in cert if k != "logits"), key=cert.get)
    print(f"{name}: certificate, logits {cert['logits']:.3g}, worst gradient {cert[grad]:.3g} ({grad}), worst "
          f"{cert[worst]:.3g} ({worst}); limit 2^24 = {xc.LIMIT:.3g}; bounds: logits {xc.bounds(case)['logits']:.3g}")
    assert all(v < xc.LIMIT for v in cert.values()), {k: v for k, v in cert.items() if v >= xc.LIMIT}


@pytest.mark.parametrize("name", NAMES)
def test_float32_port_returns_the_float64_bits(name):
    case = xc.all_cases()[name]
    _assert_bits(name, *xc.port32(case), case)


@pytest.mark.parametrize("name", NAMES)
def test_float32_port_reversed_batch_returns_the_float64_bits(name):
    case = xc.all_cases()[name]
    _assert_bits(name, *xc.port32(case, reverse=True), case)


@pytest.mark.parametrize("name", NAMES)
def test_no_degenerate_case(name):
    case = xc.all_cases()[name]
    cfg, B = case.cfg, len(case.xi)
    z, g = xc.ref64(case)
    for k, v in g.items():
        if k.startswith(UNUSED.get(name, ("\0",))):
            assert not np.any(v), k
            continue
        assert np.any(v), (k, "gradient identically zero")
    vals = set(np.abs(case.dlogit[case.dlogit != 0]).tolist())
    assert 0.0 in case.dlogit.tolist() and vals and case.dlogit[-1] != 0  # (the last row: a ragged tile's)
    for v in vals:  # each magnitude with both signs
        assert np.any(case.dlogit == v) and np.any(case.dlogit == -v), v
    if cfg["use_deep"]:
        tower = xc.deep_tower64(case)
        for k, v in tower.items():  # the hand-written tower the mutations slip in IS the reference's
            assert np.array_equal(v.reshape(g[k].shape), g[k]), k
        for i, zl in enumerate(_preactivations(case), 1):
            live = (zl > 0).sum(0)  # per neuron: the rows of the batch on which it is live
            assert np.any(live == 0) or np.any((live > 0) & (live < B)), f"layer {i}: no neuron clipped"
            assert np.any(live == B) or np.any((live > 0) & (live < B)), f"layer {i}: no neuron live"
            assert np.any((live > 0) & (live < B)), f"layer {i}: no neuron both clipped and live on the batch"
    if case.masks is not None:
        for i, m in enumerate(case.masks):
            assert bool(m.any()) and not bool(m.all()), f"mask {i}"
    hot = False
    for k, mask in tc.table_rows(cfg, case.xi).items():
        if k not in g:
            continue
        j = int(k.split(".")[1]) - cfg["numerical"]
        c = cfg["qr_collisions"]
        rows = case.xi[:, j] // c if k.endswith("weight_q") else case.xi[:, j] % c if k.endswith("weight_r") \
            else case.xi[:, j]
        counts = np.bincount(rows, minlength=len(mask))
        hot = hot or counts.max() >= B / 2
        assert np.all(g[k][~mask] == 0.0), k
        if k.endswith("weight_r") or len(mask) <= 7:  # every row of a remainder / a tiny table is read, by design
            assert mask.all(), k
            continue
        if name == "hot-4097" and j == 1:
            assert counts.max() == 1  # the field with all-distinct rows
            continue
        assert counts.max() >= 3, (k, "no row read by three samples")
        assert (~mask).any(), (k, "no untouched row")
        assert np.any(counts == 1), (k, "no row read once")
    assert hot or case.xi.shape[1] == 0, "no field with a row read by half the batch"
    if name == "hot-4097":
        assert len(np.unique(case.xi[:, 0])) == 3 and len(np.unique(case.xi[:, 1])) == B


def _preactivations(case):
    """The hidden layers' pre-activations in float64."""
    cfg, P = case.cfg, case.params
    B = len(case.xi)
    m = [np.ones((B, w)) for w in xc.widths(cfg)] if case.masks is None else [2.0 * x.numpy() for x in case.masks]
    h, out = xc._embeddings(case).reshape(B, -1) * m[0], []
    for i in range(1, cfg["h_depth"] + 1):
        zl = h @ P[f"net_1_linear_{i}.weight"].astype(np.float64).T + P[f"net_1_linear_{i}.bias"]
        out.append(zl)
        h = np.maximum(zl, 0.0) * m[i]
    return out


def test_saturated_case_is_saturated():
    sat = xc.saturated()
    z, _ = xc.ref64(sat.case)
    assert len(z) == xc.SAT_B and np.all(np.abs(z) >= xc.SAT_Z)
    dl = sat.case.dlogit
    assert set(np.unique(dl).tolist()) == {-1.0 / xc.SAT_B, 0.0, 1.0 / xc.SAT_B}
    assert np.count_nonzero(dl) * 3 >= xc.SAT_B
    # any float32 formulation of the sigmoid is exactly 0 or 1 there, and the loss has no log term left
    z32 = torch.from_numpy(z.astype(np.float32))
    assert np.array_equal(torch.sigmoid(z32).numpy(), (z > 0).astype(np.float32))
    y = torch.tensor(sat.y)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(z32.double(), y.double(), reduction="sum")
    assert float(loss) == sat.loss_sum
    assert np.array_equal(((torch.sigmoid(z32) - y) / xc.SAT_B).numpy(), dl)
    xc.sgd_ref(sat)  # asserts p - lr g is a float32


MUTATION_CASES = ("base-129", "base-129-drop", "qr_mult-37")
WANTED = {"one sample dropped from a shared table row", "R instead of (R + R^T) / 2",
          "x2 of one dropout layer skipped in the backward", "dropout in the forward only",
          "ReLU mask taken at the previous layer's width",
          "last row of a ragged tile dropped from one dW", "remainder-table half of a QR mult gradient dropped"}


def test_every_mutation_changes_a_gradient_bit():
    seen = set()
    for name in MUTATION_CASES:
        case = xc.all_cases()[name]
        _, g = xc.ref64(case)
        for what, mut in xc.mutations(case).items():
            changed = xc.differs(mut, g)
            print(f"{name}: {what}: {len(changed)} tensors differ, e.g. {changed[:2]}")
            assert changed, (name, what)
            seen.add(what)
    assert seen == WANTED, WANTED - seen


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_host_kernels_return_the_float64_bits(name, threads):
    """A CPU DeepFMs (CpuEngine: dfwfm_cpu_forward / dfwfm_cpu_backward) through out.backward(dlogit)."""
    case = xc.all_cases()[name]
    prev = torch.get_num_threads()
    try:
        torch.set_num_threads(threads)
        params = {k: v.copy() for k, v in case.params.items()}  # (the cases' arrays are read-only)
        m = cpu_model(case.cfg, params, is_deep_dropout=case.masks is not None).train()
        torch.manual_seed(99)  # train_forward then draws case.seed (train_cases.dropout_seed)
        out = m(torch.tensor(case.xi), torch.tensor(case.xv))
        out.backward(torch.tensor(case.dlogit))
    finally:
        torch.set_num_threads(prev)
    grads = {k: (None if p.grad is None else p.grad.detach().numpy()) for k, p in m.named_parameters()}
    _assert_bits(f"{name}, {threads} threads", out.detach().numpy(), grads, case)
