"""GPU: the dense half of the training step at its edges (cases and references: tests/dense_edge_cases.py; the CPU
leg that shows the references alone meet every bar: tests/test_dense_edge_cases.py; Adam: tests/test_gpu_adam_edges.py).

A. The split-K weight-gradient GEMM (dwr_kernel / dwr_reduce_kernel, dw_sum_kernel) and the final reductions against
   a float64 autograd reference, on batches that split with a ragged last split, empty waves, row counts that are no
   multiple of 4, N and F D that are no multiple of the 80-wide block, and every block grouping of dwr_xcd_plan --
   with the deterministic slices and with the atomic sums, which must also agree with each other, and the
   deterministic ones bit for bit between two runs.
B. bce_grad_kernel and its copy in the per-tile backward (dfwfm_backward_phases_bce) on saturated logits, soft labels,
   a denom that is not n, n around the lane and workgroup edges, and NaN / inf containment.

Worst figures measured on an MI355X (each test prints its own; run with -s).  Gradient error as |g - g64|.max() over
the float64 reference's largest entry: of any tensor / of the MLP weights and biases / of a touched table row (bar
2e-5 each); then the deterministic slices against the atomic sums (bar 2e-6).  Evidence of margin, not thresholds.

    case            slices, tensor / MLP / row      atomic, tensor / MLP / row      slices - atomic
    d4n96-129       4.3e-7 / 1.5e-7 / 7.1e-6        4.3e-7 / 1.5e-7 / 7.1e-6        7.4e-8
    d4n96-131       3.5e-7 / 1.8e-7 / 7.1e-6        3.5e-7 / 1.8e-7 / 7.1e-6        6.5e-8
    d4n96-200       3.4e-7 / 1.3e-7 / 7.0e-6        3.4e-7 / 1.3e-7 / 7.0e-6        1.6e-7
    d4n96-257       3.2e-7 / 1.4e-7 / 7.0e-6        3.2e-7 / 1.2e-7 / 7.0e-6        1.2e-7
    d4n96-500       2.7e-7 / 1.4e-7 / 8.8e-6        2.7e-7 / 1.7e-7 / 8.8e-6        1.6e-7
    d4n96-1000      2.6e-7 / 1.4e-7 / 8.3e-6        3.5e-7 / 1.3e-7 / 8.3e-6        1.8e-7
    d4n96-1100      2.2e-7 / 1.0e-7 / 8.3e-6        2.2e-7 / 1.3e-7 / 8.3e-6        1.7e-7
    d4n96-2617      2.2e-7 / 1.6e-7 / 8.0e-6        3.1e-7 / 1.4e-7 / 7.6e-6        2.0e-7
    d10n96-131      3.6e-7 / 1.8e-7 / 8.3e-6        3.6e-7 / 1.8e-7 / 8.3e-6        9.2e-8
    d10n96-500      2.6e-7 / 2.6e-7 / 8.7e-6        2.3e-7 / 2.1e-7 / 8.7e-6        1.4e-7
    d16n400-131     3.8e-7 / 1.8e-7 / 3.8e-6        3.8e-7 / 1.8e-7 / 3.8e-6        1.1e-7
    d16n400-500     2.6e-7 / 1.4e-7 / 5.3e-6        2.2e-7 / 1.6e-7 / 5.3e-6        1.7e-7
    d16n400-1000    2.5e-7 / 1.8e-7 / 5.4e-6        2.5e-7 / 1.6e-7 / 5.4e-6        2.1e-7
    criteo-257      3.8e-7 / 1.6e-7 / 5.7e-6        3.8e-7 / 2.0e-7 / 5.7e-6        1.4e-7
    criteo-500      2.7e-7 / 2.0e-7 / 5.5e-6        2.9e-7 / 2.0e-7 / 5.5e-6        1.5e-7
    d8n320-1100     2.4e-7 (per tensor only)        2.5e-7                          1.9e-7
    d8n320-1000     2.4e-7 (after 1100)             2.7e-7
    fused d4n96-131 3.5e-7                          3.5e-7
    fused criteo-500 2.7e-7                         2.9e-7

BCE: |dz denom - (sigmoid(z) - y)| <= 1.2e-7 over every n and denom (bar 2^-22 = 2.4e-7); the loss mean within 1.6e-6
of float64's (bar 1e-5); the per-tile backward's dlogit bit-identical to bce_grad_kernel's on every case.

With the kernels broken on purpose (wrong values only) these tests failed: dw_sum_kernel leaving out the last of more
than two splits (the slices legs of every case with three or more splits, 257 rows -- a last split of one row --
included); dwr_block without a partial last k-step (every case whose last split has 1 or 3 rows, both modes, fused
too); sigmoid as expf(x) / (1 + expf(x)) (every n that holds the saturated logits, gradient and backward legs).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dense_edge_cases as dc
import train_cases as tc
from test_gpu_train import _sparse_setup, build, hip_step

pytestmark = pytest.mark.gpu

ids = lambda k: f"{k[0]}-{k[1]}"  # noqa: E731
MODES = pytest.mark.parametrize("det", [True, False], ids=["slices", "atomic"])
ATOMIC_TOL = 2e-6  # test_gpu_train.test_sorted_scatter_bit_identical_and_matches_atomic's bar


# ---------------------------------------------------------------------------------------------------------- A
@functools.lru_cache(maxsize=None)
def _single(gpu, key, det, rep):
    """One hip_step of a case on a fresh model (rep: a second, independent run); shared between the tests."""
    cfg, params, xi, xv, y = dc.dw_case(*key)
    m = build(cfg, params, gpu, is_deep_dropout=False)
    m.deterministic = det
    return hip_step(m, xi, xv, y, gpu, dc.LR, dc.L2)


@functools.lru_cache(maxsize=None)
def _pair(gpu, det, rep):
    """The pair on one model, in order: [(step result, parameters before the step)] for the two batches."""
    steps = []
    m = None
    for key in dc.DW_PAIR:
        cfg, params, xi, xv, y = dc.dw_case(*key)
        if m is None:
            m = build(cfg, params, gpu, is_deep_dropout=False)
            m.deterministic = det
        before = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
        steps.append((hip_step(m, xi, xv, y, gpu, dc.LR, dc.L2), before))
    return steps


def _linear(grads):
    ks = [k for k in grads if k.startswith("net_1_linear_")]
    assert ks and any(k.endswith(".weight") for k in ks) and any(k.endswith(".bias") for k in ks)
    return ks


def _assert_same_bits(a, b, what):
    for k in _linear(a):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (what, k)


def _assert_modes_agree(det_grads, atomic_grads, what):
    worst = 0.0
    for k, a in atomic_grads.items():
        sc = float(np.abs(a).max())
        e = float(np.abs(det_grads[k] - a).max())
        assert e <= ATOMIC_TOL * sc + 1e-12, (what, k, e / max(sc, 1e-30))
        worst = max(worst, e / sc) if sc else worst
    return worst


@MODES
@pytest.mark.parametrize("key", dc.DW_SINGLE, ids=ids)
def test_split_weight_gradients_match_float64(gpu, key, det):
    cfg, params, xi, xv, y = dc.dw_case(*key)
    out, loss, grads, _ = _single(gpu, key, det, 0)
    ref = dc.dw_reference(*key)[0]
    wt, wr, kt, kr = tc.grad_stats(cfg, xi, grads, ref[2])
    wl = max(float(np.abs(grads[k] - ref[2][k]).max() / np.abs(ref[2][k]).max()) for k in _linear(grads))
    print(f"{ids(key)} {'slices' if det else 'atomic'}: gradient error over the tensor's max {wt:.2e} ({kt}), "
          f"MLP weights and biases {wl:.2e}, over the row's max {wr:.2e}")
    dc.check_dw_step(key, cfg, params, xi, xv, out, loss, grads, ref)


@pytest.mark.parametrize("key", dc.DW_SINGLE, ids=ids)
def test_split_slices_bit_identical_and_match_atomic(gpu, key):
    a, b, c = _single(gpu, key, True, 0), _single(gpu, key, True, 1), _single(gpu, key, False, 0)
    _assert_same_bits(a[2], b[2], ids(key))
    w = _assert_modes_agree(a[2], c[2], ids(key))
    print(f"{ids(key)}: slices against atomic sums {w:.2e} of the tensor's max (bar {ATOMIC_TOL:.0e})")


@MODES
def test_smaller_batch_with_more_splits_after_larger(gpu, det):
    """d8n320: 1100 rows (6 splits of 192) size the slices, then 1000 rows round to 8 splits of 128 on the same
    model; the second step against the oracle taken from the parameters after the first."""
    for key, (got, before) in zip(dc.DW_PAIR, _pair(gpu, det, 0)):
        cfg, params, xi, xv, y = dc.dw_case(*key)
        ref = dc.dw_reference(*key)[0] if key == dc.DW_PAIR[0] else tc.ref_step64(cfg, before, xi, xv, y)
        out, loss, grads, _ = got
        wt, wr, kt, _ = tc.grad_stats(cfg, xi, grads, ref[2])
        print(f"{ids(key)} {'slices' if det else 'atomic'}: gradient error over the tensor's max {wt:.2e} ({kt})")
        dc.check_dw_step(key, cfg, before, xi, xv, out, loss, grads, ref)


def test_pair_slices_bit_identical_and_match_atomic(gpu):
    a, b, c = _pair(gpu, True, 0), _pair(gpu, True, 1), _pair(gpu, False, 0)
    for i, key in enumerate(dc.DW_PAIR):
        _assert_same_bits(a[i][0][2], b[i][0][2], ids(key))
    # the two modes start the first step from the same parameters (the second from each mode's own update)
    w = _assert_modes_agree(a[0][0][2], c[0][0][2], ids(dc.DW_PAIR[0]))
    print(f"{ids(dc.DW_PAIR[0])}: slices against atomic sums {w:.2e} of the tensor's max")


@MODES
@pytest.mark.parametrize("key", dc.DW_FUSED, ids=ids)
def test_fused_step_split_weight_gradients(gpu, key, det):
    """FusedTrainStep.step: dwr_reduce_kernel (the GEMM and the final sums in one launch) on a ragged split batch."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, xi, xv, y = dc.dw_case(*key)
    B = len(xi)
    m = build(cfg, params, gpu, is_deep_dropout=False)
    t = FusedTrainStep(m, B, lr=dc.LR, weight_decay=dc.L2, deterministic=det)
    loss_sum = t.step(torch.from_numpy(xi).to(gpu), torch.from_numpy(xv).to(gpu), torch.from_numpy(y).to(gpu))
    torch.cuda.synchronize()
    out = t.out[:B].detach().cpu().numpy().copy()
    loss = float(loss_sum.item()) / B
    grads = {k: (None if p.grad is None else p.grad.detach().cpu().numpy().copy()) for k, p in m.named_parameters()}
    t.close()
    ref = dc.dw_reference(*key)[0]
    wt, wr, kt, _ = tc.grad_stats(cfg, xi, grads, ref[2])
    print(f"{ids(key)} fused {'slices' if det else 'atomic'}: gradient error over the tensor's max {wt:.2e} ({kt})")
    dc.check_dw_step(key, cfg, params, xi, xv, out, loss, grads, ref)


# ---------------------------------------------------------------------------------------------------------- B
SENTINEL = np.float32(-7777.25)
PAD = 67  # floats past n of the over-allocated dlogit


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(gpu):
    return ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


def _bce_grad(gpu, z, y, denom, loss0=0.0):
    """dfwfm_bce_grad on (z, y): (dz of the n elements, the floats past them, loss sum or None for loss0=None)."""
    from xsdeepfwfm_deprecated_amd import _lib
    n = len(z)
    zd, yd = torch.from_numpy(z.copy()).to(gpu), torch.from_numpy(y.copy()).to(gpu)
    dl = torch.full((n + PAD,), float(SENTINEL), device=gpu)
    loss = None if loss0 is None else torch.full((1,), float(loss0), device=gpu)
    _lib.check(_lib.lib().dfwfm_bce_grad(_ptr(zd), _ptr(yd), n, float(denom), _ptr(dl), _ptr(loss), _stream(gpu)),
               "bce")
    torch.cuda.synchronize()
    got = dl.cpu().numpy()
    return got[:n], got[n:], None if loss is None else float(loss.item())


def _check_dz(z, y, denom, dz):
    """The gradient's bars: 2^-22 against float64, and the saturated values exactly.  Returns the worst error."""
    d64, _ = dc.bce_ref64(z, y)
    err = float(np.abs(dz.astype(np.float64) * denom - d64).max())
    assert err <= dc.DZ_TOL, (len(z), denom, err)
    hi, lo, val = dc.bce_saturated32(z, y, denom)
    assert np.array_equal(dz[hi].view(np.int32), val[hi].view(np.int32)), (len(z), denom, "z >= 30")
    assert np.array_equal(dz[lo].view(np.int32), val[lo].view(np.int32)), (len(z), denom, "z <= -90")
    return err


@pytest.mark.parametrize("n", dc.BCE_N)
def test_bce_grad_matches_float64(gpu, n):
    z, y = (a[:n] for a in dc.bce_fixture())
    ref_loss = float(dc.bce_ref64(z, y)[1].sum())
    for denom in (n, 3 * n):
        dz, past, loss = _bce_grad(gpu, z, y, denom)
        err = _check_dz(z, y, denom, dz)
        assert np.all(past == SENTINEL)  # nothing written past n
        assert dc.loss_close(loss, ref_loss, n), (loss, ref_loss)
        # the sum is added onto what *loss_sum holds
        _, _, loss7 = _bce_grad(gpu, z, y, denom, loss0=7.5)
        assert dc.loss_close(loss7 - 7.5, ref_loss, n) and loss7 != loss, (loss7, ref_loss)
        dz0, past0, none = _bce_grad(gpu, z, y, denom, loss0=None)  # loss_sum = NULL
        assert none is None and np.array_equal(dz0.view(np.int32), dz.view(np.int32)) and np.all(past0 == SENTINEL)
        print(f"bce_grad n={n} denom={denom}: |dz denom - (sigmoid - y)| <= {err:.2e} (bar {dc.DZ_TOL:.2e}), "
              f"loss mean off by {abs(loss - ref_loss) / n:.1e}")


BAD = {"nan": np.float32(np.nan), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf)}


def _with_bad(z, bad):
    z = z.copy()
    z[dc.BCE_BAD] = BAD[bad]
    return z


def _check_contained(z, y, denom, bad, dz_clean, dz_bad):
    """One bad logit changes its own dz only: NaN -> NaN, +-inf -> the saturated value."""
    i = dc.BCE_BAD
    keep = np.arange(len(z)) != i
    assert np.array_equal(dz_bad[keep].view(np.int32), dz_clean[keep].view(np.int32)), (len(z), denom, bad)
    if bad == "nan":
        assert np.isnan(dz_bad[i])
    else:
        d = np.float32(denom)
        want = (np.float32(1.0) - y[i]) / d if bad == "+inf" else (np.float32(0.0) - y[i]) / d
        assert dz_bad[i] == np.float32(want), (dz_bad[i], want)


@pytest.mark.parametrize("bad", list(BAD))
@pytest.mark.parametrize("n", [n for n in dc.BCE_N if n > dc.BCE_BAD])
def test_bce_grad_contains_a_bad_logit(gpu, n, bad):
    z, y = (a[:n] for a in dc.bce_fixture())
    for denom in (n, 3 * n):
        clean, _, _ = _bce_grad(gpu, z, y, denom)
        dz, past, loss = _bce_grad(gpu, _with_bad(z, bad), y, denom)
        _check_contained(z, y, denom, bad, clean, dz)
        assert np.all(past == SENTINEL) and not np.isfinite(loss)


@functools.lru_cache(maxsize=None)
def _bce_model(gpu):
    """The model whose backward carries the fixture's logits, and its 4097-row batch (prefixes are taken)."""
    cfg, params, xi, xv, _ = tc.train_case(dc.F, dc.NUM, 4, 96, 2, B=max(dc.BCE_N))
    return build(cfg, params, gpu, is_deep_dropout=False), xi, xv


def _bce_backward(gpu, z, y, denom, split):
    """dfwfm_train_forward on the first n rows, then dfwfm_backward_phases_bce with z in place of the forward's
    logits: fused reductions (DFWFM_BWD_TABLES | MLP_WEIGHTS), or TILES, then MLP_WEIGHTS and SPREAD, whose REDUCE
    forms the loss (test_gpu_train._sparse_step's plumbing).  Returns (dlogit, loss sum)."""
    m, xi, xv = _bce_model(gpu)
    n = len(z)
    fields, dense, views, flat, _lib, _ = _sparse_setup(m, gpu)
    L, eng, st = _lib.lib(), m._sync_engine(gpu), _stream(gpu)
    xi_d, xv_d = torch.from_numpy(xi[:n].reshape(n, -1)).to(gpu), torch.from_numpy(xv[:n]).to(gpu)
    zd, yd = torch.from_numpy(z.copy()).to(gpu), torch.from_numpy(y.copy()).to(gpu)
    out = torch.empty(n, device=gpu)
    eng.train_forward(xi_d, xv_d, out, 0.0, 0)
    dl = torch.full((n + PAD,), float(SENTINEL), device=gpu)
    loss = torch.zeros(1, device=gpu)
    ptr = lambda t: None if t is None else views[id(t)][1].data_ptr()  # noqa: E731
    fg = (_lib.dfwfm_field_grads * len(fields))(*[_lib.dfwfm_field_grads(*[ptr(t) for t in tup]) for tup in fields])
    H = len(dense["lin_w"])
    gW = (ctypes.c_void_p * H)(*[ptr(t) for t in dense["lin_w"]])
    gB = (ctypes.c_void_p * H)(*[ptr(t) for t in dense["lin_b"]])
    grads = _lib.dfwfm_grads(fg, ptr(dense["field_cov"]), ptr(dense["fwfm_lin"]), ptr(dense["fm_1st"]),
                             ptr(dense["bias"]), gW, gB, ptr(dense["fc_w"]))
    first = _lib.BWD_TILES if split else _lib.BWD_TABLES | _lib.BWD_MLP_WEIGHTS
    _lib.check(L.dfwfm_backward_phases_bce(eng.handle, _ptr(zd), _ptr(yd), float(denom), _ptr(dl), _ptr(loss),
                                           ctypes.byref(grads), first, st), "bwd bce")
    if split:
        for bits in (_lib.BWD_MLP_WEIGHTS, _lib.BWD_SPREAD):
            _lib.check(L.dfwfm_backward_phases(eng.handle, _ptr(dl), ctypes.byref(grads), bits, st), "bwd phases")
    torch.cuda.synchronize()
    got = dl.cpu().numpy()
    assert np.all(got[n:] == SENTINEL)
    return got[:n], float(loss.item())


@pytest.mark.parametrize("split", [False, True], ids=["tables", "tiles-spread"])
@pytest.mark.parametrize("n", dc.BCE_N)
def test_backward_bce_matches_bce_grad(gpu, n, split):
    """The per-tile backward's copy of the loss gradient: bce_grad_kernel's dlogit bits, the loss at the same bar."""
    z, y = (a[:n] for a in dc.bce_fixture())
    ref_loss = float(dc.bce_ref64(z, y)[1].sum())
    for denom in (n, 3 * n):
        want, _, _ = _bce_grad(gpu, z, y, denom)
        dz, loss = _bce_backward(gpu, z, y, denom, split)
        assert np.array_equal(dz.view(np.int32), want.view(np.int32)), (n, denom)
        _check_dz(z, y, denom, dz)
        assert dc.loss_close(loss, ref_loss, n), (loss, ref_loss)
        print(f"backward bce n={n} denom={denom} {'tiles-spread' if split else 'tables'}: loss mean off by "
              f"{abs(loss - ref_loss) / n:.1e}")


@pytest.mark.parametrize("split", [False, True], ids=["tables", "tiles-spread"])
@pytest.mark.parametrize("n", [65, 4097])
def test_backward_bce_contains_a_nan_logit(gpu, n, split):
    z, y = (a[:n] for a in dc.bce_fixture())
    clean, _ = _bce_backward(gpu, z, y, n, split)
    dz, loss = _bce_backward(gpu, _with_bad(z, "nan"), y, n, split)
    _check_contained(z, y, n, "nan", clean, dz)
    assert not np.isfinite(loss)
