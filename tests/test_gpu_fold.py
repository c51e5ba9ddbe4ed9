"""GPU: the folded layer 1 of the fused inference forward (include/dfwfm_fold.h): the
numerical fields' share of layer 1 as Xv * P with P = W1 v_f[0] precomputed per weight update -- against the
reference goldens and the float64 oracle at the north-star bar, the same bits in every kernel form, and never a
stale pack after a weight update.  Small tables (the goldens' SMALL_SIZES) with the real tower, 39 x 10 -> 3 x 400,
where the static forms are meant."""
import numpy as np
import pytest
import torch

from conftest import load_golden, logit_close, model_kwargs
from oracle import dfwfm_oracle

pytestmark = pytest.mark.gpu

BAR = 1e-5  # |d| <= 1e-5 * max(1, |ref|), conftest.logit_close


def make_model(cfg, params, device, fold=True):
    from xsdeepfwfm_deprecated_amd import DeepFMs
    m = DeepFMs(**model_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    m = m.to(device).eval()
    m.fold_numerical = fold
    return m


def run(m, xi, xv, device):
    with torch.no_grad():
        out = m(torch.from_numpy(xi).to(device), torch.from_numpy(xv).to(device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def state_of(m):
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


_CRITEO = {}


def criteo_case(seed=55):
    """The Criteo-39 shape (39 fields, 13 numerical, D = 10, 3 x 400) over the goldens' small tables: cfg, params and
    64 input rows, built once and shared (never modified)."""
    if seed not in _CRITEO:
        from xsdeepfwfm_deprecated_amd import DeepFMs, synth
        cfg = dict(load_golden("deepfwfm_lw")[0])
        m = DeepFMs(**model_kwargs(cfg))
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        params = synth.synth_state(shapes, 39, 10, 400, True, True, seed=seed)
        xi, xv = synth.synth_inputs(cfg["feature_sizes"], 13, 64, seed=seed + 1)
        _CRITEO[seed] = (cfg, params, xi, xv)
    return _CRITEO[seed]


GOLDENS = ["deepfwfm_lw", "deepfwfm_fwlw_lw", "deepfwfm_qr_mult", "deepfwfm_pruned", "fm_deep"]


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_folded_and_unfolded(gpu, monkeypatch, name):
    """The reference goldens with the fold on (the default) and under DFWFM_DIAG fold=0, each within the bar of the
    reference's float32 and float64 logits; sync_fold reports on, then off."""
    cfg, params, xi, xv, y, l32, l64, auc = load_golden(name)
    m = make_model(cfg, params, gpu)
    on = run(m, xi, xv, gpu)
    assert m._engine._fold_on is True
    assert logit_close(on, l32) < BAR and logit_close(on, l64) < BAR
    monkeypatch.setenv("DFWFM_DIAG", "fold=0")
    m0 = make_model(cfg, params, gpu)
    off = run(m0, xi, xv, gpu)
    assert m0._engine._fold_on is False
    assert logit_close(off, l32) < BAR and logit_close(off, l64) < BAR
    monkeypatch.delenv("DFWFM_DIAG")
    # the module's own switch turns it off too
    m1 = make_model(cfg, params, gpu, fold=False)
    assert np.array_equal(run(m1, xi, xv, gpu), off)
    assert m1._engine._fold_on is False


def _sweep_case(F, num, D, N, H, seed):
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = [1] * num + [int(x) for x in 50 + (np.arange(F - num) * 37) % 400]
    cfg = dict(field_size=F, feature_sizes=sizes, embedding_size=D, use_fwfm=1, use_fm=0, use_logit=0,
               use_deep=1, use_lw=1, use_fwlw=0, h_depth=H, deep_nodes=N, numerical=num,
               embedding_bag=0, qr_flag=0, qr_operation="mult", qr_collisions=4, qr_threshold=200)
    m = DeepFMs(**model_kwargs(cfg))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    params = synth.synth_state(shapes, F, D, N, True, True, seed=seed)
    xi, xv = synth.synth_inputs(sizes, num, 48, seed=seed)
    return cfg, params, xi, xv


# both residues of num * D mod 4 that an even D allows (2, 0, 2, 0), all fields numerical, none
SWEEP = [(39, 13, 10, 400, 3), (39, 2, 10, 400, 3), (20, 1, 10, 144, 2), (24, 3, 4, 256, 1), (39, 39, 4, 64, 1),
         (20, 0, 8, 128, 2)]


@pytest.mark.parametrize("ng", ["8", "4"])
@pytest.mark.parametrize("F,num,D,N,H", SWEEP)
def test_fold_shape_sweep_matches_oracle(gpu, monkeypatch, ng, F, num, D, N, H):
    """Fold on, B = 48, against the float64 oracle, on the eight- and the four-wave kernels.  Without a numerical
    field the fold reports off and the logits are the unfolded forward's bits."""
    monkeypatch.setenv("DFWFM_DIAG", f"ng={ng}")
    cfg, params, xi, xv = _sweep_case(F, num, D, N, H, seed=F * 7 + num + D + N + H)
    m = make_model(cfg, params, gpu)
    got = run(m, xi, xv, gpu)
    assert m._engine._fold_on is (num > 0)
    ref = dfwfm_oracle.forward(cfg, params, xi, xv)
    err = logit_close(got, ref)
    print(f"fold sweep {(F, num, D, N, H)} ng={ng}: err {err:.3e}")
    assert err < BAR
    if num == 0:
        monkeypatch.setenv("DFWFM_DIAG", f"ng={ng},fold=0")
        assert np.array_equal(run(make_model(cfg, params, gpu), xi, xv, gpu), got)


@pytest.mark.parametrize("B", [1, 31, 33])
def test_fold_same_bits_fwd32_and_fwd_kernel(gpu, monkeypatch, B):
    """Fold on, Criteo-39 shape: the 32-sample-workgroup kernel (r32=1) and fwd_kernel's static form (r32=0) give the
    same bits."""
    cfg, params, xi, xv = criteo_case()
    outs = {}
    for r32 in ("0", "1"):
        monkeypatch.setenv("DFWFM_DIAG", f"r32={r32}")
        m = make_model(cfg, params, gpu)
        outs[r32] = run(m, xi[:B], xv[:B], gpu)
        assert m._engine._fold_on is True
    assert np.array_equal(outs["0"], outs["1"])
    assert logit_close(outs["1"], dfwfm_oracle.forward(cfg, params, xi[:B], xv[:B])) < BAR


@pytest.mark.parametrize("r32", ["0", "1"])
def test_fold_batch_set_and_row_alone(gpu, monkeypatch, r32):
    """Fold on: a 3-batch set of B = 33 equals each batch's own forward, and row 17 of a 33-row batch run alone has
    the bits it has in its batch."""
    from xsdeepfwfm_deprecated_amd import synth
    monkeypatch.setenv("DFWFM_DIAG", f"r32={r32}")
    cfg, params, _, _ = criteo_case()
    m = make_model(cfg, params, gpu)
    eng = m._sync_inference(gpu)
    assert eng._fold_on is True
    host = [synth.synth_inputs(cfg["feature_sizes"], 13, 33, seed=300 + i) for i in range(3)]
    dev = [(torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)) for a, b in host]
    with torch.no_grad():
        outs = [torch.full((33,), float("nan"), device=gpu) for _ in dev]
        eng.forward_batches(dev, outs)
        alone = [eng.forward(a, b) for a, b in dev]
        row = eng.forward(dev[0][0][17:18].contiguous(), dev[0][1][17:18].contiguous())
    torch.cuda.synchronize()
    for o, a in zip(outs, alone):
        assert np.array_equal(o.cpu().numpy(), a.cpu().numpy())
    assert np.array_equal(row.cpu().numpy(), alone[0][17:18].cpu().numpy())


def test_fold_on_against_fold_off(gpu):
    """Same inputs, B = 33: folded and unfolded within the bar of each other and each within the bar of the oracle."""
    cfg, params, xi, xv = criteo_case()
    on = run(make_model(cfg, params, gpu, fold=True), xi[:33], xv[:33], gpu)
    off = run(make_model(cfg, params, gpu, fold=False), xi[:33], xv[:33], gpu)
    ref = dfwfm_oracle.forward(cfg, params, xi[:33], xv[:33])
    print(f"fold on/off {logit_close(on, off):.3e}, on/oracle {logit_close(on, ref):.3e}, "
          f"off/oracle {logit_close(off, ref):.3e}")
    assert logit_close(on, off) < BAR and logit_close(off, on) < BAR
    assert logit_close(on, ref) < BAR and logit_close(off, ref) < BAR


def _fresh_equal(m, cfg, xi, xv, gpu):
    """The module's forward against a fresh model loaded from its current state_dict: the same bits."""
    got = run(m, xi, xv, gpu)
    fresh = make_model(cfg, state_of(m), gpu)
    want = run(fresh, xi, xv, gpu)
    assert fresh._engine._fold_on is True and m._engine._fold_on is True
    return got, want


def test_fold_not_stale_after_table_and_weight_edits(gpu):
    """An in-place edit of a numerical field's table, then of net_1_linear_1.weight: the forward before each update
    has run (a stale pack would show), the forward after equals a fresh model's bit for bit."""
    cfg, params, xi, xv = criteo_case(seed=61)
    m = make_model(cfg, params, gpu)
    before = run(m, xi, xv, gpu)
    with torch.no_grad():
        m.fm_2nd_embeddings[0].weight.mul_(1.5)
    got, want = _fresh_equal(m, cfg, xi, xv, gpu)
    assert np.array_equal(got, want) and not np.array_equal(got, before)
    with torch.no_grad():
        m.net_1_linear_1.weight[:, :130].mul_(-0.75)  # the numerical fields' columns of W1
    got2, want2 = _fresh_equal(m, cfg, xi, xv, gpu)
    assert np.array_equal(got2, want2) and not np.array_equal(got2, got)


def test_fold_not_stale_after_fused_training_steps(gpu):
    """Two FusedTrainStep.step calls (updates inside captured graphs, no version bump), then an eval forward."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, xi, xv = criteo_case(seed=62)
    m = make_model(cfg, params, gpu)
    before = run(m, xi, xv, gpu)
    m.train()
    from xsdeepfwfm_deprecated_amd import synth
    txi, txv = synth.synth_inputs(cfg["feature_sizes"], 13, 256, seed=640)
    t = FusedTrainStep(m, 256, lr=1e-2, weight_decay=0.0)
    dxi, dxv = torch.from_numpy(txi).to(gpu), torch.from_numpy(txv).to(gpu)
    for _ in range(2):
        t.step(dxi, dxv, (torch.arange(256, device=gpu) % 3 == 0).float())
    t.close()
    m.eval()
    got, want = _fresh_equal(m, cfg, xi, xv, gpu)
    assert np.array_equal(got, want) and not np.array_equal(got, before)


def test_fold_not_stale_after_prune_step(gpu):
    """prune_step's device-side masks (the reference's 0.90 / 0.444 schedule), then a forward."""
    from xsdeepfwfm_deprecated_amd.training import prune_step
    cfg, params, xi, xv = criteo_case(seed=63)
    m = make_model(cfg, params, gpu)
    before = run(m, xi, xv, gpu)
    prune_step(m, 0.90, 1, 1, 1, 0.444, 1.0)
    torch.cuda.synchronize()
    got, want = _fresh_equal(m, cfg, xi, xv, gpu)
    assert np.array_equal(got, want) and not np.array_equal(got, before)


def test_fold_special_values(gpu):
    """A row with Xv[b, 3] = NaN, one with +inf, one with every numerical Xv = 0: the NaN row's logit is NaN, and
    every other row has the bits it has without those rows in the batch (zero weights do not cancel a NaN: the pad
    columns hold zeros, and a row's Xv reaches only that row)."""
    cfg, params, xi, xv = criteo_case()
    m = make_model(cfg, params, gpu)
    plain = run(m, xi[:33], xv[:33], gpu)
    sx = xv[:33].copy()
    sx[5, 3] = np.nan
    sx[20, 3] = np.inf
    sx[9, :] = 0.0
    got = run(m, xi[:33], sx, gpu)
    assert m._engine._fold_on is True
    assert np.isnan(got[5])
    keep = np.array([b for b in range(33) if b not in (5, 20, 9)])
    assert np.array_equal(got[keep], plain[keep])
    zero_alone = run(m, xi[9:10], sx[9:10], gpu)
    assert np.array_equal(zero_alone, got[9:10])
    assert logit_close(got[9:10], dfwfm_oracle.forward(cfg, params, xi[9:10], sx[9:10])) < BAR


def test_fold_graph_capture(gpu):
    """The fold is built before the capture; a captured forward replayed twice equals the eager one."""
    cfg, params, xi, xv = criteo_case()
    m = make_model(cfg, params, gpu)
    dxi, dxv = torch.from_numpy(xi[:33]).to(gpu), torch.from_numpy(xv[:33]).to(gpu)
    eng = m._sync_inference(gpu)
    assert eng._fold_on is True
    out = torch.empty(33, device=gpu)
    with torch.no_grad():
        eager = eng.forward(dxi, dxv).clone()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(gpu)
        s.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                eng.forward(dxi, dxv, out)
        torch.cuda.current_stream(gpu).wait_stream(s)
        for _ in range(2):
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), eager.cpu().numpy())
