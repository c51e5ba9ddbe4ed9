"""GPU: the one-launch bf16 forward and its batch sets (include/dfwfm_bf16_fused.h, ForwardEngine.forward_bf16_fused /
forward_bf16_batches, DeepFMs.bf16_fused).  The yardstick is exact: the contract of include/dfwfm_bf16.h fixes every
sum's order, so every logit must be the per-layer path's (forward_bf16) bit for bit -- on the goldens, the shape sweep,
the exact case, every row-tile form, any batch size and row position, batch sets, a captured graph and two streams."""
import ctypes

import numpy as np
import pytest
import torch

import bf16_emul
from bf16_emul import assert_conditions
from conftest import load_golden, model_kwargs
from oracle import dfwfm_oracle

pytestmark = pytest.mark.gpu

UNSUPPORTED, STATE = -2, -4


def make_model(cfg, params, device):
    from xsdeepfwfm_deprecated_amd import DeepFMs
    m = DeepFMs(**model_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    return m.to(device).eval()


def dev_inputs(xi, xv, device):
    return torch.from_numpy(np.ascontiguousarray(xi)).to(device), torch.from_numpy(np.ascontiguousarray(xv)).to(device)


def bf16_engine(m, device):
    """The module's engine synced as its inference forward syncs it, with the bf16 weight copy in place."""
    eng = m._sync_inference(device)
    eng.sync_bf16(True)
    return eng


def layered(m, xi, xv, device):
    """eng.forward_bf16 (the per-layer path: the yardstick) on host arrays."""
    with torch.no_grad():
        out = bf16_engine(m, device).forward_bf16(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def fused(m, xi, xv, device):
    """eng.forward_bf16_fused on host arrays."""
    with torch.no_grad():
        out = bf16_engine(m, device).forward_bf16_fused(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run(m, xi, xv, device):
    with torch.no_grad():
        out = m(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def fused_rc(eng, xi_t, xv_t, out, device):
    """The status of one dfwfm_bf16_fused_forward through ctypes."""
    from xsdeepfwfm_deprecated_amd import _lib
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    rc = _lib.lib().dfwfm_bf16_fused_forward(eng.handle, ctypes.c_void_p(xi_t.data_ptr()), xi_t.stride(0),
                                             ctypes.c_void_p(xv_t.data_ptr()), xv_t.stride(0), xi_t.shape[0],
                                             ctypes.c_void_p(out.data_ptr()), st)
    torch.cuda.synchronize()
    return rc


def in_supported_set(cfg):
    return cfg["embedding_size"] == 10 and cfg["field_size"] <= 48 and cfg["deep_nodes"] <= 512


def check_case(cfg, params, xi, xv, device, what):
    """Fused == per-layer bits on a supported shape; else the C call is refused and the module keeps the per-layer
    path.  Returns the fused logits, or None."""
    m = make_model(cfg, params, device)
    want = layered(m, xi, xv, device)
    with torch.no_grad():
        eng = bf16_engine(m, device)
        sup = eng.bf16_fused_supported()
    if in_supported_set(cfg):
        assert sup, what  # so the test cannot pass by skipping
    if sup:
        got = fused(m, xi, xv, device)
        assert got.dtype == np.float32 and np.array_equal(got, want), what
        return got
    from xsdeepfwfm_deprecated_amd import _lib
    xi_t, xv_t = dev_inputs(xi, xv, device)
    out = torch.zeros(xi.shape[0], dtype=torch.float32, device=device)
    assert fused_rc(eng, xi_t, xv_t, out, device) == UNSUPPORTED, what
    assert b"not supported" in _lib.lib().dfwfm_last_error()
    m.mlp_dtype, m.bf16_fused = "bf16", True
    assert np.array_equal(run(m, xi, xv, device), want), what
    assert m._engine.bf16 and not m._engine.bf16_fused
    return None


# -- 1. equal bits with the per-layer path -----------------------------------------------------------------------
@pytest.mark.parametrize("name", bf16_emul.DEEP_GOLDENS)
def test_fused_equals_the_per_layer_path_on_goldens(gpu, name):
    cfg, params, xi, xv, y, r, e = bf16_emul.golden_case(name)
    got = check_case(cfg, params, xi, xv, gpu, name)
    if got is not None:
        assert_conditions(got, e, r, name)


@pytest.mark.parametrize("i", range(len(bf16_emul.SWEEP)))
def test_fused_equals_the_per_layer_path_on_the_sweep(gpu, i):
    cfg, params, xi, xv, r, e = bf16_emul.sweep_ref(i)
    assert xi.shape[0] == 96
    check_case(cfg, params, xi, xv, gpu, bf16_emul.SWEEP[i])


def test_the_sweep_covers_the_fused_kernels_edges():
    """(no device needed) N = 400, 144 (half-padded last K step, fwlw), 340 (ragged last tile), 100 (4 padded neurons,
    H = 4) are in the supported set, and one shape of each unsupported kind is in the sweep."""
    sup = [(N, H, fwlw) for F, num, D, N, H, fwlw, _ in bf16_emul.SWEEP if D == 10 and F <= 48 and N <= 512]
    assert {(400, 3, 0), (144, 2, 1), (340, 2, 0), (100, 4, 0)} <= set(sup)
    assert any(D != 10 for _, _, D, *_ in bf16_emul.SWEEP) and any(F > 48 and D == 10 for F, _, D, *_ in bf16_emul.SWEEP)


# -- 2. the exact case -------------------------------------------------------------------------------------------
def test_fused_exact_case_is_bit_exact(gpu):
    """No tolerance: with every rounding a no-op and every sum exact, any K-index, tile or padding mix-up shows."""
    cfg, params, xi, xv = bf16_emul.exact_case()
    ref = dfwfm_oracle.forward(cfg, params, xi, xv).astype(np.float32)
    m = make_model(cfg, params, gpu)
    assert np.array_equal(fused(m, xi, xv, gpu), ref)
    assert np.array_equal(fused(m, xi[41:42], xv[41:42], gpu), ref[41:42])
    assert np.array_equal(fused(m, xi[:33], xv[:33], gpu), ref[:33])  # one more than a 32-row tile


# -- 3. the row-tile forms ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def criteo(gpu):
    cfg, params, xi, xv, r, e = bf16_emul.sweep_ref(0)
    m = make_model(cfg, params, gpu)
    return m, xi, xv, layered(m, xi, xv, gpu)


def test_fused_row_tiles_give_equal_bits(gpu, criteo, monkeypatch):
    """16, 32 and 64 rows per workgroup, each forced (DFWFM_DIAG bf16rows=): whole tiles and ragged ones."""
    m, xi, xv, full = criteo
    for rows in (16, 32, 64):
        monkeypatch.setenv("DFWFM_DIAG", f"bf16rows={rows}")
        assert np.array_equal(fused(m, xi, xv, gpu), full), rows
        assert np.array_equal(fused(m, xi[:70], xv[:70], gpu), full[:70]), rows
    # unforced, the tile is chosen from the rows in the grid: either side of one 16-row workgroup per CU
    monkeypatch.delenv("DFWFM_DIAG")
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    for B in (16 * cus, 16 * cus + 17):
        idx = (np.arange(B) * 7) % 96
        assert np.array_equal(fused(m, xi[idx], xv[idx], gpu), full[idx]), B


@pytest.mark.parametrize("name", ["deepfwfm_qr_mult", "deepfwfm_embbag", "deepfwfm_fwlw_nolw"])
def test_fused_row_tiles_on_other_tables_and_first_orders(gpu, monkeypatch, name):
    """The wider tiles' gather (QR operands, EmbeddingBag tables, the fwlw first order) against the per-layer path."""
    cfg, params, xi, xv, *_ = bf16_emul.golden_case(name)
    m = make_model(cfg, params, gpu)
    want = layered(m, xi[:100], xv[:100], gpu)
    for rows in (32, 64):
        monkeypatch.setenv("DFWFM_DIAG", f"bf16rows={rows}")
        assert np.array_equal(fused(m, xi[:100], xv[:100], gpu), want), rows


# -- 4. independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 65, 96])
def test_fused_rows_do_not_depend_on_the_batch(gpu, criteo, B):
    m, xi, xv, full = criteo
    assert np.array_equal(fused(m, xi[:B], xv[:B], gpu), full[:B])
    n = min(B, 93)
    assert np.array_equal(fused(m, xi[3:3 + n], xv[3:3 + n], gpu), full[3:3 + n])  # the same rows, other positions
    idx = np.arange(B)[::-1].copy()
    assert np.array_equal(fused(m, xi[idx], xv[idx], gpu), full[idx])


def test_fused_nan_stays_in_its_row(gpu, criteo):
    m, xi, xv, full = criteo
    xv2 = xv[:40].copy()
    xv2[17, 2] = np.nan
    got = fused(m, xi[:40], xv2, gpu)
    keep = np.arange(40) != 17
    assert np.isnan(got[17]) and np.array_equal(got[keep], full[:40][keep]) and np.isfinite(full).all()


# -- 5. batch sets -----------------------------------------------------------------------------------------------
def set_rows(i, n):
    return (i * 7 + np.arange(40)) % n


@pytest.mark.parametrize("nb", [1, 2, 5, 35])
def test_fused_batch_sets(gpu, criteo, nb):
    """Batches of 40 rows (no multiple of any tile); 35 batches are two launches.  Each batch equals its own
    forward_bf16."""
    m, xi, xv, full = criteo
    with torch.no_grad():
        eng = bf16_engine(m, gpu)
        batches = [dev_inputs(xi[set_rows(i, 96)], xv[set_rows(i, 96)], gpu) for i in range(nb)]
        outs = [torch.zeros(40, dtype=torch.float32, device=gpu) for _ in range(nb)]
        assert eng.forward_bf16_batches(batches, outs) is outs
    torch.cuda.synchronize()
    for i in range(nb):
        assert np.array_equal(outs[i].cpu().numpy(), full[set_rows(i, 96)]), i


def test_fused_batch_sets_strided_inputs(gpu, criteo):
    m, xi, xv, full = criteo
    ncat, num = xi.shape[1], xv.shape[1]
    with torch.no_grad():
        eng = bf16_engine(m, gpu)
        batches = []
        for i in range(3):
            wi = torch.full((40, ncat + 5), -7, dtype=torch.int64, device=gpu)
            wv = torch.full((40, num + 3), float("nan"), dtype=torch.float32, device=gpu)
            a, b = dev_inputs(xi[set_rows(i, 96)], xv[set_rows(i, 96)], gpu)
            wi[:, :ncat], wv[:, :num] = a, b
            batches.append((wi[:, :ncat], wv[:, :num]))
        assert batches[0][0].stride(0) == ncat + 5 and batches[0][1].stride(0) == num + 3
        outs = [torch.zeros(40, dtype=torch.float32, device=gpu) for _ in range(3)]
        eng.forward_bf16_batches(batches, outs)
        one = eng.forward_bf16_fused(*batches[1])
    torch.cuda.synchronize()
    for i in range(3):
        assert np.array_equal(outs[i].cpu().numpy(), full[set_rows(i, 96)]), i
    assert np.array_equal(one.cpu().numpy(), full[set_rows(1, 96)])


def test_fused_batch_set_index_out_of_range(gpu, criteo):
    """The bad index sets the sticky flag and reads row 0; every other batch of the set is unchanged."""
    m, xi, xv, full = criteo
    rows = [set_rows(i, 96) for i in range(4)]
    bad = xi[rows[2]].copy()
    bad[11, 3] = 10 ** 9
    zero = xi[rows[2]].copy()
    zero[11, 3] = 0
    with torch.no_grad():
        eng = bf16_engine(m, gpu)
        assert eng.read_error_flag() == 0
        batches = [dev_inputs(bad if i == 2 else xi[rows[i]], xv[rows[i]], gpu) for i in range(4)]
        outs = [torch.zeros(40, dtype=torch.float32, device=gpu) for _ in range(4)]
        eng.forward_bf16_batches(batches, outs)
        assert eng.read_error_flag() & 1
        assert eng.read_error_flag() == 0  # sticky only until read
    want2 = layered(m, zero, xv[rows[2]], gpu)
    for i in range(4):
        assert np.array_equal(outs[i].cpu().numpy(), want2 if i == 2 else full[rows[i]]), i
    assert xi[rows[2]][11, 3] == 0 or want2[11] != full[rows[2]][11]


def test_fused_batch_set_argument_checks(gpu, criteo):
    m, xi, xv, full = criteo
    with torch.no_grad():
        eng = bf16_engine(m, gpu)
        a = dev_inputs(xi[:40], xv[:40], gpu)
        b = dev_inputs(xi[:39], xv[:39], gpu)
        o = [torch.zeros(40, dtype=torch.float32, device=gpu) for _ in range(2)]
        with pytest.raises(ValueError, match="same size"):
            eng.forward_bf16_batches([a, b], o)
        with pytest.raises(ValueError, match="one output per batch"):
            eng.forward_bf16_batches([a, a], o[:1])
        with pytest.raises(ValueError, match="smaller"):
            eng.forward_bf16_batches([a, a], [o[0], o[1][:39]])
        with pytest.raises(ValueError, match="smaller"):
            eng.forward_bf16_fused(*a, o[0][:39])
        assert eng.forward_bf16_batches([], []) == []
        assert eng.forward_bf16_fused(*dev_inputs(xi[:0], xv[:0], gpu)).shape == (0,)


# -- 6. state ----------------------------------------------------------------------------------------------------
def test_fused_state_errors_and_weight_update(gpu):
    from xsdeepfwfm_deprecated_amd import _lib
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    xi, xv = xi[:50], xv[:50]
    m = make_model(cfg, params, gpu)
    xi_t, xv_t = dev_inputs(xi, xv, gpu)
    out = torch.zeros(50, dtype=torch.float32, device=gpu)
    with torch.no_grad():
        eng = m._sync_inference(gpu)  # mlp_dtype f32: no bf16 copy yet
    assert fused_rc(eng, xi_t, xv_t, out, gpu) == STATE
    assert b"pack_bf16" in _lib.lib().dfwfm_last_error()
    before = fused(m, xi, xv, gpu)
    with torch.no_grad():
        m.net_1_linear_2.weight.mul_(-1.0)
        eng = m._sync_engine(gpu)  # dfwfm_model_set_dense, no re-pack
    assert fused_rc(eng, xi_t, xv_t, out, gpu) == STATE
    after = fused(m, xi, xv, gpu)  # sync_bf16: the new weights
    assert not np.array_equal(after, before) and np.array_equal(after, layered(m, xi, xv, gpu))
    assert fused_rc(eng, xi_t, xv_t, out, gpu) == 0 and np.array_equal(out.cpu().numpy(), after)

    # a model without a deep tower
    cfg2, params2, xi2, xv2, *_ = load_golden("fwfm_nolw")
    mf = make_model(cfg2, params2, gpu)
    with torch.no_grad():
        engf = mf._sync_inference(gpu)
    assert not engf.bf16_fused_supported()
    assert fused_rc(engf, *dev_inputs(xi2[:8], xv2[:8], gpu), out, gpu) == UNSUPPORTED
    assert b"deep tower" in _lib.lib().dfwfm_last_error()


# -- 7. graph capture, two streams -------------------------------------------------------------------------------
def test_fused_graph_capture(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_embbag")
    m = make_model(cfg, params, gpu)
    eager = fused(m, xi[:64], xv[:64], gpu)
    with torch.no_grad():
        eng = bf16_engine(m, gpu)
        xi_s, xv_s = dev_inputs(xi[:17], xv[:17], gpu)
        xi_o, xv_o = dev_inputs(xi[40:57], xv[40:57], gpu)
        out = torch.empty(17, dtype=torch.float32, device=gpu)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.forward_bf16_fused(xi_s, xv_s, out)
        g.replay()
        torch.cuda.synchronize()
        first = out.cpu().numpy()
        xi_s.copy_(xi_o)
        xv_s.copy_(xv_o)
        g.replay()
        torch.cuda.synchronize()
        second = out.cpu().numpy()
    assert np.array_equal(first, eager[:17]) and np.array_equal(second, eager[40:57])


def test_fused_two_streams(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_qr_add_fwlw")
    xi, xv = xi[:256], xv[:256]
    m = make_model(cfg, params, gpu)
    serial = fused(m, xi, xv, gpu)
    with torch.no_grad():
        eng = bf16_engine(m, gpu)
        a_in = dev_inputs(xi[:37], xv[:37], gpu)
        b_in = dev_inputs(xi[100:201], xv[100:201], gpu)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        outs = []
        for _ in range(4):  # calls in flight on both streams, back to back
            with torch.cuda.stream(s1):
                oa = eng.forward_bf16_fused(*a_in)
            with torch.cuda.stream(s2):
                ob = eng.forward_bf16_fused(*b_in)
            outs.append((oa, ob))
        torch.cuda.synchronize()
    for oa, ob in outs:
        assert np.array_equal(oa.cpu().numpy(), serial[:37]) and np.array_equal(ob.cpu().numpy(), serial[100:201])


# -- 8. the module -----------------------------------------------------------------------------------------------
def test_fused_module_routing(gpu):
    cfg, params, xi, xv, y, *_ = load_golden("deepfwfm_lw")
    m = make_model(cfg, params, gpu)
    assert m.bf16_fused is False
    want = layered(m, xi[:65], xv[:65], gpu)
    m.bf16_fused = True  # without mlp_dtype = "bf16" the switch does nothing
    f32 = run(m, xi[:65], xv[:65], gpu)
    assert not np.array_equal(f32, want) and not m._engine.bf16_fused
    m.mlp_dtype = "bf16"
    calls = []
    eng = m._sync_inference(gpu)
    one, sets = eng.forward_bf16_fused, eng.forward_bf16_batches
    eng.forward_bf16_fused = lambda *a: calls.append("one") or one(*a)
    eng.forward_bf16_batches = lambda *a: calls.append("set") or sets(*a)
    assert np.array_equal(run(m, xi[:65], xv[:65], gpu), want) and calls == ["one"]

    # eval_by_batch: three full batches as one batch set, the ragged tail through the fused call
    n = 3 * 8192 + 5
    idx = np.arange(n) % xi.shape[0]
    Xi, Xv, Y = xi[idx], xv[idx], y[idx].astype(np.float32)
    del calls[:]
    got = m.eval_by_batch(Xi, Xv, Y, n)
    assert calls == ["set", "one"]
    m.bf16_fused = False
    del calls[:]
    assert m.eval_by_batch(Xi, Xv, Y, n) == got and calls == []
    m.bf16_fused = True
    with torch.no_grad():
        logits = torch.empty(n, dtype=torch.float32, device=gpu)
        Xi_d, Xv_d = dev_inputs(Xi, Xv, gpu)
        sets([(Xi_d[i * 8192:(i + 1) * 8192], Xv_d[i * 8192:(i + 1) * 8192]) for i in range(3)],
             [logits[i * 8192:(i + 1) * 8192] for i in range(3)])
        one(Xi_d[3 * 8192:], Xv_d[3 * 8192:], logits[3 * 8192:])
        ref = bf16_engine(m, gpu).forward_bf16(Xi_d, Xv_d)
    torch.cuda.synchronize()
    assert np.array_equal(logits.cpu().numpy(), ref.cpu().numpy())
