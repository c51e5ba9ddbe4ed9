"""GPU: the one-launch forward with an int8 deep tower and its batch sets (include/dfwfm_int8.h,
ForwardEngine.forward_int8 / forward_int8_batches, DeepFMs.mlp_dtype = "int8").  The yardstick is the numpy statement of
the contract (tests/int8_emul.py): integer accumulation is exact, so the kernel's only freedom is f32 rounding in the
epilogue and the order of deep's sum -- and on the exact case none at all.  Every row's bits are the same for every row
tile, batch size, row position, batch set, captured graph and stream."""
import ctypes

import numpy as np
import pytest
import torch

import int8_emul
from int8_emul import assert_conditions
from conftest import load_golden, model_kwargs
from oracle import dfwfm_oracle

pytestmark = pytest.mark.gpu

UNSUPPORTED, STATE = -2, -4
GOLDENS_UNSUPPORTED = ["deepfwfm_small_mlp"]  # embedding_size 8
GOLDENS_SUPPORTED = [n for n in int8_emul.DEEP_GOLDENS if n not in GOLDENS_UNSUPPORTED]


def make_model(cfg, params, device):
    from xsdeepfwfm_deprecated_amd import DeepFMs
    m = DeepFMs(**model_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    return m.to(device).eval()


def dev_inputs(xi, xv, device):
    return torch.from_numpy(np.ascontiguousarray(xi)).to(device), torch.from_numpy(np.ascontiguousarray(xv)).to(device)


def int8_engine(m, device):
    """The module's engine synced as its inference forward syncs it, with the int8 pack in place."""
    eng = m._sync_inference(device)
    eng.sync_int8(True)
    return eng


def int8(m, xi, xv, device):
    """eng.forward_int8 on host arrays."""
    with torch.no_grad():
        out = int8_engine(m, device).forward_int8(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run(m, xi, xv, device):
    with torch.no_grad():
        out = m(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def int8_rc(eng, xi_t, xv_t, out, device, batch=None):
    """The status of one dfwfm_int8_forward through ctypes."""
    from xsdeepfwfm_deprecated_amd import _lib
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    rc = _lib.lib().dfwfm_int8_forward(eng.handle, ctypes.c_void_p(xi_t.data_ptr()), xi_t.stride(0),
                                       ctypes.c_void_p(xv_t.data_ptr()), xv_t.stride(0),
                                       xi_t.shape[0] if batch is None else batch, ctypes.c_void_p(out.data_ptr()), st)
    torch.cuda.synchronize()
    return rc


# -- 1. parity with the contract ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS_SUPPORTED)
def test_int8_meets_the_contract_on_goldens(gpu, name):
    cfg, params, xi, xv, y, r, e = int8_emul.golden_case(name)
    assert cfg["embedding_size"] == 10 and cfg["field_size"] <= 48 and cfg["deep_nodes"] <= 512
    assert xi.shape[0] == (2000 if name == "tiny_deepfwfm_lw" else 256)
    m = make_model(cfg, params, gpu)
    with torch.no_grad():
        assert int8_engine(m, gpu).int8_supported(), name  # so the test cannot pass by skipping
    got = int8(m, xi, xv, gpu)
    assert got.dtype == np.float32
    assert_conditions(got, e, r, name)


@pytest.mark.parametrize("i", int8_emul.SWEEP_SUPPORTED)
def test_int8_meets_the_contract_on_the_sweep(gpu, i):
    cfg, params, xi, xv, r, e = int8_emul.sweep_ref(i)
    assert xi.shape[0] == 96
    m = make_model(cfg, params, gpu)
    with torch.no_grad():
        assert int8_engine(m, gpu).int8_supported(), int8_emul.SWEEP[i]
    assert_conditions(int8(m, xi, xv, gpu), e, r, int8_emul.SWEEP[i])


@pytest.mark.parametrize("i", int8_emul.SWEEP_UNSUPPORTED + GOLDENS_UNSUPPORTED)
def test_int8_refuses_unsupported_shapes(gpu, i):
    """embedding_size != 10 or field_size > 48: the C calls refuse, the module raises -- no other path is taken."""
    from xsdeepfwfm_deprecated_amd import DfwfmError, _lib
    if isinstance(i, str):
        cfg, params, xi, xv, *_ = int8_emul.golden_case(i)
    else:
        cfg, params, xi, xv, r, e = int8_emul.sweep_ref(i)
    assert cfg["embedding_size"] != 10 or cfg["field_size"] > 48
    m = make_model(cfg, params, gpu)
    with torch.no_grad():
        eng = m._sync_inference(gpu)
    assert not eng.int8_supported()
    xi_t, xv_t = dev_inputs(xi, xv, gpu)
    out = torch.zeros(xi.shape[0], dtype=torch.float32, device=gpu)
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    assert _lib.lib().dfwfm_model_pack_int8(eng.handle, st) == UNSUPPORTED
    assert int8_rc(eng, xi_t, xv_t, out, gpu) == UNSUPPORTED
    assert b"not supported" in _lib.lib().dfwfm_last_error()
    m.mlp_dtype = "int8"
    with pytest.raises(DfwfmError):
        run(m, xi, xv, gpu)


# -- 2. the exact case -------------------------------------------------------------------------------------------
def test_int8_exact_case_is_bit_exact(gpu):
    """No tolerance: with every quantization exact, any K-index, tile, scale or padding mix-up shows."""
    cfg, params, xi, xv = int8_emul.exact_case()
    ref = dfwfm_oracle.forward(cfg, params, xi, xv).astype(np.float32)
    m = make_model(cfg, params, gpu)
    assert np.array_equal(int8(m, xi, xv, gpu), ref)
    assert np.array_equal(int8(m, xi[41:42], xv[41:42], gpu), ref[41:42])
    assert np.array_equal(int8(m, xi[:33], xv[:33], gpu), ref[:33])  # one more than a 32-row tile


# -- 3. the row-tile forms ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def criteo(gpu):
    cfg, params, xi, xv, r, e = int8_emul.sweep_ref(0)
    m = make_model(cfg, params, gpu)
    return m, xi, xv, int8(m, xi, xv, gpu)


def test_int8_row_tiles_give_equal_bits(gpu, criteo, monkeypatch):
    """16 and 32 rows per workgroup, each forced (DFWFM_DIAG int8rows=): whole tiles and ragged ones."""
    m, xi, xv, full = criteo
    cfg, params, _, _, r, e = int8_emul.sweep_ref(0)
    assert_conditions(full, e, r, "criteo, unforced")
    for rows in (16, 32):
        monkeypatch.setenv("DFWFM_DIAG", f"int8rows={rows}")
        assert np.array_equal(int8(m, xi, xv, gpu), full), rows
        assert np.array_equal(int8(m, xi[:70], xv[:70], gpu), full[:70]), rows
    # unforced, the tile is chosen from the rows in the grid: either side of one 16-row workgroup per CU
    monkeypatch.delenv("DFWFM_DIAG")
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    for B in (16 * cus, 16 * cus + 17):
        idx = (np.arange(B) * 7) % 96
        assert np.array_equal(int8(m, xi[idx], xv[idx], gpu), full[idx]), B


@pytest.mark.parametrize("name", ["deepfwfm_qr_mult", "deepfwfm_embbag", "deepfwfm_fwlw_nolw"])
def test_int8_row_tiles_on_other_tables_and_first_orders(gpu, monkeypatch, name):
    """The gathers of both tiles (QR operands, EmbeddingBag tables, the fwlw first order): equal bits."""
    cfg, params, xi, xv, *_ = int8_emul.golden_case(name)
    m = make_model(cfg, params, gpu)
    want = int8(m, xi[:100], xv[:100], gpu)
    for rows in (16, 32):
        monkeypatch.setenv("DFWFM_DIAG", f"int8rows={rows}")
        assert np.array_equal(int8(m, xi[:100], xv[:100], gpu), want), rows


# -- 4. independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 65, 96])
def test_int8_rows_do_not_depend_on_the_batch(gpu, criteo, B):
    m, xi, xv, full = criteo
    assert np.array_equal(int8(m, xi[:B], xv[:B], gpu), full[:B])
    n = min(B, 93)
    assert np.array_equal(int8(m, xi[3:3 + n], xv[3:3 + n], gpu), full[3:3 + n])  # the same rows, other positions
    idx = np.arange(B)[::-1].copy()
    assert np.array_equal(int8(m, xi[idx], xv[idx], gpu), full[idx])


def test_int8_nan_stays_in_its_row(gpu, criteo):
    m, xi, xv, full = criteo
    xv2 = xv[:40].copy()
    xv2[17, 2] = np.nan
    got = int8(m, xi[:40], xv2, gpu)
    keep = np.arange(40) != 17
    assert np.isnan(got[17]) and np.array_equal(got[keep], full[:40][keep]) and np.isfinite(full).all()


# -- 5. batch sets -----------------------------------------------------------------------------------------------
def set_rows(i, n):
    return (i * 7 + np.arange(40)) % n


@pytest.mark.parametrize("nb", [1, 2, 5, 35])
def test_int8_batch_sets(gpu, criteo, nb):
    """Batches of 40 rows (no multiple of any tile); 35 batches are two launches.  Each batch equals its own
    forward_int8."""
    m, xi, xv, full = criteo
    with torch.no_grad():
        eng = int8_engine(m, gpu)
        batches = [dev_inputs(xi[set_rows(i, 96)], xv[set_rows(i, 96)], gpu) for i in range(nb)]
        outs = [torch.zeros(40, dtype=torch.float32, device=gpu) for _ in range(nb)]
        assert eng.forward_int8_batches(batches, outs) is outs
        one = eng.forward_int8(*batches[nb - 1])
    torch.cuda.synchronize()
    for i in range(nb):
        assert np.array_equal(outs[i].cpu().numpy(), full[set_rows(i, 96)]), i
    assert np.array_equal(one.cpu().numpy(), outs[nb - 1].cpu().numpy())


def test_int8_empty_calls_launch_nothing(gpu, criteo):
    from xsdeepfwfm_deprecated_amd import _lib
    m, xi, xv, full = criteo
    with torch.no_grad():
        eng = int8_engine(m, gpu)
        assert eng.forward_int8_batches([], []) == []
        assert eng.forward_int8(*dev_inputs(xi[:0], xv[:0], gpu)).shape == (0,)
        xi_t, xv_t = dev_inputs(xi[:8], xv[:8], gpu)
        out = torch.full((8,), 7.0, dtype=torch.float32, device=gpu)
        assert int8_rc(eng, xi_t, xv_t, out, gpu, batch=0) == 0
        st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
        assert _lib.lib().dfwfm_int8_forward_batches(eng.handle, 0, None, 0, None, 0, 8, None, st) == 0
        P = ctypes.c_void_p * 1
        assert _lib.lib().dfwfm_int8_forward_batches(eng.handle, 1, P(xi_t.data_ptr()), xi_t.stride(0),
                                                     P(xv_t.data_ptr()), xv_t.stride(0), 0, P(out.data_ptr()), st) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()


# -- 6. state ----------------------------------------------------------------------------------------------------
def test_int8_state_errors_and_weight_update(gpu):
    from xsdeepfwfm_deprecated_amd import _lib
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    xi, xv = xi[:50], xv[:50]
    m = make_model(cfg, params, gpu)
    xi_t, xv_t = dev_inputs(xi, xv, gpu)
    out = torch.zeros(50, dtype=torch.float32, device=gpu)
    with torch.no_grad():
        eng = m._sync_inference(gpu)  # mlp_dtype f32: no int8 pack yet
    assert int8_rc(eng, xi_t, xv_t, out, gpu) == STATE
    assert b"pack_int8" in _lib.lib().dfwfm_last_error()
    before = int8(m, xi, xv, gpu)
    with torch.no_grad():
        m.net_1_linear_2.weight.mul_(-0.75)
        eng = m._sync_engine(gpu)  # dfwfm_model_set_dense, no re-pack
    assert int8_rc(eng, xi_t, xv_t, out, gpu) == STATE
    # a re-sync through the module: the new weights' emulation
    m.mlp_dtype = "int8"
    after = run(m, xi, xv, gpu)
    params2 = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    assert not np.array_equal(after, before)
    assert_conditions(after, int8_emul.forward(cfg, params2, xi, xv), dfwfm_oracle.forward(cfg, params2, xi, xv),
                      "after the weight update")
    assert int8_rc(eng, xi_t, xv_t, out, gpu) == 0 and np.array_equal(out.cpu().numpy(), after)

    # a model without a deep tower
    cfg2, params2, xi2, xv2, *_ = load_golden("fwfm_nolw")
    mf = make_model(cfg2, params2, gpu)
    with torch.no_grad():
        engf = mf._sync_inference(gpu)
    assert not engf.int8_supported()
    assert int8_rc(engf, *dev_inputs(xi2[:8], xv2[:8], gpu), out, gpu) == UNSUPPORTED
    assert b"deep tower" in _lib.lib().dfwfm_last_error()


def test_int8_index_out_of_range(gpu, criteo):
    """The bad index sets the sticky flag and reads row 0; DeepFMs.forward raises IndexError as on the other paths."""
    m, xi, xv, full = criteo
    bad = xi[:40].copy()
    bad[11, 3] = 10 ** 9
    zero = xi[:40].copy()
    zero[11, 3] = 0
    with torch.no_grad():
        eng = int8_engine(m, gpu)
        assert eng.read_error_flag() == 0
        got = eng.forward_int8(*dev_inputs(bad, xv[:40], gpu))
        assert eng.read_error_flag() & 1
        assert eng.read_error_flag() == 0  # sticky only until read
    assert np.array_equal(got.cpu().numpy(), int8(m, zero, xv[:40], gpu))
    m.mlp_dtype = "int8"
    try:
        with pytest.raises(IndexError):
            run(m, bad, xv[:40], gpu)
        assert np.array_equal(run(m, xi[:40], xv[:40], gpu), full[:40])
    finally:
        m.mlp_dtype = "f32"


# -- 7. graph capture, two streams -------------------------------------------------------------------------------
def test_int8_graph_capture(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_embbag")
    m = make_model(cfg, params, gpu)
    eager = int8(m, xi[:64], xv[:64], gpu)
    with torch.no_grad():
        eng = int8_engine(m, gpu)
        xi_s, xv_s = dev_inputs(xi[:17], xv[:17], gpu)
        xi_o, xv_o = dev_inputs(xi[40:57], xv[40:57], gpu)
        out = torch.empty(17, dtype=torch.float32, device=gpu)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.forward_int8(xi_s, xv_s, out)
        g.replay()
        torch.cuda.synchronize()
        first = out.cpu().numpy()
        xi_s.copy_(xi_o)
        xv_s.copy_(xv_o)
        g.replay()
        torch.cuda.synchronize()
        second = out.cpu().numpy()
    assert np.array_equal(first, eager[:17]) and np.array_equal(second, eager[40:57])


def test_int8_two_streams(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_qr_add_fwlw")
    xi, xv = xi[:256], xv[:256]
    m = make_model(cfg, params, gpu)
    serial = int8(m, xi, xv, gpu)
    with torch.no_grad():
        eng = int8_engine(m, gpu)
        a_in = dev_inputs(xi[:37], xv[:37], gpu)
        b_in = dev_inputs(xi[100:201], xv[100:201], gpu)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        outs = []
        for _ in range(4):  # calls in flight on both streams, back to back
            with torch.cuda.stream(s1):
                oa = eng.forward_int8(*a_in)
            with torch.cuda.stream(s2):
                ob = eng.forward_int8(*b_in)
            outs.append((oa, ob))
        torch.cuda.synchronize()
    for oa, ob in outs:
        assert np.array_equal(oa.cpu().numpy(), serial[:37]) and np.array_equal(ob.cpu().numpy(), serial[100:201])


# -- 8. the module -----------------------------------------------------------------------------------------------
def test_int8_module_routing(gpu):
    from xsdeepfwfm_deprecated_amd import DfwfmError
    cfg, params, xi, xv, y, *_ = load_golden("deepfwfm_lw")
    m = make_model(cfg, params, gpu)
    f32 = run(m, xi[:65], xv[:65], gpu)
    want = int8(m, xi[:65], xv[:65], gpu)
    assert not np.array_equal(f32, want)
    m.mlp_dtype = "int8"
    m.bf16_fused = m.bf16_fold = True  # ignored with int8
    calls = []
    eng = m._sync_inference(gpu)
    one, sets = eng.forward_int8, eng.forward_int8_batches
    eng.forward_int8 = lambda *a: calls.append("one") or one(*a)
    eng.forward_int8_batches = lambda *a: calls.append("set") or sets(*a)
    assert np.array_equal(run(m, xi[:65], xv[:65], gpu), want) and calls == ["one"]
    assert m._engine.int8 and not m._engine.bf16

    # eval_by_batch: two full batches as one batch set, the ragged tail through the single call
    n = 2 * 8192 + 5
    idx = np.arange(n) % xi.shape[0]
    Xi, Xv, Y = xi[idx], xv[idx], y[idx].astype(np.float32)
    del calls[:]
    got = m.eval_by_batch(Xi, Xv, Y, n)
    assert calls == ["set", "one"]
    m.eval_batch_sets = False
    del calls[:]
    assert m.eval_by_batch(Xi, Xv, Y, n) == got and calls == ["one"] * 3
    m.eval_batch_sets = True

    # a sparse tower beside int8 is refused; so is an unknown string, as before
    m.sparse_mlp_max_density = 0.5
    with pytest.raises(DfwfmError, match="int8"):
        run(m, xi[:8], xv[:8], gpu)
    m.sparse_mlp_max_density = 0.0
    m.mlp_dtype = "fp8"
    with pytest.raises(ValueError, match="mlp_dtype must be"):
        run(m, xi[:8], xv[:8], gpu)

    # back to f32: the f32 logits bit for bit
    m.mlp_dtype = "f32"
    del calls[:]
    assert np.array_equal(run(m, xi[:65], xv[:65], gpu), f32) and calls == []


def test_int8_refuses_an_active_fwfm_pair_list(gpu):
    """A pruned field_cov with fwfm_pair_max on builds a pair list; the int8 forward raises rather than take another
    path."""
    from xsdeepfwfm_deprecated_amd import DfwfmError
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    params = dict(params)
    R = np.array(params["field_cov.weight"], dtype=np.float32)
    keep = np.zeros_like(R)
    keep[0, 1] = keep[1, 0] = keep[2, 5] = keep[5, 2] = 1
    params["field_cov.weight"] = R * keep
    m = make_model(cfg, params, gpu)
    m.mlp_dtype = "int8"
    m.fwfm_pair_max = 0
    ok = run(m, xi[:20], xv[:20], gpu)
    assert np.isfinite(ok).all()
    m.fwfm_pair_max = 64
    with torch.no_grad():
        m._sync_inference(gpu)
        on = m._engine.sync_pairs(64)
    assert on  # the pair list is on: the case is the one meant
    with pytest.raises(DfwfmError):
        run(m, xi[:20], xv[:20], gpu)


def test_int8_tiny_golden_auc_through_eval_by_batch(gpu):
    """The AUC of the kernel's logits against the AUC of the emulation's, each pair under one definition of the
    metric: sklearn on the float64 logits, and eval_by_batch's own (metrics.DeviceMetrics: sigmoid in f32 on the
    device, whose ties move the AUC of the SAME 2000 logits by 3.5e-6 -- 0.50833306 against 0.50832960 for the
    emulation itself -- so the two definitions are not compared with each other)."""
    from sklearn.metrics import roc_auc_score
    from xsdeepfwfm_deprecated_amd import metrics
    cfg, params, xi, xv, y, r, e = int8_emul.golden_case("tiny_deepfwfm_lw")
    auc_ref = float(load_golden("tiny_deepfwfm_lw")[7])
    m = make_model(cfg, params, gpu)
    m.mlp_dtype = "int8"
    loss, auc, prauc, rce = m.eval_by_batch(xi, xv, y.astype(np.float32), xi.shape[0])
    g = run(m, xi, xv, gpu)
    auc_g, auc_e = roc_auc_score(y, g.astype(np.float64)), roc_auc_score(y, e)
    e_d = torch.from_numpy(e.astype(np.float32)).to(gpu)
    y_d = torch.from_numpy(y.astype(np.float32)).to(gpu)
    auc_e_dev = metrics.DeviceMetrics(gpu)(e_d, y_d)["auc"]
    print("tiny_deepfwfm_lw AUC:", dict(eval_by_batch=auc, emulation_device_metric=auc_e_dev, kernel_logits=auc_g,
                                        emulation=auc_e, auc_ref=auc_ref))
    assert abs(auc_g - auc_e) <= 1e-6
    assert abs(auc - auc_e_dev) <= 1e-6
    assert abs(auc - auc_ref) <= 1e-4 and abs(auc_g - auc_ref) <= 1e-4
