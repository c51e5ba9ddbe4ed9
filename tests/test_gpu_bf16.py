"""GPU: the inference forward with a bf16 deep tower (include/dfwfm_bf16.h, ForwardEngine.forward_bf16,
DeepFMs.mlp_dtype) against the numpy statement of its contract (tests/bf16_emul.py), the reference's golden vectors
and the oracle: the contract's bounds, an exact case, batch / position / workspace independence, NaN containment,
routing, boundary errors, graph capture, two streams."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_emul
from bf16_emul import assert_conditions
from conftest import load_golden, model_kwargs
from oracle import dfwfm_oracle

pytestmark = pytest.mark.gpu


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


def bf16(m, xi, xv, device):
    """eng.forward_bf16 on host arrays."""
    with torch.no_grad():
        out = bf16_engine(m, device).forward_bf16(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run(m, xi, xv, device):
    with torch.no_grad():
        out = m(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bf16_direct(eng, xi_t, xv_t, device, fill=0xFF):
    """One dfwfm_bf16_forward through ctypes with a workspace of the caller's making, filled with `fill` bytes."""
    from xsdeepfwfm_deprecated_amd import _lib
    L = _lib.lib()
    B = xi_t.shape[0]
    n = ctypes.c_size_t(0)
    _lib.check(L.dfwfm_bf16_workspace_bytes(eng.handle, B, ctypes.byref(n)), "dfwfm_bf16_workspace_bytes")
    ws = torch.full((n.value,), fill, dtype=torch.uint8, device=device)
    out = torch.empty(B, dtype=torch.float32, device=device)
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    rc = L.dfwfm_bf16_forward(eng.handle, ctypes.c_void_p(xi_t.data_ptr()), xi_t.stride(0),
                              ctypes.c_void_p(xv_t.data_ptr()), xv_t.stride(0), B, ctypes.c_void_p(out.data_ptr()),
                              ctypes.c_void_p(ws.data_ptr()), n.value, st)
    _lib.check(rc, "dfwfm_bf16_forward")
    torch.cuda.synchronize()
    return out.cpu().numpy(), n.value


# -- 1. goldens ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bf16_emul.DEEP_GOLDENS)
def test_bf16_forward_meets_the_contract_on_goldens(gpu, name):
    """g = kernel, e = the contract with float64 accumulation, r = logits_ref64, errors over max(1, |r|),
    fmt = max |e - r|: 90 % of rows within 1e-5 of e, every row within max(1e-5, fmt) of e and 2 fmt of r.
    tiny_deepfwfm_lw (2000 rows): the AUC of g within 1e-4 of the AUC of e."""
    from sklearn.metrics import roc_auc_score
    cfg, params, xi, xv, y, r, e = bf16_emul.golden_case(name)
    m = make_model(cfg, params, gpu)
    g = bf16(m, xi, xv, gpu)
    assert g.dtype == np.float32 and g.shape == r.shape
    assert_conditions(g, e, r, name)
    Fd, D, N = cfg["field_size"], cfg["embedding_size"], cfg["deep_nodes"]
    NT, NC0 = -(-N // 16), -(-Fd * D // 16)
    n = ctypes.c_size_t(0)
    from xsdeepfwfm_deprecated_amd import _lib
    assert _lib.lib().dfwfm_bf16_workspace_bytes(bf16_engine(m, gpu).handle, 250, ctypes.byref(n)) == 0
    # f32 deep_emb, first + second, partials, two bf16 activation buffers, for 256 rows
    assert n.value == 256 * (4 * (NC0 * 16 + 1 + NT) + 2 * 2 * NT * 16)
    if name == "tiny_deepfwfm_lw":
        auc_g, auc_e = roc_auc_score(y, g.astype(np.float64)), roc_auc_score(y, e)
        print(name, dict(auc_g=auc_g, auc_e=auc_e, auc_ref=load_golden(name)[7]))
        assert abs(auc_g - auc_e) <= 1e-4


# -- 2. the exact case -----------------------------------------------------------------------------------------
def test_bf16_exact_case_is_bit_exact(gpu):
    """No tolerance: with every rounding a no-op and every sum exact, any K-index, tile or padding mix-up shows."""
    cfg, params, xi, xv = bf16_emul.exact_case()
    ref = dfwfm_oracle.forward(cfg, params, xi, xv).astype(np.float32)
    m = make_model(cfg, params, gpu)
    assert m.mlp_dtype == "f32"
    assert np.array_equal(run(m, xi, xv, gpu), ref)  # the fixture holds on the device's f32 path too
    assert np.array_equal(bf16(m, xi, xv, gpu), ref)
    assert np.array_equal(bf16(m, xi[41:42], xv[41:42], gpu), ref[41:42])


# -- 3. the shallow half ---------------------------------------------------------------------------------------
def test_bf16_shallow_half_is_the_f32_gather(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_fwlw_lw")
    xi, xv = xi[:100], xv[:100]
    p2 = dict(params)
    p2["net_1_fc.weight"] = np.zeros_like(params["net_1_fc.weight"])
    m = make_model(cfg, p2, gpu)
    g = bf16(m, xi, xv, gpu)
    with torch.no_grad():
        eng = m._sync_inference(gpu)
        _, fs = eng.forward_gather(*dev_inputs(xi, xv, gpu))
    torch.cuda.synchronize()
    fs = fs.cpu().numpy()
    assert fs.dtype == np.float32
    want = (fs + np.float32(0.0)) + np.float32(p2["bias"][0])
    assert np.array_equal(g, want)


# -- 4. the shape sweep ----------------------------------------------------------------------------------------
# deep_nodes: whole tiles (400, 256, 512: the widest layer), few tiles (144, 96), ragged last tiles (340, 100: 4
# padded neurons), odd tile counts (a K step of 32 half padded: 400, 144, 340, 100); D = 32: 39 layer-0 K steps;
# D = 10: F D = 390, 26 padding columns; H = 1: the first layer is also the last; 64 fields, no numerical field,
# only numerical fields (no Xi at all), five hidden layers
@pytest.mark.parametrize("i", range(len(bf16_emul.SWEEP)))
def test_bf16_shape_sweep_meets_the_contract(gpu, i):
    cfg, params, xi, xv, r, e = bf16_emul.sweep_ref(i)
    assert xi.shape[0] == 96
    m = make_model(cfg, params, gpu)
    assert_conditions(bf16(m, xi, xv, gpu), e, r, bf16_emul.SWEEP[i])


# -- 5. independence -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def qr_mult(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_qr_mult")
    xi, xv = xi[:256], xv[:256]
    m = make_model(cfg, params, gpu)
    return m, xi, xv, bf16(m, xi, xv, gpu)


@pytest.mark.parametrize("B", [1, 2, 15, 16, 17, 33, 63, 64, 65, 100, 255])
def test_bf16_ragged_batches(gpu, qr_mult, B):
    m, xi, xv, full = qr_mult
    got = bf16(m, xi[:B], xv[:B], gpu)
    # a row's logit does not depend on its batch-mates, the batch size or its slot in the tile
    n = min(B, 253)
    off = bf16(m, xi[3:3 + n], xv[3:3 + n], gpu)
    assert np.array_equal(full[:B], got) and np.array_equal(full[3:3 + n], off)
    alone = bf16(m, xi[B - 1:B], xv[B - 1:B], gpu)
    assert np.array_equal(alone, full[B - 1:B])
    assert np.array_equal(bf16(m, xi[:B], xv[:B], gpu), got)  # and not on the run


def test_bf16_many_row_tiles(gpu, qr_mult):
    m, xi, xv, full = qr_mult
    idx = (np.arange(1041) * 7) % 256
    got = bf16(m, xi[idx], xv[idx], gpu)
    assert np.array_equal(got, full[idx])


def test_bf16_tile_shapes_give_equal_bits(gpu, qr_mult, monkeypatch):
    """The layer kernel's form (a wave's tile 16 x 16, 16 x 80 or 32 x 80, the last also with the weights in LDS) is
    chosen from the batch size: the batch sizes on either side of the three thresholds, ragged in the wider tiles,
    and every form forced on one ragged batch."""
    m, xi, xv, full = qr_mult
    cb5 = -(-(-(-m.deep_layers[0] // 16)) // 5)  # column blocks of 5 tiles
    sizes = []
    for rows, waves in ((16, 512), (32, 1024), (32, 4096)):  # rows per wave, waves from which the next form runs
        rb = -(-waves // cb5)
        sizes += [rows * (rb - 1), rows * (rb - 1) + 17]
    for B in sizes:
        idx = (np.arange(B) * 7) % 256
        assert np.array_equal(bf16(m, xi[idx], xv[idx], gpu), full[idx]), B
    for shape in (0, 1, 2, 3):
        monkeypatch.setenv("DFWFM_DIAG", f"bf16tile={shape}")
        assert np.array_equal(bf16(m, xi[:100], xv[:100], gpu), full[:100]), shape
        assert np.array_equal(bf16(m, xi[7:8], xv[7:8], gpu), full[7:8]), shape


def test_bf16_workspace_contents_do_not_matter(gpu, qr_mult):
    """A ragged batch (rows of the last tile never written by the gather) in a workspace of 0xFF bytes (NaNs)."""
    m, xi, xv, full = qr_mult
    with torch.no_grad():
        eng = bf16_engine(m, gpu)
    direct, _ = bf16_direct(eng, *dev_inputs(xi[:250], xv[:250], gpu), gpu)
    assert np.array_equal(direct, full[:250])


def test_bf16_serving_copy_gives_equal_bits(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    outs = []
    for pack in (True, False):
        m = make_model(cfg, params, gpu)
        m.pack_tables = pack
        outs.append(bf16(m, xi[:100], xv[:100], gpu))
    assert np.array_equal(outs[0], outs[1])


# -- 6. NaN containment ----------------------------------------------------------------------------------------
def test_bf16_nan_stays_in_its_row(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    assert cfg["numerical"] > 2
    xi, xv = xi[:40], xv[:40].copy()
    m = make_model(cfg, params, gpu)
    clean = bf16(m, xi, xv, gpu)
    xv[17, 2] = np.nan
    got = bf16(m, xi, xv, gpu)
    assert np.isnan(got[17])
    keep = np.arange(40) != 17
    assert np.array_equal(got[keep], clean[keep]) and np.isfinite(clean).all()


# -- 7. routing ------------------------------------------------------------------------------------------------
def test_bf16_routing(gpu):
    from xsdeepfwfm_deprecated_amd import DfwfmError
    cfg, params, xi, xv, y, *_ = load_golden("deepfwfm_lw")
    m = make_model(cfg, params, gpu)
    assert m.mlp_dtype == "f32"

    def eng_forward(n):  # the parent path: the engine's default forward, whatever the switches say
        with torch.no_grad():
            eng = m._sync_inference(gpu)
            keep, eng.bf16, eng.small_rows = (eng.bf16, eng.small_rows), False, 0
            out = eng.forward(*dev_inputs(xi[:n], xv[:n], gpu)).cpu().numpy()
            eng.bf16, eng.small_rows = keep
        return out

    parent = {n: eng_forward(n) for n in (1, 8, 64, 65)}
    for n in (1, 64, 65):  # off: the module's output is the parent path's, bit for bit
        assert np.array_equal(run(m, xi[:n], xv[:n], gpu), parent[n])
    b65 = bf16(m, xi[:65], xv[:65], gpu)
    assert not np.array_equal(b65, parent[65])  # another path, not the same sums
    m.mlp_dtype = "bf16"
    assert np.array_equal(run(m, xi[:65], xv[:65], gpu), b65)
    assert np.array_equal(run(m, xi[:1], xv[:1], gpu), b65[:1])
    # predict_proba goes through the module's forward: the bf16 logits under the device's sigmoid
    assert np.array_equal(m.predict_proba(xi[:65], xv[:65]),
                          torch.sigmoid(torch.from_numpy(b65).to(gpu)).cpu().numpy())
    assert run(m, xi[:0], xv[:0], gpu).shape == (0,)
    # ahead of the small-batch path
    m.small_batch_rows = 64
    assert np.array_equal(run(m, xi[:8], xv[:8], gpu), b65[:8])
    m.small_batch_rows = 0

    # eval_by_batch: one bf16 forward per 8192-row batch (two full batches and a tail), not the f32 batch sets
    n = 2 * 8192 + 5
    idx = np.arange(n) % xi.shape[0]
    Xi, Xv, Y = xi[idx], xv[idx], y[idx].astype(np.float32)
    got = m.eval_by_batch(Xi, Xv, Y, n)
    with torch.no_grad():
        logits = bf16_engine(m, gpu).forward_bf16(*dev_inputs(Xi, Xv, gpu))
        y_d = torch.from_numpy(Y).to(gpu)
        loss = torch.zeros((), dtype=torch.float64, device=gpu)
        for off in range(0, n, 8192):
            end = min(n, off + 8192)
            loss += F.binary_cross_entropy_with_logits(logits[off:end], y_d[off:end]).double() * (end - off)
        from xsdeepfwfm_deprecated_amd import metrics
        dm = metrics.DeviceMetrics(gpu)(logits, y_d)
    assert got == (loss.item() / n, dm["auc"], dm["prauc"], dm["rce"])
    f32_logits = np.concatenate([eng_forward(xi.shape[0])] * (n // xi.shape[0] + 1))[:n]
    assert not np.array_equal(logits.cpu().numpy(), f32_logits)

    # a grad-enabled forward stays the f32 training forward
    # (eval mode: no dropout, so two training forwards give the same bits)
    xi_t, xv_t = dev_inputs(xi[:32], xv[:32], gpu)
    with_switch = m(xi_t, xv_t)
    assert with_switch.requires_grad
    with_switch = with_switch.detach().cpu().numpy()
    m.mlp_dtype = "f32"
    without = m(xi_t, xv_t).detach().cpu().numpy()
    assert np.array_equal(with_switch, without) and not np.array_equal(with_switch, b65[:32])

    # back to f32: the parent bits
    for k in (1, 64, 65):
        assert np.array_equal(run(m, xi[:k], xv[:k], gpu), parent[k])

    m.mlp_dtype = "fp8"
    with pytest.raises(ValueError, match="mlp_dtype"):
        run(m, xi[:8], xv[:8], gpu)
    m.mlp_dtype = "bf16"
    m.sparse_mlp_max_density = 0.5
    with pytest.raises(ValueError, match="sparse_mlp_max_density"):
        run(m, xi[:8], xv[:8], gpu)

    # a model without a deep tower ignores the switch; a direct forward_bf16 on it is refused
    cfg2, params2, xi2, xv2, *_ = load_golden("fwfm_nolw")
    mf = make_model(cfg2, params2, gpu)
    ref = run(mf, xi2[:32], xv2[:32], gpu)
    mf.mlp_dtype = "bf16"
    assert np.array_equal(run(mf, xi2[:32], xv2[:32], gpu), ref)
    with torch.no_grad():
        eng = mf._sync_inference(gpu)
        assert eng.bf16 is False
        with pytest.raises(DfwfmError, match="deep tower"):
            eng.forward_bf16(*dev_inputs(xi2[:32], xv2[:32], gpu))


def test_bf16_cpu_model_is_refused():
    """(no device needed, but the switch is part of the GPU feature's routing)"""
    from xsdeepfwfm_deprecated_amd import DeepFMs, DfwfmError
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_small_mlp")
    m = DeepFMs(**model_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m.eval()
    m.mlp_dtype = "bf16"
    with torch.no_grad(), pytest.raises(DfwfmError, match="HIP"):
        m(torch.from_numpy(xi[:4]), torch.from_numpy(xv[:4]))


# -- 8. boundary errors ----------------------------------------------------------------------------------------
def test_bf16_boundary_errors(gpu):
    """Workspace too small or misaligned: invalid argument with the needed size in the message; batch 0: OK; no
    bf16 copy, or a stale one: the state error."""
    from xsdeepfwfm_deprecated_amd import _lib
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_small_mlp")
    m = make_model(cfg, params, gpu)
    with torch.no_grad():
        eng = m._sync_inference(gpu)  # mlp_dtype f32: no bf16 copy yet
    L = _lib.lib()
    xi_t, xv_t = dev_inputs(xi[:5], xv[:5], gpu)
    n = ctypes.c_size_t(0)
    assert L.dfwfm_bf16_workspace_bytes(eng.handle, 5, ctypes.byref(n)) == 0
    ws = torch.empty(n.value + 16, dtype=torch.uint8, device=gpu)
    out = torch.empty(5, dtype=torch.float32, device=gpu)
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(batch, ws_ptr, ws_bytes, out_ptr=out.data_ptr()):
        return L.dfwfm_bf16_forward(eng.handle, ctypes.c_void_p(xi_t.data_ptr()), xi_t.stride(0),
                                    ctypes.c_void_p(xv_t.data_ptr()), xv_t.stride(0), batch,
                                    ctypes.c_void_p(out_ptr), ctypes.c_void_p(ws_ptr), ws_bytes, st)

    assert call(5, ws.data_ptr(), n.value) == -4  # before dfwfm_model_pack_bf16
    assert b"pack_bf16" in L.dfwfm_last_error()
    assert L.dfwfm_model_pack_bf16(eng.handle, 1, st) == 0
    assert call(5, ws.data_ptr(), n.value - 1) == -1
    assert str(n.value).encode() in L.dfwfm_last_error()
    assert call(5, ws.data_ptr() + 4, n.value) == -1
    assert b"aligned" in L.dfwfm_last_error()
    assert call(5, None, n.value) == -1
    assert call(5, ws.data_ptr(), n.value, None) == -1
    assert call(0, None, 0) == 0
    assert call(5, ws.data_ptr(), n.value) == 0
    torch.cuda.synchronize()
    first = out.cpu().numpy()
    assert np.array_equal(first, bf16(m, xi[:5], xv[:5], gpu))
    # set_dense invalidates the copy until the next pack
    with torch.no_grad():
        m.net_1_linear_1.bias.add_(1.0)
        eng = m._sync_engine(gpu)  # dfwfm_model_set_dense, no re-pack
    assert call(5, ws.data_ptr(), n.value) == -4
    assert L.dfwfm_model_pack_bf16(eng.handle, 0, st) == 0  # dropped: still the state error
    assert call(5, ws.data_ptr(), n.value) == -4
    assert L.dfwfm_model_pack_bf16(eng.handle, 1, st) == 0
    assert call(5, ws.data_ptr(), n.value) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(out.cpu().numpy(), first)


# -- 9. graph capture, two streams -----------------------------------------------------------------------------
def test_bf16_graph_capture(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_embbag")
    m = make_model(cfg, params, gpu)
    eager = bf16(m, xi[:64], xv[:64], gpu)
    with torch.no_grad():
        eng = bf16_engine(m, gpu)
        xi_s, xv_s = dev_inputs(xi[:17], xv[:17], gpu)
        xi_o, xv_o = dev_inputs(xi[40:57], xv[40:57], gpu)
        out = torch.empty(17, dtype=torch.float32, device=gpu)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.forward_bf16(xi_s, xv_s, out)
        g.replay()
        torch.cuda.synchronize()
        first = out.cpu().numpy()
        xi_s.copy_(xi_o)
        xv_s.copy_(xv_o)
        g.replay()
        torch.cuda.synchronize()
        second = out.cpu().numpy()
    assert np.array_equal(first, eager[:17]) and np.array_equal(second, eager[40:57])


def test_bf16_two_streams(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_qr_add_fwlw")
    xi, xv = xi[:256], xv[:256]
    m = make_model(cfg, params, gpu)
    serial = bf16(m, xi, xv, gpu)
    with torch.no_grad():
        eng = bf16_engine(m, gpu)
        a_in = dev_inputs(xi[:37], xv[:37], gpu)
        b_in = dev_inputs(xi[100:201], xv[100:201], gpu)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        outs = []
        for _ in range(4):  # calls in flight on both streams, each with its own workspace
            with torch.cuda.stream(s1):
                oa = eng.forward_bf16(*a_in)
            with torch.cuda.stream(s2):
                ob = eng.forward_bf16(*b_in)
            outs.append((oa, ob))
        torch.cuda.synchronize()
    for oa, ob in outs:
        assert np.array_equal(oa.cpu().numpy(), serial[:37]) and np.array_equal(ob.cpu().numpy(), serial[100:201])


# -- 10. weight update -----------------------------------------------------------------------------------------
def test_bf16_weight_update_is_picked_up(gpu):
    cfg, params, xi, xv, y, l32, l64, _ = load_golden("deepfwfm_lw")
    m = make_model(cfg, params, gpu)
    m.mlp_dtype = "bf16"
    xi, xv = xi[:256], xv[:256]
    before = run(m, xi, xv, gpu)
    with torch.no_grad():
        m.net_1_linear_2.weight.mul_(-1.0)
    p2 = dict(params)
    p2["net_1_linear_2.weight"] = -params["net_1_linear_2.weight"]
    got = run(m, xi, xv, gpu)  # the module re-syncs: set_dense, then the bf16 copy is re-packed
    assert not np.array_equal(got, before)
    assert_conditions(got, bf16_emul.forward(cfg, p2, xi, xv), dfwfm_oracle.forward(cfg, p2, xi, xv), "updated")
    assert np.array_equal(got, bf16(m, xi, xv, gpu))


# -- 11. out-of-range index ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1, "n"])
def test_bf16_index_out_of_range_raises(gpu, bad):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    m = make_model(cfg, params, gpu)
    m.mlp_dtype = "bf16"
    x = xi[:8].copy()
    x[5, 3] = cfg["feature_sizes"][13 + 3] if bad == "n" else -1
    with pytest.raises(IndexError):
        run(m, x, xv[:8], gpu)
    # the flag is sticky only until read: a clean batch afterwards passes
    got = run(m, xi[:8], xv[:8], gpu)
    assert np.array_equal(got, bf16(m, xi[:8], xv[:8], gpu))
