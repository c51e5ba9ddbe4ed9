"""GPU: the small-batch serving forward (include/dfwfm_serve.h, ForwardEngine.forward_small, DeepFMs.small_batch_rows)
against the reference's golden vectors and the oracle: parity at the north-star bar, batch / position / workspace
independence, routing, graph capture, two streams."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden, logit_close, model_kwargs
from oracle import dfwfm_oracle

pytestmark = pytest.mark.gpu

DEEP_GOLDENS = ["deepfwfm_lw", "deepfwfm_fwlw_lw", "deepfwfm_fwlw_nolw", "deepfwfm_embbag", "deepfwfm_qr_mult",
                "deepfwfm_qr_add_fwlw", "deepfwfm_pruned", "deepfwfm_small_mlp", "fm_deep", "tiny_deepfwfm_lw"]


def make_model(cfg, params, device):
    from xsdeepfwfm_deprecated_amd import DeepFMs
    m = DeepFMs(**model_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return m.to(device).eval()


def dev_inputs(xi, xv, device):
    return torch.from_numpy(np.ascontiguousarray(xi)).to(device), torch.from_numpy(np.ascontiguousarray(xv)).to(device)


def small(m, xi, xv, device):
    """eng.forward_small on host arrays, with the engine synced as the module's inference forward syncs it."""
    with torch.no_grad():
        eng = m._sync_inference(device)
        out = eng.forward_small(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run(m, xi, xv, device):
    with torch.no_grad():
        out = m(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def serve_direct(eng, xi_t, xv_t, device, fill=0xFF):
    """One dfwfm_serve_forward through ctypes with a workspace of the caller's making, filled with `fill` bytes."""
    from xsdeepfwfm_deprecated_amd import _lib
    L = _lib.lib()
    B = xi_t.shape[0]
    n = ctypes.c_size_t(0)
    _lib.check(L.dfwfm_serve_workspace_bytes(eng.handle, B, ctypes.byref(n)), "dfwfm_serve_workspace_bytes")
    ws = torch.full((n.value,), fill, dtype=torch.uint8, device=device)
    out = torch.empty(B, dtype=torch.float32, device=device)
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    rc = L.dfwfm_serve_forward(eng.handle, ctypes.c_void_p(xi_t.data_ptr()), xi_t.stride(0),
                               ctypes.c_void_p(xv_t.data_ptr()), xv_t.stride(0), B, ctypes.c_void_p(out.data_ptr()),
                               ctypes.c_void_p(ws.data_ptr()), n.value, st)
    _lib.check(rc, "dfwfm_serve_forward")
    torch.cuda.synchronize()
    return out.cpu().numpy(), n.value


@pytest.mark.parametrize("name", DEEP_GOLDENS)
def test_small_forward_matches_reference(gpu, name):
    cfg, params, xi, xv, y, l32, l64, auc = load_golden(name)
    xi, xv, l32, l64 = xi[:256], xv[:256], l32[:256], l64[:256]
    m = make_model(cfg, params, gpu)
    got = small(m, xi, xv, gpu)
    assert got.dtype == np.float32 and got.shape == l32.shape
    assert logit_close(got, l32) < 1e-5, name
    assert logit_close(got, l64) < 1e-5, name
    # the workspace's previous contents do not matter: a ragged batch (rows of the last tile never written by the
    # gather) in a workspace of 0xFF bytes (NaNs) gives the same bits
    eng = m._sync_inference(gpu)
    xi_t, xv_t = dev_inputs(xi[:250], xv[:250], gpu)
    direct, nbytes = serve_direct(eng, xi_t, xv_t, gpu)
    assert np.array_equal(direct, got[:250])
    F, D, N = cfg["field_size"], cfg["embedding_size"], cfg["deep_nodes"]
    NT, NC0 = -(-N // 16), -(-F * D // 16)
    # deep_emb, first + second, two activation buffers, partials, for 256 rows
    assert nbytes == 4 * 256 * (NC0 * 16 + 1 + 2 * NT * 16 + NT)


@pytest.fixture(scope="module")
def qr_mult(gpu):
    cfg, params, xi, xv, y, l32, l64, auc = load_golden("deepfwfm_qr_mult")
    m = make_model(cfg, params, gpu)
    return m, xi, xv, l32, small(m, xi, xv, gpu)


@pytest.mark.parametrize("B", [1, 2, 15, 16, 17, 37, 100, 255])
def test_small_ragged_batches(gpu, qr_mult, B):
    m, xi, xv, l32, full = qr_mult
    got = small(m, xi[:B], xv[:B], gpu)
    assert logit_close(got, l32[:B]) < 1e-5
    # a row's logit does not depend on its batch-mates, the batch size or its slot in the 16-row tile
    off = small(m, xi[3:3 + B], xv[3:3 + B], gpu)
    assert np.array_equal(full[:B], got) and np.array_equal(full[3:3 + B], off)
    alone = small(m, xi[B - 1:B], xv[B - 1:B], gpu)
    assert np.array_equal(alone, full[B - 1:B])
    assert np.array_equal(small(m, xi[:B], xv[:B], gpu), got)  # and not on the run


def test_small_many_row_tiles(gpu, qr_mult):
    m, xi, xv, l32, full = qr_mult
    idx = (np.arange(1041) * 7) % 256
    got = small(m, xi[idx], xv[idx], gpu)
    assert np.array_equal(got, full[idx])


def _sweep_case(F, num, D, N, H, fwlw, seed):
    """A synthetic DeepFwFM config (small tables) and its params / inputs, for shape sweeps."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = [1] * num + [int(x) for x in 50 + (np.arange(F - num) * 37) % 400]
    cfg = dict(field_size=F, feature_sizes=sizes, embedding_size=D, use_fwfm=1, use_fm=0, use_logit=0,
               use_deep=1, use_lw=1, use_fwlw=int(fwlw), h_depth=H, deep_nodes=N, numerical=num,
               embedding_bag=0, qr_flag=0, qr_operation="mult", qr_collisions=4, qr_threshold=200)
    m = DeepFMs(**model_kwargs(cfg))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    params = synth.synth_state(shapes, F, D, N, True, True, seed=seed)
    xi, xv = synth.synth_inputs(sizes, num, 48, seed=seed)
    return cfg, params, xi, xv


# deep_nodes: whole tiles (400, 256, 512: the widest layer), few tiles (144, 96) and a ragged last tile (340: 22
# tiles, 4 padded neurons); D = 32: 78 layer-1 K chunks (three rounds of a wave's chunks in flight); H = 1: the first
# layer is also the last
@pytest.mark.parametrize("D,N,H,fwlw", [(10, 400, 3, 0), (10, 144, 2, 1), (4, 256, 1, 0), (16, 512, 2, 0),
                                        (8, 96, 3, 1), (32, 400, 1, 0), (10, 340, 2, 0)])
def test_small_shape_sweep_matches_oracle(gpu, D, N, H, fwlw):
    cfg, params, xi, xv = _sweep_case(39, 13, D, N, H, fwlw, seed=D * 1000 + N + H)
    m = make_model(cfg, params, gpu)
    got = small(m, xi, xv, gpu)
    ref = dfwfm_oracle.forward(cfg, params, xi, xv)
    assert logit_close(got, ref) < 1e-5


@pytest.mark.parametrize("F,num,D,N,H", [(64, 16, 10, 256, 5), (20, 0, 8, 128, 2), (39, 39, 4, 64, 1)])
def test_small_extreme_shapes_match_oracle(gpu, F, num, D, N, H):
    """The limits of the layout: 64 fields, no numerical field, only numerical fields (no Xi at all), five hidden
    layers."""
    cfg, params, xi, xv = _sweep_case(F, num, D, N, H, 0, seed=F + num + D + N + H)
    m = make_model(cfg, params, gpu)
    got = small(m, xi, xv, gpu)
    ref = dfwfm_oracle.forward(cfg, params, xi, xv)
    assert logit_close(got, ref) < 1e-5


def test_small_serving_copy_gives_equal_bits(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    outs = []
    for pack in (True, False):
        m = make_model(cfg, params, gpu)
        m.pack_tables = pack
        outs.append(small(m, xi[:100], xv[:100], gpu))
    assert np.array_equal(outs[0], outs[1])


def test_small_agrees_with_forward(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_fwlw_lw")
    m = make_model(cfg, params, gpu)
    assert logit_close(small(m, xi, xv, gpu), run(m, xi, xv, gpu)) < 1e-5


@pytest.mark.parametrize("bad", [-1, "n"])
def test_small_index_out_of_range_raises(gpu, bad):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    m = make_model(cfg, params, gpu)
    m.small_batch_rows = 16
    x = xi[:8].copy()
    x[5, 3] = cfg["feature_sizes"][13 + 3] if bad == "n" else -1
    with pytest.raises(IndexError):
        run(m, x, xv[:8], gpu)
    # the flag is sticky only until read: a clean batch afterwards passes
    got = run(m, xi[:8], xv[:8], gpu)
    assert np.array_equal(got, small(m, xi[:8], xv[:8], gpu))


def test_small_routing(gpu):
    from xsdeepfwfm_deprecated_amd import DfwfmError
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    m = make_model(cfg, params, gpu)
    assert m.small_batch_rows == 0

    def eng_forward(n):  # the parent path: the engine's default forward, whatever the switch says
        with torch.no_grad():
            eng = m._sync_inference(gpu)
            keep, eng.small_rows = eng.small_rows, 0
            out = eng.forward(*dev_inputs(xi[:n], xv[:n], gpu)).cpu().numpy()
            eng.small_rows = keep
        return out

    for n in (1, 64, 65):  # off: the module's output is the parent path's, bit for bit
        assert np.array_equal(run(m, xi[:n], xv[:n], gpu), eng_forward(n))
    m.small_batch_rows = 64
    s64 = small(m, xi[:64], xv[:64], gpu)
    assert np.array_equal(run(m, xi[:64], xv[:64], gpu), s64)
    assert np.array_equal(run(m, xi[:65], xv[:65], gpu), eng_forward(65))
    # predict_proba goes through the module's forward: the small path's logits under the device's sigmoid
    assert np.array_equal(m.predict_proba(xi[:64], xv[:64]),
                          torch.sigmoid(torch.from_numpy(s64).to(gpu)).cpu().numpy())
    assert run(m, xi[:0], xv[:0], gpu).shape == (0,)
    m.small_batch_rows = 0
    assert np.array_equal(run(m, xi[:64], xv[:64], gpu), eng_forward(64))

    # a model without a deep tower ignores the switch; a direct forward_small on it is refused
    cfg2, params2, xi2, xv2, *_ = load_golden("fwfm_nolw")
    mf = make_model(cfg2, params2, gpu)
    ref = run(mf, xi2[:32], xv2[:32], gpu)
    mf.small_batch_rows = 64
    assert np.array_equal(run(mf, xi2[:32], xv2[:32], gpu), ref)
    with pytest.raises(DfwfmError, match="deep tower"):
        small(mf, xi2[:32], xv2[:32], gpu)


def test_small_boundary_errors(gpu):
    """Workspace too small or misaligned: invalid argument with the needed size in the message; batch 0: OK."""
    from xsdeepfwfm_deprecated_amd import _lib
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_small_mlp")
    m = make_model(cfg, params, gpu)
    with torch.no_grad():
        eng = m._sync_inference(gpu)
    L = _lib.lib()
    xi_t, xv_t = dev_inputs(xi[:5], xv[:5], gpu)
    n = ctypes.c_size_t(0)
    assert L.dfwfm_serve_workspace_bytes(eng.handle, 5, ctypes.byref(n)) == 0
    ws = torch.empty(n.value + 16, dtype=torch.uint8, device=gpu)
    out = torch.empty(5, dtype=torch.float32, device=gpu)
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)

    def call(batch, ws_ptr, ws_bytes, out_ptr=out.data_ptr()):
        return L.dfwfm_serve_forward(eng.handle, ctypes.c_void_p(xi_t.data_ptr()), xi_t.stride(0),
                                     ctypes.c_void_p(xv_t.data_ptr()), xv_t.stride(0), batch,
                                     ctypes.c_void_p(out_ptr), ctypes.c_void_p(ws_ptr), ws_bytes, st)

    assert call(5, ws.data_ptr(), n.value - 1) == -1
    assert str(n.value).encode() in L.dfwfm_last_error()
    assert call(5, ws.data_ptr() + 4, n.value) == -1
    assert b"aligned" in L.dfwfm_last_error()
    assert call(5, None, n.value) == -1
    assert call(5, ws.data_ptr(), n.value, None) == -1
    assert call(0, None, 0) == 0
    assert call(5, ws.data_ptr(), n.value) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), small(m, xi[:5], xv[:5], gpu))


def test_small_graph_capture(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_embbag")
    m = make_model(cfg, params, gpu)
    eager = small(m, xi[:64], xv[:64], gpu)
    with torch.no_grad():
        eng = m._sync_inference(gpu)
        xi_s, xv_s = dev_inputs(xi[:17], xv[:17], gpu)
        xi_o, xv_o = dev_inputs(xi[40:57], xv[40:57], gpu)
        out = torch.empty(17, dtype=torch.float32, device=gpu)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            eng.forward_small(xi_s, xv_s, out)
        g.replay()
        torch.cuda.synchronize()
        first = out.cpu().numpy()
        xi_s.copy_(xi_o)
        xv_s.copy_(xv_o)
        g.replay()
        torch.cuda.synchronize()
        second = out.cpu().numpy()
    assert np.array_equal(first, eager[:17]) and np.array_equal(second, eager[40:57])


def test_small_two_streams(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_qr_add_fwlw")
    m = make_model(cfg, params, gpu)
    serial = small(m, xi, xv, gpu)
    with torch.no_grad():
        eng = m._sync_inference(gpu)
        a_in = dev_inputs(xi[:37], xv[:37], gpu)
        b_in = dev_inputs(xi[100:201], xv[100:201], gpu)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        outs = []
        for _ in range(4):  # calls in flight on both streams, each with its own workspace
            with torch.cuda.stream(s1):
                oa = eng.forward_small(*a_in)
            with torch.cuda.stream(s2):
                ob = eng.forward_small(*b_in)
            outs.append((oa, ob))
        torch.cuda.synchronize()
    for oa, ob in outs:
        assert np.array_equal(oa.cpu().numpy(), serial[:37]) and np.array_equal(ob.cpu().numpy(), serial[100:201])


def test_small_weight_update_is_picked_up(gpu):
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    m = make_model(cfg, params, gpu)
    m.small_batch_rows = 64
    xi, xv = xi[:64], xv[:64]
    run(m, xi, xv, gpu)
    with torch.no_grad():
        m.net_1_linear_2.weight.mul_(-1.0)
    p2 = dict(params)
    p2["net_1_linear_2.weight"] = -params["net_1_linear_2.weight"]
    got = run(m, xi, xv, gpu)  # the module re-syncs; the small path reads the same re-packed fragments
    assert logit_close(got, dfwfm_oracle.forward(cfg, p2, xi, xv)) < 1e-5
    assert np.array_equal(got, small(m, xi, xv, gpu))
