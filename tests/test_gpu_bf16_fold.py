"""GPU: the folded layer 1 of the one-launch bf16 forward (include/dfwfm_bf16_fold.h, ForwardEngine.sync_bf16_fold,
DeepFMs.bf16_fold).  The yardsticks: the exact case bit for bit against the float64 oracle; the goldens and the shape
edges against the folded contract in numpy (bf16_fold_emul) by bf16_emul.assert_conditions, whose bounds come from the
emulation's own distance to the oracle; and equal bits across row tiles, batch sizes, row positions, table forms, batch
sets, a captured graph and two streams."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bf16_emul
import bf16_fold_emul
from bf16_emul import assert_conditions
from conftest import load_golden, model_kwargs
from oracle import dfwfm_oracle

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -4


def make_model(cfg, params, device, fold=True):
    """The module on the device with the bf16 tower's one-launch form asked for, and the fold as given."""
    from xsdeepfwfm_deprecated_amd import DeepFMs
    m = DeepFMs(**model_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    m = m.to(device).eval()
    m.mlp_dtype, m.bf16_fused, m.bf16_fold = "bf16", True, fold
    return m


def dev_inputs(xi, xv, device):
    return torch.from_numpy(np.ascontiguousarray(xi)).to(device), torch.from_numpy(np.ascontiguousarray(xv)).to(device)


def engine(m, device):
    with torch.no_grad():
        return m._sync_inference(device)


def fused(m, xi, xv, device, fold=None):
    """eng.forward_bf16_fused on host arrays, the engine synced as the module's inference forward syncs it (fold: the
    module's switch for this call)."""
    if fold is not None:
        m.bf16_fold = fold
    with torch.no_grad():
        out = engine(m, device).forward_bf16_fused(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run(m, xi, xv, device):
    with torch.no_grad():
        out = m(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def state_of(m):
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}


def fold_rc(eng, enable, device):
    """(status, enabled) of one dfwfm_model_fold_bf16 through ctypes."""
    from xsdeepfwfm_deprecated_amd import _lib
    en = ctypes.c_int32(7)
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    rc = _lib.lib().dfwfm_model_fold_bf16(eng.handle, enable, ctypes.byref(en), st)
    return rc, en.value


def raw_fused(eng, xi_t, xv_t, device):
    """dfwfm_bf16_fused_forward through the engine, nothing synced first: the library's state as it stands."""
    with torch.no_grad():
        out = eng.forward_bf16_fused(xi_t, xv_t)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def supported(cfg):
    return cfg["embedding_size"] == 10 and cfg["field_size"] <= 48 and cfg["deep_nodes"] <= 512


# -- 1. the exact case -------------------------------------------------------------------------------------------
def test_fold_exact_case_is_bit_exact(gpu):
    """No tolerance: with every rounding a no-op and every sum exact, any K-row, Xv-column or padding mix-up shows."""
    cfg, params, xi, xv, ref = bf16_fold_emul.exact_case()
    assert xi.shape[0] == 96
    m = make_model(cfg, params, gpu)
    got = fused(m, xi, xv, gpu)
    assert m._engine._bf16_fold_on is True
    assert got.dtype == np.float32 and np.array_equal(got, ref)
    assert np.array_equal(fused(m, xi[41:42], xv[41:42], gpu), ref[41:42])


# -- 2. the goldens ----------------------------------------------------------------------------------------------
def auc(y, s):
    from xsdeepfwfm_deprecated_amd import metrics
    return float(metrics.roc_auc_score(np.asarray(y), np.asarray(s, dtype=np.float64)))


@pytest.mark.parametrize("name", bf16_emul.DEEP_GOLDENS)
def test_fold_goldens(gpu, name):
    cfg, params, xi, xv, y, r, e = bf16_fold_emul.golden_case(name)
    assert 0 < y.sum() < len(y)
    m = make_model(cfg, params, gpu)
    got = run(m, xi, xv, gpu)
    if not supported(cfg):  # the fused form refuses the shape: asking for the fold changes nothing
        assert not m._engine.bf16_fused and not m._engine._bf16_fold_on
        m.bf16_fold = False
        assert np.array_equal(run(m, xi, xv, gpu), got)
        return
    assert m._engine.bf16_fused and m._engine._bf16_fold_on is True
    assert np.array_equal(fused(m, xi, xv, gpu), got)
    assert_conditions(got, e, r, name)
    a_g, a_e = auc(y, got), auc(y, e)
    print(name, "auc", a_g, a_e, auc(y, r))
    assert abs(a_g - a_e) <= 1e-4
    if name == "deepfwfm_lw":  # the fold is really on: another rounding than the unfolded fused forward's
        assert not np.array_equal(fused(m, xi, xv, gpu, fold=False), got)
        assert m._engine._bf16_fold_on is False


def test_the_goldens_cover_a_refused_shape():
    """(no device needed) one deep golden is outside the fused form's shapes, the others inside."""
    sup = [supported(load_golden(n)[0]) for n in bf16_emul.DEEP_GOLDENS]
    assert not all(sup) and sum(sup) >= 8


# -- 3. shape edges ----------------------------------------------------------------------------------------------
# (F, num, D, N, H, fwlw, seed), 96 rows each
EDGES = {
    "a": (39, 13, 10, 400, 3, 0, 10403),  # the Criteo-39 shape: bf16_emul.SWEEP[0]
    "b": (39, 39, 10, 128, 2, 0, 11),     # no categorical block, 2 K steps
    "c": (20, 0, 10, 128, 2, 0, 12),      # no numerical field: enabled == 0
    "d": (5, 2, 10, 64, 2, 0, 13),        # folded K = 32 exactly: no pad, no shift
    "e": (33, 1, 10, 96, 2, 1, 14),       # no K step saved (11 either way), shift 2
    "f": (39, 13, 10, 400, 1, 0, 15),     # the folded layer is also the last
    "g": (39, 13, 10, 100, 3, 0, 16),     # 7 tiles with padded neurons
    "h": (48, 16, 10, 512, 2, 0, 17),     # the supported limits
}


@functools.lru_cache(maxsize=None)
def edge_ref(key):
    """(cfg, params, xi, xv, ref64, folded emul64) of EDGES[key]; computed once, shared, never modified."""
    cfg, params, xi, xv = bf16_emul.sweep_case(*EDGES[key])
    return cfg, params, xi, xv, dfwfm_oracle.forward(cfg, params, xi, xv), bf16_fold_emul.forward(cfg, params, xi, xv)


def test_the_edges_are_what_they_claim():
    """(no device needed) the folded step counts and shifts the cases are there for."""
    def steps(F, num, D):
        return -(-((F - num) * D + num) // 32), -(-(-(-F * D // 16) * 16) // 32), (-num * D) % 4
    assert steps(39, 13, 10) == (9, 13, 2) and steps(39, 39, 10) == (2, 13, 2) and steps(5, 2, 10) == (1, 2, 0)
    assert (5 - 2) * 10 + 2 == 32
    assert steps(33, 1, 10) == (11, 11, 2) and steps(48, 16, 10) == (11, 15, 0)
    assert EDGES["a"] == bf16_emul.SWEEP[0] and EDGES["g"][3] % 16 != 0 and -(-EDGES["g"][3] // 16) == 7


@pytest.mark.parametrize("key", sorted(EDGES))
def test_fold_shape_edges(gpu, key):
    cfg, params, xi, xv, r, e = edge_ref(key)
    assert xi.shape[0] == 96
    m = make_model(cfg, params, gpu)
    got = fused(m, xi, xv, gpu)
    assert m._engine.bf16_fused
    if cfg["numerical"] == 0:
        assert m._engine._bf16_fold_on is False
        assert np.array_equal(got, fused(m, xi, xv, gpu, fold=False))
    else:
        assert m._engine._bf16_fold_on is True
    assert_conditions(got, e, r, (key, EDGES[key]))
    assert np.array_equal(fused(m, xi[70:87], xv[70:87], gpu), got[70:87])  # 17 rows alone, other positions


# -- 4. equal bits -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def criteo(gpu):
    cfg, params, xi, xv, r, e = edge_ref("a")
    m = make_model(cfg, params, gpu)
    full = fused(m, xi, xv, gpu)
    assert m._engine._bf16_fold_on is True
    return m, xi, xv, full


def test_fold_row_tiles_give_equal_bits(gpu, criteo, monkeypatch):
    """16, 32 and 64 rows per workgroup, each forced (DFWFM_DIAG bf16rows=): whole tiles and ragged ones."""
    m, xi, xv, full = criteo
    for rows in (16, 32, 64):
        monkeypatch.setenv("DFWFM_DIAG", f"bf16rows={rows}")
        assert np.array_equal(fused(m, xi, xv, gpu), full), rows
        assert np.array_equal(fused(m, xi[:70], xv[:70], gpu), full[:70]), rows
    assert m._engine._bf16_fold_on is True


@pytest.mark.parametrize("key", ["b", "e", "h"])
def test_fold_row_tiles_on_the_edges(gpu, monkeypatch, key):
    cfg, params, xi, xv, r, e = edge_ref(key)
    m = make_model(cfg, params, gpu)
    want = fused(m, xi, xv, gpu)
    for rows in (32, 64):
        monkeypatch.setenv("DFWFM_DIAG", f"bf16rows={rows}")
        assert np.array_equal(fused(m, xi[:81], xv[:81], gpu), want[:81]), rows


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 65, 96])
def test_fold_rows_do_not_depend_on_the_batch(gpu, criteo, B):
    m, xi, xv, full = criteo
    assert np.array_equal(fused(m, xi[:B], xv[:B], gpu), full[:B])
    n = min(B, 93)
    assert np.array_equal(fused(m, xi[3:3 + n], xv[3:3 + n], gpu), full[3:3 + n])  # the same rows, other positions
    idx = np.arange(B)[::-1].copy()
    assert np.array_equal(fused(m, xi[idx], xv[idx], gpu), full[idx])


@pytest.mark.parametrize("name", ["deepfwfm_qr_mult", "deepfwfm_embbag", "deepfwfm_fwlw_nolw"])
def test_fold_row_tiles_on_other_tables_and_first_orders(gpu, monkeypatch, name):
    """The wider tiles' gather (QR operands, EmbeddingBag tables, the fwlw first order) with the Xv columns."""
    cfg, params, xi, xv, *_ = bf16_fold_emul.golden_case(name)
    m = make_model(cfg, params, gpu)
    want = fused(m, xi[:100], xv[:100], gpu)
    assert m._engine._bf16_fold_on is True
    for rows in (32, 64):
        monkeypatch.setenv("DFWFM_DIAG", f"bf16rows={rows}")
        assert np.array_equal(fused(m, xi[:100], xv[:100], gpu), want), rows


def test_fold_serving_copy_against_plain_tables(gpu):
    cfg, params, xi, xv, *_ = bf16_fold_emul.golden_case("deepfwfm_lw")
    m = make_model(cfg, params, gpu)
    m.pack_tables = True
    a = fused(m, xi[:100], xv[:100], gpu)
    assert m._engine._packed_on is True and m._engine._bf16_fold_on is True
    m.pack_tables = False
    b = fused(m, xi[:100], xv[:100], gpu)
    assert m._engine._packed_on is False and m._engine._bf16_fold_on is True
    assert np.array_equal(a, b)


# -- 5. batch sets -----------------------------------------------------------------------------------------------
def set_rows(i, n):
    return (i * 7 + np.arange(48)) % n


@pytest.mark.parametrize("nb", [1, 2, 5, 35])
def test_fold_batch_sets(gpu, criteo, nb):
    """Batches of 48 rows; 35 batches are two launches.  Each batch equals its lone call."""
    m, xi, xv, full = criteo
    with torch.no_grad():
        eng = engine(m, gpu)
        assert eng._bf16_fold_on is True
        batches = [dev_inputs(xi[set_rows(i, 96)], xv[set_rows(i, 96)], gpu) for i in range(nb)]
        outs = [torch.zeros(48, dtype=torch.float32, device=gpu) for _ in range(nb)]
        assert eng.forward_bf16_batches(batches, outs) is outs
    torch.cuda.synchronize()
    for i in range(nb):
        assert np.array_equal(outs[i].cpu().numpy(), full[set_rows(i, 96)]), i


def test_fold_batch_sets_strided_inputs(gpu, criteo):
    m, xi, xv, full = criteo
    ncat, num = xi.shape[1], xv.shape[1]
    with torch.no_grad():
        eng = engine(m, gpu)
        batches = []
        for i in range(3):
            wi = torch.full((48, ncat + 5), -7, dtype=torch.int64, device=gpu)
            wv = torch.full((48, num + 3), float("nan"), dtype=torch.float32, device=gpu)
            a, b = dev_inputs(xi[set_rows(i, 96)], xv[set_rows(i, 96)], gpu)
            wi[:, :ncat], wv[:, :num] = a, b
            batches.append((wi[:, :ncat], wv[:, :num]))
        assert batches[0][0].stride(0) == ncat + 5 and batches[0][1].stride(0) == num + 3
        outs = [torch.zeros(48, dtype=torch.float32, device=gpu) for _ in range(3)]
        eng.forward_bf16_batches(batches, outs)
        one = eng.forward_bf16_fused(*batches[1])
    torch.cuda.synchronize()
    for i in range(3):
        assert np.array_equal(outs[i].cpu().numpy(), full[set_rows(i, 96)]), i
    assert np.array_equal(one.cpu().numpy(), full[set_rows(1, 96)])


# -- 6. robustness -----------------------------------------------------------------------------------------------
def test_fold_nan_stays_in_its_row(gpu, criteo):
    """A NaN and an Inf in Xv reach their own rows only (zero weights do not cancel a NaN: the pad columns hold zeros
    and the FwFM reads no Xv column), and nothing of them is left for the next call."""
    m, xi, xv, full = criteo
    xv2 = xv[:40].copy()
    xv2[17, 2] = np.nan
    xv2[30, 12] = np.inf
    got = fused(m, xi[:40], xv2, gpu)
    keep = ~np.isin(np.arange(40), (17, 30))
    assert np.isnan(got[17]) and not np.isfinite(got[30])
    assert np.array_equal(got[keep], full[:40][keep]) and np.isfinite(full).all()
    assert np.array_equal(fused(m, xi[:40], xv[:40], gpu), full[:40])
    # the unfolded forward on the same rows: the same rows are non-finite
    off = fused(m, xi[:40], xv2, gpu, fold=False)
    m.bf16_fold = True
    assert np.array_equal(np.isfinite(off), np.isfinite(got))


def test_fold_index_out_of_range(gpu, criteo):
    """The bad index sets the sticky flag and reads row 0; the module raises IndexError."""
    m, xi, xv, full = criteo
    bad = xi[:40].copy()
    bad[11, 3] = 10 ** 9
    zero = xi[:40].copy()
    zero[11, 3] = 0
    eng = engine(m, gpu)
    assert eng.read_error_flag() == 0
    got = fused(m, bad, xv[:40], gpu)
    assert eng.read_error_flag() & 1
    assert eng.read_error_flag() == 0  # sticky only until read
    assert np.array_equal(got, fused(m, zero, xv[:40], gpu))
    assert m.strict_index_check
    with pytest.raises(IndexError):
        run(m, bad, xv[:40], gpu)
    assert np.array_equal(run(m, xi[:40], xv[:40], gpu), full[:40])


def test_fold_batch_set_index_out_of_range(gpu, criteo):
    """In a batch set the bad index sets the sticky flag and reads row 0; every other batch of the set is unchanged."""
    m, xi, xv, full = criteo
    rows = [set_rows(i, 96) for i in range(4)]
    bad = xi[rows[2]].copy()
    bad[11, 3] = 10 ** 9
    zero = xi[rows[2]].copy()
    zero[11, 3] = 0
    with torch.no_grad():
        eng = engine(m, gpu)
        assert eng._bf16_fold_on is True and eng.read_error_flag() == 0
        batches = [dev_inputs(bad if i == 2 else xi[rows[i]], xv[rows[i]], gpu) for i in range(4)]
        outs = [torch.zeros(48, dtype=torch.float32, device=gpu) for _ in range(4)]
        eng.forward_bf16_batches(batches, outs)
        assert eng.read_error_flag() & 1
        assert eng.read_error_flag() == 0  # sticky only until read
    want2 = fused(m, zero, xv[rows[2]], gpu)
    for i in range(4):
        assert np.array_equal(outs[i].cpu().numpy(), want2 if i == 2 else full[rows[i]]), i


def test_fold_graph_capture(gpu):
    """A captured folded forward replayed on new inputs, and the pack itself captured after one eager call."""
    cfg, params, xi, xv, *_ = bf16_fold_emul.golden_case("deepfwfm_embbag")
    m = make_model(cfg, params, gpu)
    eager = fused(m, xi[:64], xv[:64], gpu)
    with torch.no_grad():
        eng = engine(m, gpu)
        assert eng._bf16_fold_on is True
        xi_s, xv_s = dev_inputs(xi[:17], xv[:17], gpu)
        xi_o, xv_o = dev_inputs(xi[40:57], xv[40:57], gpu)
        out = torch.empty(17, dtype=torch.float32, device=gpu)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            assert fold_rc(eng, 1, gpu) == (0, 1)  # no allocation, no synchronisation: the pack is rebuilt in the graph
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


def test_fold_two_streams(gpu):
    cfg, params, xi, xv, *_ = bf16_fold_emul.golden_case("deepfwfm_qr_add_fwlw")
    m = make_model(cfg, params, gpu)
    serial = fused(m, xi, xv, gpu)
    with torch.no_grad():
        eng = engine(m, gpu)
        assert eng._bf16_fold_on is True
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


# -- 7. staleness through the module -----------------------------------------------------------------------------
def check_fresh(m, cfg, xi, xv, gpu, before, what):
    """The module's forward after an update: a fresh model's bits, the conditions against the new parameters, and not
    the logits from before (a stale pack would show)."""
    got = run(m, xi, xv, gpu)
    params = state_of(m)
    fresh = make_model(cfg, params, gpu)
    want = run(fresh, xi, xv, gpu)
    assert fresh._engine._bf16_fold_on is True and m._engine._bf16_fold_on is True
    assert np.array_equal(got, want) and not np.array_equal(got, before), what
    assert_conditions(got, bf16_fold_emul.forward(cfg, params, xi, xv), dfwfm_oracle.forward(cfg, params, xi, xv), what)
    return got


def test_fold_not_stale_after_weight_and_table_edits(gpu):
    cfg, params, xi, xv, *_ = bf16_fold_emul.golden_case("deepfwfm_lw")
    xi, xv = xi[:64], xv[:64]
    m = make_model(cfg, params, gpu)
    before = run(m, xi, xv, gpu)
    with torch.no_grad():
        m.net_1_linear_1.weight[:, :130].mul_(-0.75)  # the numerical fields' columns of W1: only P sees them
    got = check_fresh(m, cfg, xi, xv, gpu, before, "W1")
    with torch.no_grad():
        m.fm_2nd_embeddings[0].weight.mul_(1.5)  # a numerical table's row 0
    check_fresh(m, cfg, xi, xv, gpu, got, "table row 0")


def test_fold_not_stale_after_prune_step(gpu):
    """prune_step's device-side masks (the reference's 0.90 / 0.444 schedule), then a forward."""
    from xsdeepfwfm_deprecated_amd.training import prune_step
    cfg, params, xi, xv, *_ = bf16_fold_emul.golden_case("deepfwfm_lw")
    xi, xv = xi[:64], xv[:64]
    m = make_model(cfg, params, gpu)
    before = run(m, xi, xv, gpu)
    prune_step(m, 0.90, 1, 1, 1, 0.444, 1.0)
    torch.cuda.synchronize()
    check_fresh(m, cfg, xi, xv, gpu, before, "prune_step")


# -- 8. the C ABI ------------------------------------------------------------------------------------------------
def test_fold_is_turned_off_by_set_dense_set_tables_and_pack_bf16(gpu, monkeypatch):
    cfg, params, xi, xv, *_ = bf16_fold_emul.golden_case("deepfwfm_lw")
    xi, xv = xi[:50], xv[:50]
    m = make_model(cfg, params, gpu)
    on = fused(m, xi, xv, gpu)
    off = fused(m, xi, xv, gpu, fold=False)
    assert not np.array_equal(on, off)
    eng = m._engine
    t = dev_inputs(xi, xv, gpu)
    assert fold_rc(eng, 1, gpu) == (0, 1) and np.array_equal(raw_fused(eng, *t, gpu), on)
    assert fold_rc(eng, 0, gpu) == (0, 0) and np.array_equal(raw_fused(eng, *t, gpu), off)
    # dfwfm_model_pack_bf16
    assert fold_rc(eng, 1, gpu) == (0, 1)
    eng._bf16_key = None
    eng.sync_bf16(True)
    assert np.array_equal(raw_fused(eng, *t, gpu), off)
    # dfwfm_model_set_tables (the same tables again)
    assert fold_rc(eng, 1, gpu) == (0, 1) and np.array_equal(raw_fused(eng, *t, gpu), on)
    eng._tables_key = None
    with torch.no_grad():
        m._sync_engine(gpu)
    assert np.array_equal(raw_fused(eng, *t, gpu), off)
    # dfwfm_model_set_dense (the same parameters again): the bf16 copy is stale, and so the fold cannot be built
    assert fold_rc(eng, 1, gpu) == (0, 1)
    eng._dense_key = None
    with torch.no_grad():
        m._sync_engine(gpu)
    from xsdeepfwfm_deprecated_amd import _lib
    rc, en = fold_rc(eng, 1, gpu)
    assert (rc, en) == (STATE, 0) and b"pack_bf16" in _lib.lib().dfwfm_last_error()
    eng.sync_bf16(True)
    assert np.array_equal(raw_fused(eng, *t, gpu), off)
    assert fold_rc(eng, 1, gpu) == (0, 1) and np.array_equal(raw_fused(eng, *t, gpu), on)
    # DFWFM_DIAG bf16fold=0
    monkeypatch.setenv("DFWFM_DIAG", "bf16fold=0")
    assert fold_rc(eng, 1, gpu) == (0, 0)
    assert np.array_equal(raw_fused(eng, *t, gpu), off)


def test_fold_state_and_argument_errors(gpu):
    from xsdeepfwfm_deprecated_amd import _lib
    from xsdeepfwfm_deprecated_amd.engine import ForwardEngine
    cfg, params, xi, xv, *_ = bf16_fold_emul.golden_case("deepfwfm_lw")
    m = make_model(cfg, params, gpu)
    with torch.cuda.device(gpu):
        bare = ForwardEngine(m.engine_config(), gpu)  # neither tables nor dense parameters set
    assert fold_rc(bare, 0, gpu) == (0, 0)
    rc, en = fold_rc(bare, 1, gpu)
    assert (rc, en) == (STATE, 0) and b"set_tables" in _lib.lib().dfwfm_last_error()
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    assert _lib.lib().dfwfm_model_fold_bf16(bare.handle, 1, None, st) == INVALID
    bare.close()
    # a model without a deep tower: DFWFM_OK, never on
    cfg2, params2, *_ = load_golden("fwfm_nolw")
    from xsdeepfwfm_deprecated_amd import DeepFMs
    mf = DeepFMs(**model_kwargs(cfg2))
    mf.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params2.items()})
    mf = mf.to(gpu).eval()
    assert fold_rc(engine(mf, gpu), 1, gpu) == (0, 0)


# -- 9. the module -----------------------------------------------------------------------------------------------
def test_fold_module_routing(gpu):
    cfg, params, xi, xv, y, *_ = load_golden("deepfwfm_lw")
    m = make_model(cfg, params, gpu, fold=False)
    assert type(m)(**model_kwargs(cfg)).bf16_fold is False
    with torch.no_grad():
        eng = engine(m, gpu)
        layered = eng.forward_bf16(*dev_inputs(xi[:65], xv[:65], gpu)).cpu().numpy()  # today's bits
    n = 2 * 8192 + 5
    idx = np.arange(n) % xi.shape[0]
    Xi, Xv, Y = xi[idx], xv[idx], y[idx].astype(np.float32)
    seen = []
    sets = eng.forward_bf16_batches
    eng.forward_bf16_batches = lambda b, o: seen.append(o) or sets(b, o)

    def eval_logits():
        del seen[:]
        res = m.eval_by_batch(Xi, Xv, Y, n)
        assert len(seen) == 1 and len(seen[0]) == 2
        return res, torch.cat(seen[0]).cpu().numpy()

    # off: every path gives the per-layer path's bits
    assert np.array_equal(run(m, xi[:65], xv[:65], gpu), layered) and eng._bf16_fold_on is False
    res_off, lg = eval_logits()
    assert np.array_equal(lg[:65], layered)
    m.bf16_fused = False  # the switch alone does nothing
    m.bf16_fold = True
    assert np.array_equal(run(m, xi[:65], xv[:65], gpu), layered) and eng._bf16_fold_on is False
    m.mlp_dtype, m.bf16_fused = "f32", True
    f32 = run(m, xi[:65], xv[:65], gpu)
    assert not np.array_equal(f32, layered) and not eng.bf16

    # on: forward, predict_proba and eval_by_batch give the same folded bits
    m.mlp_dtype = "bf16"
    want = fused(m, xi[:65], xv[:65], gpu)
    assert eng._bf16_fold_on is True and not np.array_equal(want, layered)
    assert np.array_equal(run(m, xi[:65], xv[:65], gpu), want)
    with torch.no_grad():
        p = torch.sigmoid(torch.from_numpy(want).to(gpu)).cpu().numpy()
    assert np.array_equal(m.predict_proba(xi[:65], xv[:65]), p)
    res_on, lg = eval_logits()
    assert np.array_equal(lg[:65], want) and np.array_equal(lg[2 * xi.shape[0]:2 * xi.shape[0] + 65], want)
    assert np.array_equal(lg[8192:], fused(m, Xi[8192:2 * 8192], Xv[8192:2 * 8192], gpu))
    assert all(np.isfinite(v) for v in res_on) and all(np.isfinite(v) for v in res_off)
    # back off without a manual call
    m.bf16_fold = False
    assert np.array_equal(run(m, xi[:65], xv[:65], gpu), layered)


@pytest.mark.parametrize("i", [3, 8])
def test_asking_for_the_fold_on_an_unsupported_shape_changes_nothing(gpu, i):
    """D = 16 (SWEEP[3]) and F = 64 (SWEEP[8]): the module keeps the per-layer bf16 path, the same bits."""
    cfg, params, xi, xv, r, e = bf16_emul.sweep_ref(i)
    assert not supported(cfg)
    m = make_model(cfg, params, gpu, fold=False)
    want = run(m, xi, xv, gpu)
    m.bf16_fold = True
    assert np.array_equal(run(m, xi, xv, gpu), want)
    assert m._engine.bf16 and not m._engine.bf16_fused and m._engine._bf16_fold_on is False
    assert fold_rc(m._engine, 1, gpu) == (0, 0)
