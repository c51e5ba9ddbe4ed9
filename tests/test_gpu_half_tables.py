"""GPU: the fp16 serving copy of the categorical tables (include/dfwfm_half_tables.h, DeepFMs.table_dtype = "fp16").
The yardstick is exact: half -> float is exact and everything behind the load is the f32 copy's arithmetic, so with
fp16 tables a model's logits are, bit for bit, the logits of the same path on tests/half_tables_ref.rounded_model --
the model whose categorical second-order tables are w.half().float() -- with the f32 copy.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import half_tables_ref
from conftest import golden_names, load_golden, model_kwargs

pytestmark = pytest.mark.gpu

UNSUPPORTED, STATE = -2, -4
MUST_BE_COVERED = ["deepfwfm_lw", "tiny_deepfwfm_lw", "tiny_fwfm_lw"]
NON_QR_GOLDENS = [n for n in golden_names() if "qr" not in n]
SETS = [(3, 33), (2, 256)]


def make_model(cfg, params, device):
    from xsdeepfwfm_deprecated_amd import DeepFMs
    m = DeepFMs(**model_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    return m.to(device).eval()


def dev_inputs(xi, xv, device):
    return torch.from_numpy(np.ascontiguousarray(xi)).to(device), torch.from_numpy(np.ascontiguousarray(xv)).to(device)


def batch_set(xi, xv, nb, B, device):
    """nb batches of B rows cut from the case's rows (wrapping around when it has fewer than nb * B)."""
    n = xi.shape[0]
    return [dev_inputs(xi[(i * B + np.arange(B)) % n], xv[(i * B + np.arange(B)) % n], device) for i in range(nb)]


def lone(m, xi, xv, device):
    with torch.no_grad():
        out = m(*dev_inputs(xi, xv, device))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def as_set(m, call, xi, xv, nb, B, device):
    with torch.no_grad():
        eng = m._sync_inference(device)
        if call == "forward_int8_batches":
            eng.sync_int8(True)
        dev = batch_set(xi, xv, nb, B, device)
        outs = getattr(eng, call)(dev, [torch.full((B,), float("nan"), device=device) for _ in dev])
    torch.cuda.synchronize()
    return torch.stack(outs).cpu().numpy()


def all_paths(m, xi, xv, device):
    """{path: logits} over every forward the fp16 copy composes with, on this module as it is configured (its
    table_dtype); the module's other switches are restored."""
    out = {}
    keep = (m.mlp_dtype, m.bf16_fused, m.bf16_fold)
    try:
        m.mlp_dtype, m.bf16_fused, m.bf16_fold = "f32", False, False
        out["f32 lone"] = lone(m, xi, xv, device)  # (a model without a deep tower: the MLP-free forward)
        for nb, B in SETS:
            out[f"f32 set {nb}x{B}"] = as_set(m, "forward_batches", xi, xv, nb, B, device)
        if m.use_deep:
            with torch.no_grad():
                eng = m._sync_inference(device)
                fused_ok, int8_ok = eng.bf16_fused_supported(), eng.int8_supported()
            if fused_ok:
                for fold in (False, True):
                    m.mlp_dtype, m.bf16_fused, m.bf16_fold = "bf16", True, fold
                    out[f"bf16 fused fold={fold} lone"] = lone(m, xi, xv, device)
                    assert m._engine.bf16_fused
                    for nb, B in SETS:
                        out[f"bf16 fused fold={fold} set {nb}x{B}"] = as_set(m, "forward_bf16_batches", xi, xv, nb, B,
                                                                             device)
            if int8_ok:
                m.mlp_dtype, m.bf16_fused, m.bf16_fold = "int8", False, False
                out["int8 lone"] = lone(m, xi, xv, device)
                for nb, B in SETS:
                    out[f"int8 set {nb}x{B}"] = as_set(m, "forward_int8_batches", xi, xv, nb, B, device)
    finally:
        m.mlp_dtype, m.bf16_fused, m.bf16_fold = keep
    return out


def assert_fp16_is_the_rounded_model(m, xi, xv, device, what):
    """table_dtype = 'fp16' on m == the f32 copy on rounded_model(m), every path, array_equal; and the rounding is
    visible (the rounded model's logits differ from the original's somewhere, so the comparison is not vacuous)."""
    r = half_tables_ref.rounded_model(m)
    r.table_dtype = "f32"
    ref = all_paths(r, xi, xv, device)
    assert r._engine._packed_on and r._engine.serving_copy_bytes() > 0
    m.table_dtype = "fp16"
    got = all_paths(m, xi, xv, device)
    assert m._engine._packed_on
    assert set(got) == set(ref)
    for k in ref:
        assert np.all(np.isfinite(ref[k])), (what, k)
        assert np.array_equal(got[k], ref[k]), (what, k, float(np.abs(got[k] - ref[k]).max()))
    return got, ref


# -- 1. bit identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NON_QR_GOLDENS)
def test_fp16_tables_are_the_rounded_model_on_goldens(gpu, name):
    cfg, params, xi, xv, *_ = load_golden(name)
    xi, xv = xi[:256], xv[:256]
    m = make_model(cfg, params, gpu)
    with torch.no_grad():
        covered = m._sync_inference(gpu)._packed_on
    if name in MUST_BE_COVERED:
        assert covered, name  # so the test cannot pass by doing nothing
    if not covered:
        return  # fwlw without first-order tables, no second order: the refusal test's ground
    plain = lone(m, xi, xv, gpu)
    got, ref = assert_fp16_is_the_rounded_model(m, xi, xv, gpu, name)
    assert len(got) >= (9 if name in MUST_BE_COVERED and cfg["use_deep"] else 3)
    assert not np.array_equal(got["f32 lone"], plain), "the rounding must be visible"


def fwfm_only_case(F, num, D, lw, fm, seed, sizes=None):
    """tests/test_gpu_batches.py::_fwfm_only_case: a model without a deep tower over odd table sizes."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    if sizes is None:
        sizes = [1] * num + [int(x) for x in 7 + (np.arange(F - num) * 389 + seed) % 20000]
    cfg = dict(field_size=F, feature_sizes=sizes, embedding_size=D, use_fwfm=1 - fm, use_fm=fm, use_logit=0,
               use_deep=0, use_lw=lw, use_fwlw=0, h_depth=1, deep_nodes=16, numerical=num, embedding_bag=0,
               qr_flag=0, qr_operation="mult", qr_collisions=4, qr_threshold=200)
    m = DeepFMs(**model_kwargs(cfg))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    params = synth.synth_state(shapes, F, D, 16, True, False, seed=seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return cfg, params, m


@pytest.mark.parametrize("B", [1, 17, 33])
@pytest.mark.parametrize("F,num,D,lw,fm", [(39, 13, 10, 1, 0), (39, 13, 16, 1, 0), (48, 16, 8, 0, 0),
                                           (20, 5, 4, 1, 1), (16, 3, 32, 0, 1)])
def test_fp16_tables_fwfm_only_shapes(gpu, F, num, D, lw, fm, B):
    """Every embedding size the library instantiates (row strides 32, 48 and 80 bytes), FwFM row tiles 1 to 3, FM,
    with and without lw: lone (eight waves) and as a set (four waves)."""
    from xsdeepfwfm_deprecated_amd import synth
    cfg, params, m = fwfm_only_case(F, num, D, lw, fm, seed=F * 100 + D)
    m = m.to(gpu).eval()
    xi, xv = synth.synth_inputs(cfg["feature_sizes"], num, 3 * B, seed=F + D + B)
    r = half_tables_ref.rounded_model(m)
    m.table_dtype = "fp16"
    assert np.array_equal(lone(m, xi[:B], xv[:B], gpu), lone(r, xi[:B], xv[:B], gpu))
    assert np.array_equal(as_set(m, "forward_batches", xi, xv, 3, B, gpu),
                          as_set(r, "forward_batches", xi, xv, 3, B, gpu))
    rows = sum(cfg["feature_sizes"][num:])
    stride = {4: 32, 8: 32, 10: 32, 16: 48, 32: 80}[D]
    assert m._engine.serving_copy_bytes() == rows * stride


@pytest.mark.parametrize("D,N,H", [(8, 64, 2), (10, 100, 1), (16, 400, 3), (10, 400, 3)])
def test_fp16_tables_deep_f32_forms(gpu, D, N, H):
    """The f32 deep forward's forms: generic tile counts and embedding sizes (their own fp16 instantiations), the
    static 3x400 one, folded and unfolded, 16-row lone batches and sets."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = [1] * 13 + [int(x) for x in 50 + (np.arange(26) * 37) % 400]
    cfg = dict(field_size=39, feature_sizes=sizes, embedding_size=D, use_fwfm=1, use_fm=0, use_logit=0, use_deep=1,
               use_lw=1, use_fwlw=0, h_depth=H, deep_nodes=N, numerical=13, embedding_bag=0, qr_flag=0,
               qr_operation="mult", qr_collisions=4, qr_threshold=200)
    m = DeepFMs(**model_kwargs(cfg))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    params = synth.synth_state(shapes, 39, D, N, True, True, seed=D + N)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(gpu).eval()
    xi, xv = synth.synth_inputs(sizes, 13, 99, seed=D)
    for fold in (True, False):
        m.fold_numerical = fold
        m.table_dtype = "f32"
        plain = lone(m, xi, xv, gpu)
        got, _ = assert_fp16_is_the_rounded_model(m, xi, xv, gpu, (D, N, H, fold))
        assert not np.array_equal(got["f32 lone"], plain)


# -- 2. edges ----------------------------------------------------------------------------------------------------
CRITICAL = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1e-6, 3e-8, -0.0, 65504.0, 65519.0, -65519.0, -(1 + 2.0 ** -11)]


def edge_case(gpu, D=10):
    """Tables of 1, 256 and 257 rows (the pack kernel's one-row, full and last partial workgroup) among others,
    seeded with the values where an fp16 rounding can go wrong."""
    sizes = [1, 1, 1] + [1, 256, 257, 2, 255, 513, 300]
    cfg, params, m = fwfm_only_case(10, 3, D, 1, 0, seed=3, sizes=sizes)
    with torch.no_grad():
        for f in range(3, 10):
            w = m.fm_2nd_embeddings[f].weight
            flat = w.view(-1)
            vals = torch.tensor(CRITICAL, dtype=torch.float32)
            flat[:min(len(vals), flat.numel())] = vals[:flat.numel()]   # the first row(s)
            flat[-min(len(vals), flat.numel()):] = vals[:flat.numel()]  # ... and the last, whatever else is there
    return cfg, m.to(gpu).eval(), sizes


def test_fp16_tables_edge_rows_and_critical_values(gpu):
    cfg, m, sizes = edge_case(gpu)
    cat = np.array(sizes[3:], dtype=np.int64)
    rng = np.random.default_rng(5)
    B = 40
    xv = rng.random((B, 3), dtype=np.float32)
    last = np.tile(cat - 1, (B, 1))                      # every index at its table's last row
    first = np.zeros((B, 7), dtype=np.int64)
    mixed = rng.integers(0, cat, size=(B, 7))
    r = half_tables_ref.rounded_model(m)
    m.table_dtype = "fp16"
    for what, xi in (("last", last), ("first", first), ("mixed", mixed)):
        a, b = lone(m, xi, xv, gpu), lone(r, xi, xv, gpu)
        assert np.all(np.isfinite(b)), what
        assert np.array_equal(a, b), what
        assert np.array_equal(as_set(m, "forward_batches", xi, xv, 2, 20, gpu),
                              as_set(r, "forward_batches", xi, xv, 2, 20, gpu)), what
    # the seeded values survive exactly as the cast says: the rounded model is not the original one
    m.table_dtype = "f32"
    assert not np.array_equal(lone(m, last, xv, gpu), lone(r, last, xv, gpu))


def test_fp16_tables_out_of_range_index_clamps_and_raises(gpu):
    cfg, m, sizes = edge_case(gpu)
    cat = np.array(sizes[3:], dtype=np.int64)
    xv = np.full((5, 3), 0.5, dtype=np.float32)
    xi = np.tile(cat - 1, (5, 1))
    bad = xi.copy()
    bad[2, 5] = cat[5]  # one past the last row of the 513-row table
    bad[4, 1] = -1
    clamped = bad.copy()
    clamped[2, 5] = 0
    clamped[4, 1] = 0
    m.table_dtype = "fp16"
    with pytest.raises(IndexError):
        lone(m, bad, xv, gpu)
    m.strict_index_check = False
    got = lone(m, bad, xv, gpu)
    assert m._engine.read_error_flag() != 0
    m.strict_index_check = True
    assert np.array_equal(got, lone(m, clamped, xv, gpu))


# -- 3. overflow -------------------------------------------------------------------------------------------------
def test_fp16_overflow_is_refused_and_the_model_stays_usable(gpu):
    from xsdeepfwfm_deprecated_amd import DfwfmError, _lib
    cfg, m, sizes = edge_case(gpu)
    with torch.no_grad():
        m.fm_2nd_embeddings[5].weight[200, 7] = 70000.0
    cat = np.array(sizes[3:], dtype=np.int64)
    xi = np.tile(np.minimum(cat - 1, 200), (6, 1))
    xv = np.full((6, 3), 0.25, dtype=np.float32)
    before = lone(m, xi, xv, gpu)
    eng = m._engine
    f32_bytes = eng.serving_copy_bytes()
    assert f32_bytes == sum(sizes[3:]) * 64
    # the C call: UNSUPPORTED, the count, the message, and the model back on the plain tables
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    en, over, nb = ctypes.c_int32(7), ctypes.c_int64(7), ctypes.c_int64(7)
    L = _lib.lib()
    assert L.dfwfm_model_pack_tables_half(eng.handle, 1, ctypes.byref(en), ctypes.byref(over), st) == UNSUPPORTED
    assert (en.value, over.value) == (0, 1)
    assert b"1 categorical" in L.dfwfm_last_error()
    assert L.dfwfm_model_serving_copy_bytes(eng.handle, ctypes.byref(nb)) == 0 and nb.value == 0
    eng._packed_key = None
    # the module: DfwfmError naming the count; then f32 again, the same bits as before the attempt
    m.table_dtype = "fp16"
    with pytest.raises(DfwfmError, match=r"\b1 categorical"):
        lone(m, xi, xv, gpu)
    assert m._engine.serving_copy_bytes() == 0
    m.table_dtype = "f32"
    assert np.array_equal(lone(m, xi, xv, gpu), before)
    assert m._engine.serving_copy_bytes() == f32_bytes
    # 65519 and 65504 are not overflows (edge_case seeds them), inf and two more values are counted
    with torch.no_grad():
        m.fm_2nd_embeddings[5].weight[200, 7] = 65519.99
        m.fm_2nd_embeddings[9].weight[0, 0] = float("inf")
        m.fm_2nd_embeddings[4].weight[255, 9] = -65520.0
    m.table_dtype = "fp16"
    with pytest.raises(DfwfmError, match=r"\b2 categorical"):
        lone(m, xi, xv, gpu)


def test_pack_tables_half_state_and_drop(gpu):
    """The C calls on a device: before set_tables a state error; set_tables and pack_tables drop the fp16 copy."""
    from xsdeepfwfm_deprecated_amd import _lib
    L = _lib.lib()
    cfg = _lib.dfwfm_config(field_size=10, numerical=3, embedding_size=10, use_fwfm=1, use_fm=0, use_logit=0,
                            use_deep=0, use_lw=1, use_fwlw=0, h_depth=1, deep_nodes=16)
    h = ctypes.c_void_p()
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    en, over, nb = ctypes.c_int32(7), ctypes.c_int64(7), ctypes.c_int64(7)
    with torch.cuda.device(gpu):
        assert L.dfwfm_model_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        assert L.dfwfm_model_pack_tables_half(h, 1, ctypes.byref(en), ctypes.byref(over), st) == STATE
        assert b"set_tables" in L.dfwfm_last_error() and (en.value, over.value) == (0, 0)
    finally:
        L.dfwfm_model_destroy(h)
    _, m, sizes = edge_case(gpu)
    m.table_dtype = "fp16"
    xi = np.zeros((3, 7), dtype=np.int64)
    xv = np.ones((3, 3), dtype=np.float32)
    lone(m, xi, xv, gpu)
    eng = m._engine
    rows = sum(sizes[3:])
    assert eng.serving_copy_bytes() == rows * 32
    assert L.dfwfm_model_pack_tables(eng.handle, 1, ctypes.byref(en), st) == 0 and en.value == 1
    assert eng.serving_copy_bytes() == rows * 64  # the f32 copy took its place
    assert L.dfwfm_model_pack_tables_half(eng.handle, 1, ctypes.byref(en), None, st) == 0 and en.value == 1
    assert eng.serving_copy_bytes() == rows * 32
    assert L.dfwfm_model_pack_tables(eng.handle, 0, ctypes.byref(en), st) == 0 and en.value == 0
    assert eng.serving_copy_bytes() == 0
    eng._packed_key = None


# -- 4. refresh --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deep", [0, 1])
def test_fp16_tables_refreshed_after_updates_and_flips(gpu, deep):
    """tests/test_gpu_batches.py::test_packed_tables_bit_identical_and_refreshed for the fp16 copy: an in-place table
    update re-packs it; flipping f32 -> fp16 -> f32 re-packs each time; the copy's size is rows x 32, half the f32
    copy's, and 0 with pack_tables off."""
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw" if deep else "fwfm_nolw")
    xi, xv = xi[:100], xv[:100]
    m = make_model(cfg, params, gpu)
    rows = sum(cfg["feature_sizes"][cfg["numerical"]:])
    f32 = lone(m, xi, xv, gpu)
    assert m._engine.serving_copy_bytes() == rows * 64
    m.table_dtype = "fp16"
    h16 = lone(m, xi, xv, gpu)
    assert m._engine.serving_copy_bytes() == rows * 32
    assert np.array_equal(h16, lone(half_tables_ref.rounded_model(m), xi, xv, gpu))
    assert not np.array_equal(h16, f32)
    m.table_dtype = "f32"
    assert np.array_equal(lone(m, xi, xv, gpu), f32)
    assert m._engine.serving_copy_bytes() == rows * 64
    m.pack_tables = False
    assert np.array_equal(lone(m, xi, xv, gpu), f32)
    assert m._engine.serving_copy_bytes() == 0
    m.pack_tables = True
    m.table_dtype = "fp16"
    assert np.array_equal(lone(m, xi, xv, gpu), h16)
    # an in-place update (torch bumps the tables' version counters) -> the next forward re-packs
    with torch.no_grad():
        m.fm_2nd_embeddings[20].weight.mul_(-0.37)
        m.fm_1st_embeddings[30].weight.add_(0.25)
    new = lone(m, xi, xv, gpu)
    assert not np.array_equal(new, h16)
    assert np.array_equal(new, lone(half_tables_ref.rounded_model(m), xi, xv, gpu))


def test_fp16_tables_after_fused_training_steps(gpu):
    """tests/test_gpu_batches.py::test_packed_tables_after_fused_training_steps: the fused step updates the tables
    inside captured graphs (no version bump) and drops the copy's key; the next fp16 forward is the rounded model of
    the NEW tables."""
    from xsdeepfwfm_deprecated_amd import synth
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, m = fwfm_only_case(39, 13, 10, 1, 0, seed=29)
    m = m.to(gpu)
    m.eval()
    B = 256
    host = [synth.synth_inputs(cfg["feature_sizes"], 13, B, seed=8 + i) for i in range(3)]
    dev = [dev_inputs(xi, xv, gpu) for xi, xv in host]
    m.table_dtype = "fp16"
    before = lone(m, *host[0], gpu)  # packs
    m.train()
    t = FusedTrainStep(m, B, lr=1e-2, weight_decay=0.0)
    for xi, xv in dev[1:]:
        t.step(xi, xv, (torch.arange(B, device=gpu) % 3 == 0).float())
    t.close()
    m.eval()
    after = lone(m, *host[0], gpu)
    assert not np.array_equal(after, before)
    assert np.array_equal(after, lone(half_tables_ref.rounded_model(m), *host[0], gpu))


# -- 5. refusals, and training untouched ---------------------------------------------------------------------------
def test_fp16_tables_refusals(gpu):
    """One path, no fallback: every forward that would serve unrounded rows raises DfwfmError."""
    from xsdeepfwfm_deprecated_amd import DfwfmError
    for name in ("deepfwfm_qr_mult", "deepfwfm_fwlw_lw"):  # QR fields; fwlw without first-order tables
        cfg, params, xi, xv, *_ = load_golden(name)
        m = make_model(cfg, params, gpu)
        ok = lone(m, xi[:8], xv[:8], gpu)
        m.table_dtype = "fp16"
        with pytest.raises(DfwfmError, match="fp16"):
            lone(m, xi[:8], xv[:8], gpu)
        m.table_dtype = "f32"
        assert np.array_equal(lone(m, xi[:8], xv[:8], gpu), ok)
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    xi, xv = xi[:8], xv[:8]
    for knob, value in (("pack_tables", False), ("small_batch_rows", 64), ("mlp_dtype", "bf16")):
        m = make_model(cfg, params, gpu)
        m.table_dtype = "fp16"
        setattr(m, knob, value)  # (mlp_dtype = "bf16" with bf16_fused off: the per-layer forward)
        with pytest.raises(DfwfmError, match="fp16"):
            lone(m, xi, xv, gpu)
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_pruned")
    m = make_model(cfg, params, gpu)
    m.sparse_mlp_max_density = 0.25
    lone(m, xi[:8], xv[:8], gpu)
    assert m._engine._sparse_on
    m.table_dtype = "fp16"
    with pytest.raises(DfwfmError, match="sparse"):
        lone(m, xi[:8], xv[:8], gpu)
    m.table_dtype = "half"
    with pytest.raises(ValueError, match="table_dtype must be"):
        lone(m, xi[:8], xv[:8], gpu)


def test_training_does_not_read_the_fp16_copy(gpu):
    """A grad-mode forward and one fit step give the same bits with table_dtype = 'fp16' as with 'f32'."""
    cfg, params, xi, xv, y, *_ = load_golden("deepfwfm_lw")
    xi, xv, y = xi[:128], xv[:128], y[:128].astype(np.float32)
    res = {}
    for dt in ("f32", "fp16"):
        from xsdeepfwfm_deprecated_amd import DeepFMs
        m = DeepFMs(**model_kwargs(cfg), is_deep_dropout=False, n_epochs=1, batch_size=128, learning_rate=1e-2)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
        m = m.to(gpu).eval()
        m.table_dtype = dt
        lone(m, xi, xv, gpu)  # the copy is in place while training runs
        m.train()
        out = m(*dev_inputs(xi, xv, gpu))
        assert out.requires_grad
        grad_logits = out.detach().cpu().numpy()
        torch.manual_seed(3)
        np.random.seed(3)
        m.fit(xi.reshape(128, -1, 1), xv, y, [], [], [])
        res[dt] = (grad_logits, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()})
    assert np.array_equal(res["f32"][0], res["fp16"][0])
    for k in res["f32"][1]:
        assert np.array_equal(res["f32"][1][k], res["fp16"][1][k]), k


def test_eval_by_batch_and_predict_with_fp16_tables(gpu):
    """eval_by_batch (its batch sets) and predict_proba run the fp16 copy: the rounded model's numbers."""
    from xsdeepfwfm_deprecated_amd import synth
    cfg, params, m = fwfm_only_case(39, 13, 10, 1, 0, seed=41)
    m = m.to(gpu).eval()
    n = 2 * 8192 + 50
    xi, xv = synth.synth_inputs(cfg["feature_sizes"], 13, n, seed=6)
    y = (np.random.default_rng(2).random(n) < 0.3).astype(np.float32)
    r = half_tables_ref.rounded_model(m)
    m.table_dtype = "fp16"
    a = m.eval_by_batch(xi.reshape(n, 26, 1), xv, y, n)
    b = r.eval_by_batch(xi.reshape(n, 26, 1), xv, y, n)
    assert a == b
    assert np.array_equal(m.predict_proba(xi[:300].reshape(300, 26, 1), xv[:300]),
                          r.predict_proba(xi[:300].reshape(300, 26, 1), xv[:300]))
