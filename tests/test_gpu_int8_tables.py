"""GPU: the int8 serving copy of the categorical tables (include/dfwfm_int8_tables.h, DeepFMs.table_dtype = "int8").
The yardstick is exact: the served value q * s is an exact f32 product and everything behind the load is the f32 copy's
arithmetic, so with int8 tables a model's logits are, bit for bit, the logits of the same path on
tests/int8_tables_ref.quantized_model -- the model whose categorical second-order tables are the dequantized values --
with the f32 copy.  No tolerance anywhere.

One case differs from the issue that asked for this file.  It lists 1.7e38 among three values the pack must refuse,
and the contract it sets refuses |x| >= 2^127 = 1.70141...e38: float32(1.7e38) is below that bound and is served.
The test below keeps the contract's bound: it refuses +inf, -2^127 and 1.71e38 (count 3), and serves 1.6e38 and 1.7e38."""
import ctypes

import numpy as np
import pytest
import torch

import half_tables_ref
import int8_tables_ref
from conftest import golden_names, load_golden, model_kwargs

pytestmark = pytest.mark.gpu

UNSUPPORTED, STATE = -2, -4
MUST_BE_COVERED = ["deepfwfm_lw", "tiny_deepfwfm_lw", "tiny_fwfm_lw"]
NON_QR_GOLDENS = [n for n in golden_names() if "qr" not in n]
SETS = [(3, 33), (2, 256)]
STRIDE = {4: 16, 8: 16, 10: 16, 16: 32, 32: 48}


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
    """{path: logits} over every forward the int8 copy composes with, on this module as it is configured (its
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


def assert_int8_is_the_quantized_model(m, xi, xv, device, what):
    """table_dtype = 'int8' on m == the f32 copy on quantized_model(m), every path, array_equal."""
    r = int8_tables_ref.quantized_model(m)
    r.table_dtype = "f32"
    ref = all_paths(r, xi, xv, device)
    assert r._engine._packed_on and r._engine.serving_copy_bytes() > 0
    m.table_dtype = "int8"
    got = all_paths(m, xi, xv, device)
    assert m._engine._packed_on
    assert set(got) == set(ref)
    for k in ref:
        assert np.all(np.isfinite(ref[k])), (what, k)
        assert np.array_equal(got[k], ref[k]), (what, k, float(np.abs(got[k] - ref[k]).max()))
    return got, ref


# -- 1. bit identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NON_QR_GOLDENS)
def test_int8_tables_are_the_quantized_model_on_goldens(gpu, name):
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
    got, ref = assert_int8_is_the_quantized_model(m, xi, xv, gpu, name)
    assert len(got) >= (9 if name in MUST_BE_COVERED and cfg["use_deep"] else 3)
    assert not np.array_equal(got["f32 lone"], plain), "the quantization must be visible"
    rows = sum(cfg["feature_sizes"][cfg["numerical"]:])
    assert m._engine.serving_copy_bytes() == rows * STRIDE[cfg["embedding_size"]]


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
def test_int8_tables_fwfm_only_shapes(gpu, F, num, D, lw, fm, B):
    """Every embedding size the library instantiates (row strides 16, 32 and 48 bytes), FwFM row tiles 1 to 3, FM,
    with and without lw: lone (eight waves) and as a set (four waves)."""
    from xsdeepfwfm_deprecated_amd import synth
    cfg, params, m = fwfm_only_case(F, num, D, lw, fm, seed=F * 100 + D)
    m = m.to(gpu).eval()
    xi, xv = synth.synth_inputs(cfg["feature_sizes"], num, 3 * B, seed=F + D + B)
    r = int8_tables_ref.quantized_model(m)
    plain = lone(m, xi[:B], xv[:B], gpu)
    m.table_dtype = "int8"
    got = lone(m, xi[:B], xv[:B], gpu)
    assert np.array_equal(got, lone(r, xi[:B], xv[:B], gpu))
    assert not np.array_equal(got, plain)
    assert np.array_equal(as_set(m, "forward_batches", xi, xv, 3, B, gpu),
                          as_set(r, "forward_batches", xi, xv, 3, B, gpu))
    rows = sum(cfg["feature_sizes"][num:])
    assert m._engine.serving_copy_bytes() == rows * STRIDE[D]


@pytest.mark.parametrize("D,N,H", [(8, 64, 2), (10, 100, 1), (16, 400, 3), (10, 400, 3)])
def test_int8_tables_deep_f32_forms(gpu, D, N, H):
    """The f32 deep forward's forms: generic tile counts and embedding sizes (their own int8 instantiations), the
    static 3x400 one, folded and unfolded, at 99 rows, lone and as sets."""
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
        got, _ = assert_int8_is_the_quantized_model(m, xi, xv, gpu, (D, N, H, fold))
        assert not np.array_equal(got["f32 lone"], plain)


# -- 2. edges ----------------------------------------------------------------------------------------------------
# the critical rows of tests/test_int8_tables_boundary.py; its 3e38 row is beyond what the pack serves (the refusal
# test's ground), so a row of large servable magnitudes whose pair products stay finite stands in for it
TIES = [127, .5, 1.5, 2.5, -.5, -1.5, 63.5, -126.5, 126.5, -127]
ODD254 = [1.0] + [(2 * i + 1) / 254.0 for i in range(9)]
CRITICAL_ROWS = [
    [0.0] * 10,
    [1e-45] * 10,
    TIES,
    ODD254,
    [3e17, -1e17, 1.0, 0.0, 2e16, -3e17, 1e10, 5e15, -7e16, 2.9e17],
]


def edge_case(gpu):
    """Tables of 1, 256 and 257 rows (the pack kernel's one-row, full and last partial workgroup) among others, their
    first and last rows seeded with the rows where the quantizer can go wrong."""
    sizes = [1, 1, 1] + [1, 256, 257, 2, 255, 513, 300]
    cfg, params, m = fwfm_only_case(10, 3, 10, 1, 0, seed=3, sizes=sizes)
    rows = torch.tensor(CRITICAL_ROWS, dtype=torch.float32)
    with torch.no_grad():
        for i, f in enumerate(range(3, 10)):
            w = m.fm_2nd_embeddings[f].weight
            w[-1] = rows[(i + 2) % len(rows)]  # the last row ...
            w[0] = rows[i % len(rows)]         # ... and the first (a one-row table keeps this one)
    return cfg, m.to(gpu).eval(), sizes


def test_int8_tables_edge_rows_and_critical_values(gpu):
    cfg, m, sizes = edge_case(gpu)
    cat = np.array(sizes[3:], dtype=np.int64)
    rng = np.random.default_rng(5)
    B = 40
    xv = rng.random((B, 3), dtype=np.float32)
    last = np.tile(cat - 1, (B, 1))                      # every index at its table's last row
    first = np.zeros((B, 7), dtype=np.int64)
    mixed = rng.integers(0, cat, size=(B, 7))
    mixed[::3] = np.where(rng.random((len(mixed[::3]), 7)) < 0.5, 0, cat - 1)  # first and last rows side by side
    r = int8_tables_ref.quantized_model(m)
    # the reference model holds what the CPU test expects of the seeded rows: the tie row under scale 1
    w = r.fm_2nd_embeddings[5].weight.detach().cpu().numpy()  # (table 2 of 7: first row TIES)
    assert w[0].tolist() == [127.0, 0.0, 2.0, 2.0, 0.0, -2.0, 64.0, -126.0, 126.0, -127.0]
    m.table_dtype = "int8"
    for what, xi in (("last", last), ("first", first), ("mixed", mixed)):
        a, b = lone(m, xi, xv, gpu), lone(r, xi, xv, gpu)
        assert np.all(np.isfinite(b)), what
        assert np.array_equal(a, b), what
        assert np.array_equal(as_set(m, "forward_batches", xi, xv, 2, 20, gpu),
                              as_set(r, "forward_batches", xi, xv, 2, 20, gpu)), what
    assert m._engine.serving_copy_bytes() == sum(sizes[3:]) * 16
    # the quantized model is not the original one
    m.table_dtype = "f32"
    assert not np.array_equal(lone(m, last, xv, gpu), lone(r, last, xv, gpu))


def test_int8_tables_out_of_range_index_clamps_and_raises(gpu):
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
    m.table_dtype = "int8"
    with pytest.raises(IndexError):
        lone(m, bad, xv, gpu)
    m.strict_index_check = False
    got = lone(m, bad, xv, gpu)
    assert m._engine.read_error_flag() != 0
    m.strict_index_check = True
    assert np.array_equal(got, lone(m, clamped, xv, gpu))
    assert np.array_equal(got, lone(int8_tables_ref.quantized_model(m), clamped, xv, gpu))


# -- 3. unservable values ------------------------------------------------------------------------------------------
def test_int8_unservable_values_are_refused_and_the_model_stays_usable(gpu):
    from xsdeepfwfm_deprecated_amd import DfwfmError, _lib
    cfg, m, sizes = edge_case(gpu)
    with torch.no_grad():
        m.fm_2nd_embeddings[5].weight[200, 7] = float("nan")
    cat = np.array(sizes[3:], dtype=np.int64)
    rows = int(cat.sum())
    xi = np.tile(np.minimum(cat - 1, 100), (6, 1))  # (not the row that holds the NaN: the logits stay finite)
    xv = np.full((6, 3), 0.25, dtype=np.float32)
    before = lone(m, xi, xv, gpu)
    assert np.all(np.isfinite(before))
    eng = m._engine
    f32_bytes = eng.serving_copy_bytes()
    assert f32_bytes == rows * 64
    # the C call: UNSUPPORTED, the count, the message, and the model back on the plain tables
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    en, bad, nb = ctypes.c_int32(7), ctypes.c_int64(7), ctypes.c_int64(7)
    L = _lib.lib()
    assert L.dfwfm_model_pack_tables_int8(eng.handle, 1, ctypes.byref(en), ctypes.byref(bad), st) == UNSUPPORTED
    assert (en.value, bad.value) == (0, 1)
    assert b"1 categorical" in L.dfwfm_last_error()
    assert L.dfwfm_model_serving_copy_bytes(eng.handle, ctypes.byref(nb)) == 0 and nb.value == 0
    eng._packed_key = None
    # the module: DfwfmError naming the dtype and the count; then f32 again, the same bits as before the attempt
    m.table_dtype = "int8"
    with pytest.raises(DfwfmError, match=r"table_dtype='int8': 1 categorical"):
        lone(m, xi, xv, gpu)
    assert m._engine.serving_copy_bytes() == 0
    m.table_dtype = "f32"
    assert np.array_equal(lone(m, xi, xv, gpu).view(np.uint32), before.view(np.uint32))
    assert m._engine.serving_copy_bytes() == f32_bytes
    # +inf, -2^127 and a finite value above 2^127 are counted
    with torch.no_grad():
        m.fm_2nd_embeddings[5].weight[200, 7] = 0.01
        m.fm_2nd_embeddings[9].weight[0, 0] = float("inf")
        m.fm_2nd_embeddings[4].weight[255, 9] = -(2.0 ** 127)
        m.fm_2nd_embeddings[8].weight[512, 3] = 1.71e38
    m.table_dtype = "int8"
    with pytest.raises(DfwfmError, match=r"table_dtype='int8': 3 categorical"):
        lone(m, xi, xv, gpu)
    # 1.6e38 alone is served, and so is 1.7e38 (below 2^127): 127 s stays finite after the scale's round-up
    with torch.no_grad():
        m.fm_2nd_embeddings[9].weight[0, 0] = 0.02
        m.fm_2nd_embeddings[4].weight[255, 9] = 1.7e38
        m.fm_2nd_embeddings[8].weight[512, 3] = 1.6e38
    got = lone(m, xi, xv, gpu)
    assert m._engine._packed_on and m._engine.serving_copy_bytes() == rows * 16
    assert np.array_equal(got, lone(int8_tables_ref.quantized_model(m), xi, xv, gpu))
    for f, row in ((4, 255), (8, 512)):
        w = m.fm_2nd_embeddings[f].weight.detach().cpu().numpy()[row:row + 1]
        assert np.all(np.isfinite(int8_tables_ref.dequantized(w)))
    xi2 = xi.copy()
    xi2[:, 5] = 512  # the row that holds 1.6e38, read through the copy: the same bits as the quantized model's
    a, b = lone(m, xi2, xv, gpu), lone(int8_tables_ref.quantized_model(m), xi2, xv, gpu)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_pack_tables_int8_state_and_drop(gpu):
    """The C calls on a device: before set_tables a state error; the three pack calls replace one another's copy."""
    from xsdeepfwfm_deprecated_amd import _lib
    L = _lib.lib()
    cfg = _lib.dfwfm_config(field_size=10, numerical=3, embedding_size=10, use_fwfm=1, use_fm=0, use_logit=0,
                            use_deep=0, use_lw=1, use_fwlw=0, h_depth=1, deep_nodes=16)
    h = ctypes.c_void_p()
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    en, bad = ctypes.c_int32(7), ctypes.c_int64(7)
    with torch.cuda.device(gpu):
        assert L.dfwfm_model_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        assert L.dfwfm_model_pack_tables_int8(h, 1, ctypes.byref(en), ctypes.byref(bad), st) == STATE
        assert b"set_tables" in L.dfwfm_last_error() and (en.value, bad.value) == (0, 0)
    finally:
        L.dfwfm_model_destroy(h)
    sizes = [1, 1, 1] + [1, 256, 257, 2, 255, 513, 300]  # (edge_case's tables, unseeded: 3e17 overflows the fp16 copy)
    m = fwfm_only_case(10, 3, 10, 1, 0, seed=3, sizes=sizes)[2].to(gpu).eval()
    r = int8_tables_ref.quantized_model(m)
    m.table_dtype = "int8"
    xi = np.zeros((3, 7), dtype=np.int64)
    xv = np.ones((3, 3), dtype=np.float32)
    want = lone(r, xi, xv, gpu)
    assert np.array_equal(lone(m, xi, xv, gpu), want)
    eng = m._engine
    rows = sum(sizes[3:])
    assert eng.serving_copy_bytes() == rows * 16
    assert L.dfwfm_model_pack_tables(eng.handle, 1, ctypes.byref(en), st) == 0 and en.value == 1
    assert eng.serving_copy_bytes() == rows * 64  # the f32 copy took its place
    assert L.dfwfm_model_pack_tables_int8(eng.handle, 1, ctypes.byref(en), None, st) == 0 and en.value == 1
    assert eng.serving_copy_bytes() == rows * 16
    assert L.dfwfm_model_pack_tables_half(eng.handle, 1, ctypes.byref(en), None, st) == 0 and en.value == 1
    assert eng.serving_copy_bytes() == rows * 32  # ... and the fp16 copy
    assert L.dfwfm_model_pack_tables_int8(eng.handle, 1, ctypes.byref(en), ctypes.byref(bad), st) == 0
    assert (en.value, bad.value) == (1, 0) and eng.serving_copy_bytes() == rows * 16
    with torch.no_grad():  # the engine's key still says int8: this forward reads the copy the C call just built
        out = torch.empty(3, device=gpu)
        eng.forward(*dev_inputs(xi, xv, gpu), out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert L.dfwfm_model_pack_tables_int8(eng.handle, 0, ctypes.byref(en), None, st) == 0 and en.value == 0
    assert eng.serving_copy_bytes() == 0  # enable = 0 drops the copy
    eng._packed_key = None


# -- 4. refresh --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deep", [0, 1])
def test_int8_tables_refreshed_after_updates_and_flips(gpu, deep):
    """An in-place table update re-packs the copy; the flips f32 -> int8 -> fp16 -> f32 re-pack each time; the copy's
    size is rows x 16, a quarter of the f32 copy's; pack_tables = False raises."""
    from xsdeepfwfm_deprecated_amd import DfwfmError
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw" if deep else "fwfm_nolw")
    xi, xv = xi[:100], xv[:100]
    m = make_model(cfg, params, gpu)
    rows = sum(cfg["feature_sizes"][cfg["numerical"]:])
    f32 = lone(m, xi, xv, gpu)
    assert m._engine.serving_copy_bytes() == rows * 64
    m.table_dtype = "int8"
    q8 = lone(m, xi, xv, gpu)
    assert m._engine.serving_copy_bytes() == rows * 16
    assert np.array_equal(q8, lone(int8_tables_ref.quantized_model(m), xi, xv, gpu))
    assert not np.array_equal(q8, f32)
    m.table_dtype = "fp16"
    h16 = lone(m, xi, xv, gpu)
    assert m._engine.serving_copy_bytes() == rows * 32
    assert np.array_equal(h16, lone(half_tables_ref.rounded_model(m), xi, xv, gpu))
    assert not np.array_equal(h16, q8)
    m.table_dtype = "f32"
    assert np.array_equal(lone(m, xi, xv, gpu), f32)
    assert m._engine.serving_copy_bytes() == rows * 64
    m.table_dtype = "int8"
    m.pack_tables = False
    with pytest.raises(DfwfmError, match="table_dtype='int8'"):
        lone(m, xi, xv, gpu)
    m.pack_tables = True
    assert np.array_equal(lone(m, xi, xv, gpu), q8)
    # an in-place update (torch bumps the tables' version counters) -> the next forward re-packs
    with torch.no_grad():
        m.fm_2nd_embeddings[20].weight.mul_(-0.37)
        m.fm_1st_embeddings[30].weight.add_(0.25)
    new = lone(m, xi, xv, gpu)
    assert not np.array_equal(new, q8)
    assert np.array_equal(new, lone(int8_tables_ref.quantized_model(m), xi, xv, gpu))


def test_int8_tables_after_fused_training_steps(gpu):
    """The fused step updates the tables inside captured graphs (no version bump) and drops the copy's key; the next
    int8 forward is the quantized model of the NEW tables."""
    from xsdeepfwfm_deprecated_amd import synth
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, m = fwfm_only_case(39, 13, 10, 1, 0, seed=29)
    m = m.to(gpu)
    m.eval()
    B = 256
    host = [synth.synth_inputs(cfg["feature_sizes"], 13, B, seed=8 + i) for i in range(3)]
    dev = [dev_inputs(xi, xv, gpu) for xi, xv in host]
    m.table_dtype = "int8"
    before = lone(m, *host[0], gpu)  # packs
    m.train()
    t = FusedTrainStep(m, B, lr=1e-2, weight_decay=0.0)
    for xi, xv in dev[1:]:
        t.step(xi, xv, (torch.arange(B, device=gpu) % 3 == 0).float())
    t.close()
    m.eval()
    after = lone(m, *host[0], gpu)
    assert not np.array_equal(after, before)
    assert np.array_equal(after, lone(int8_tables_ref.quantized_model(m), *host[0], gpu))


# -- 5. refusals ---------------------------------------------------------------------------------------------------
def test_int8_tables_refusals(gpu):
    """One path, no fallback: every forward that would serve unquantized rows raises DfwfmError."""
    from xsdeepfwfm_deprecated_amd import DfwfmError
    for name in ("deepfwfm_qr_mult", "deepfwfm_fwlw_lw"):  # QR fields; fwlw without first-order tables
        cfg, params, xi, xv, *_ = load_golden(name)
        m = make_model(cfg, params, gpu)
        ok = lone(m, xi[:8], xv[:8], gpu)
        m.table_dtype = "int8"
        with pytest.raises(DfwfmError, match="table_dtype='int8'"):
            lone(m, xi[:8], xv[:8], gpu)
        m.table_dtype = "f32"
        assert np.array_equal(lone(m, xi[:8], xv[:8], gpu), ok)
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_lw")
    xi, xv = xi[:8], xv[:8]
    for knob, value in (("pack_tables", False), ("small_batch_rows", 64), ("mlp_dtype", "bf16")):
        m = make_model(cfg, params, gpu)
        m.table_dtype = "int8"
        setattr(m, knob, value)  # (mlp_dtype = "bf16" with bf16_fused off: the per-layer forward)
        with pytest.raises(DfwfmError, match="table_dtype='int8'"):
            lone(m, xi, xv, gpu)
    cfg, params, xi, xv, *_ = load_golden("deepfwfm_pruned")
    m = make_model(cfg, params, gpu)
    m.sparse_mlp_max_density = 0.25
    lone(m, xi[:8], xv[:8], gpu)
    assert m._engine._sparse_on
    m.table_dtype = "int8"
    with pytest.raises(DfwfmError, match="table_dtype='int8'.*sparse"):
        lone(m, xi[:8], xv[:8], gpu)
    m.table_dtype = "int4"
    with pytest.raises(ValueError, match="^table_dtype must be"):
        lone(m, xi[:8], xv[:8], gpu)


def test_eval_by_batch_and_predict_with_int8_tables(gpu):
    """eval_by_batch (its batch sets) and predict_proba run the int8 copy: the quantized model's numbers."""
    from xsdeepfwfm_deprecated_amd import synth
    cfg, params, m = fwfm_only_case(39, 13, 10, 1, 0, seed=41)
    m = m.to(gpu).eval()
    n = 2 * 8192 + 50
    xi, xv = synth.synth_inputs(cfg["feature_sizes"], 13, n, seed=6)
    y = (np.random.default_rng(2).random(n) < 0.3).astype(np.float32)
    r = int8_tables_ref.quantized_model(m)
    m.table_dtype = "int8"
    a = m.eval_by_batch(xi.reshape(n, 26, 1), xv, y, n)
    b = r.eval_by_batch(xi.reshape(n, 26, 1), xv, y, n)
    assert a == b
    assert np.array_equal(m.predict_proba(xi[:300].reshape(300, 26, 1), xv[:300]),
                          r.predict_proba(xi[:300].reshape(300, 26, 1), xv[:300]))
