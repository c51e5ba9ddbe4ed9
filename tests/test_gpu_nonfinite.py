"""GPU: a NaN (and, where the references agree, +Inf) in any parameter reaches the logits on every forward path.

The sites, the models and the expected masks are tests/nonfinite_cases.py's; its CPU leg (test_nonfinite_cases.py)
checks them.  One model per test, the parameter edited in place and restored; for every site the device's mask is the
CPU reference's row by row, and the rows a site cannot reach keep the clean model's bits (np.array_equal).  A path that
gives finite logits for a diverged model hides the divergence from eval_by_batch and from whoever serves the model.

The Criteo shape runs every path twice, with plain tables and with QR tables (the QR quotient-row site; the kernels'
QR gathers are code of their own).  One cell does not exist: the fp16 serving copy refuses a model with a QR field
(include/dfwfm_half_tables.h), which test_fp16_tables_refuse_the_qr_model pins.  The generic shape (D = 8) is outside
the supported set of the one-launch bf16 and int8 forwards; it runs the per-layer bf16 forward.  Every test asks the
engine which route it took after each poisoned forward, so no cell passes on another path."""
import numpy as np
import pytest
import torch

import nonfinite_cases as nf
from conftest import model_kwargs

pytestmark = pytest.mark.gpu

NO_TABLE_INF = ("table2", "table2_qr")  # the fp16 pack refuses an infinity in a table (test_gpu_half_tables.py)


def make_model(name, device, **kw):
    from xsdeepfwfm_deprecated_amd import DeepFMs
    cfg, params, xi, xv = nf.CASES[name]()
    m = DeepFMs(**model_kwargs(cfg), **kw)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    return m.to(device).eval()


def dev(xi, xv, device):
    return torch.from_numpy(np.array(xi)).to(device), torch.from_numpy(np.array(xv)).to(device)


def module_forward(m, device):
    """The module's own inference forward: the path its switches select."""
    def forward(xi, xv):
        with torch.no_grad():
            out = m(*dev(xi, xv, device))
        torch.cuda.synchronize()
        return out.cpu().numpy()
    return forward


def set_forward(m, device, method):
    """A batch set of two through eng.<method>: the rows, and the rows in reverse order.  Each batch must be its own
    lone forward, so the second is the first reversed, NaNs included."""
    def forward(xi, xv):
        with torch.no_grad():
            eng = m._sync_inference(device)
            batches = [dev(xi, xv, device), dev(xi[::-1], xv[::-1], device)]
            outs = [torch.zeros(nf.ROWS, dtype=torch.float32, device=device) for _ in batches]
            getattr(eng, method)(batches, outs)
        torch.cuda.synchronize()
        a, b = (o.cpu().numpy() for o in outs)
        assert np.array_equal(a, b[::-1], equal_nan=True)
        return a
    return forward


def fp16_copy_on(eng):
    """Whether the engine's serving copy is in use and is the fp16 one."""
    key = getattr(eng, "_packed_key", None)
    return bool(getattr(eng, "_packed_on", False)) and key is not None and key[1] == "fp16"


# -- the f32 forwards --------------------------------------------------------------------------------------------
F32_FORMS = ["fold", "nofold", "ng=8", "ng=4", "r32=1", "batches", "small", "fp16"]


@pytest.mark.parametrize("name,form", [(n, f) for n in ("criteo", "criteo_qr", "generic") for f in F32_FORMS
                                       if (n, f) != ("criteo_qr", "fp16")])
def test_f32_forward_paths(gpu, monkeypatch, name, form):
    """The one-launch forward, folded and not, on eight and four waves, its 32-row form, a batch set of two; the
    small-batch forward; the fp16 serving copy of the tables under it."""
    if "=" in form:
        monkeypatch.setenv("DFWFM_DIAG", form)
    m = make_model(name, gpu)
    m.fold_numerical = form != "nofold"
    if form == "small":
        m.small_batch_rows = 64
    if form == "fp16":
        m.table_dtype = "fp16"
    forward = set_forward(m, gpu, "forward_batches") if form == "batches" else module_forward(m, gpu)
    num = nf.CASES[name]()[0]["numerical"]

    def taken():
        eng = m._engine
        return (eng._fold_on is (form != "nofold" and num > 0) and eng.small_rows == (64 if form == "small" else 0)
                and not eng.bf16 and not eng.int8 and not getattr(eng, "_sparse_on", False)
                and fp16_copy_on(eng) is (form == "fp16"))
    nf.check_path(forward, m, name, "f32", (name, form), no_inf=NO_TABLE_INF if form == "fp16" else (), taken=taken)


def test_fp16_tables_refuse_the_qr_model(gpu):
    """Why there is no fp16 cell with QR tables: the copy does not cover a QR field, and the module raises rather
    than read the f32 tables under the fp16 switch."""
    from xsdeepfwfm_deprecated_amd import DfwfmError
    cfg, params, xi, xv = nf.CASES["criteo_qr"]()
    for dtype in ("f32", "int8"):
        m = make_model("criteo_qr", gpu)
        m.mlp_dtype, m.table_dtype = dtype, "fp16"
        with pytest.raises(DfwfmError):
            module_forward(m, gpu)(xi, xv)


@pytest.mark.parametrize("name", ["criteo", "criteo_qr", "generic"])
def test_train_mode_forward(gpu, name):
    """The training forward with dropout off: logits only."""
    m = make_model(name, gpu, is_deep_dropout=False).train()

    def forward(xi, xv):
        out = m(*dev(xi, xv, gpu))
        assert out.requires_grad
        torch.cuda.synchronize()
        return out.detach().cpu().numpy()
    nf.check_path(forward, m, name, "f32", (name, "train"))


@pytest.mark.parametrize("name", ["criteo_pruned_mlp", "criteo_qr_pruned_mlp"])
def test_sparse_mlp(gpu, name):
    """The pruned tower's ELL lists: a NaN weight is a kept entry, a NaN activation is read through nonzero weights."""
    m = make_model(name, gpu)
    m.sparse_mlp_max_density = 0.25
    nf.check_path(module_forward(m, gpu), m, name, "f32", ("sparse MLP", name), taken=lambda: m._engine._sparse_on)


@pytest.mark.parametrize("name,form", [(n, f) for n in ("criteo_shallow", "criteo_qr_shallow", "generic_shallow")
                                       for f in ("gram", "part3=0")]
                         + [("criteo_pruned_pairs", "pairs"), ("criteo_qr_pruned_pairs", "pairs")])
def test_mlp_free_kernels(gpu, monkeypatch, name, form):
    """Without a deep tower: the Gram form, the pieces form, and the pair list over a pruned field_cov."""
    if "=" in form:
        monkeypatch.setenv("DFWFM_DIAG", form)
    m = make_model(name, gpu)
    if form == "pairs":
        m.fwfm_pair_max = 192
    nf.check_path(module_forward(m, gpu), m, name, "f32", (name, form),
                  taken=lambda: bool(getattr(m._engine, "_pairs_on", False)) is (form == "pairs"))


# -- bf16 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [(n, f) for n in ("criteo", "criteo_qr")
                                       for f in ("layers", "fused", "fold", "batches", "fold batches")]
                         + [("generic", "layers")])
def test_bf16_forward_paths(gpu, name, form):
    """The per-layer bf16 forward, the one-launch form, its fold, and their batch sets."""
    m = make_model(name, gpu)
    m.mlp_dtype, m.bf16_fused, m.bf16_fold = "bf16", form != "layers", "fold" in form
    forward = set_forward(m, gpu, "forward_bf16_batches") if "batches" in form else module_forward(m, gpu)

    def taken():
        eng = m._engine
        return eng.bf16 and eng.bf16_fused is (form != "layers") and eng._bf16_fold_on is ("fold" in form)
    nf.check_path(forward, m, name, "bf16_fold" if "fold" in form else "bf16", (name, form), taken=taken)


# -- int8 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [(n, f) for n in ("criteo", "criteo_qr")
                                       for f in ("one", "int8rows=16", "int8rows=32", "batches")]
                         + [("criteo", "fp16")])
def test_int8_forward_paths(gpu, monkeypatch, name, form):
    """The int8 forward under both row tiles, its batch set, and over the fp16 tables.  A NaN hidden weight used to
    be packed as an ordinary zero (the pack's max dropped it): finite logits where f32 and bf16 give NaN."""
    if "=" in form:
        monkeypatch.setenv("DFWFM_DIAG", form)
    m = make_model(name, gpu)
    m.mlp_dtype = "int8"
    if form == "fp16":
        m.table_dtype = "fp16"
    forward = set_forward(m, gpu, "forward_int8_batches") if form == "batches" else module_forward(m, gpu)

    def taken():
        eng = m._engine
        return eng.int8 and not eng.bf16 and fp16_copy_on(eng) is (form == "fp16")
    nf.check_path(forward, m, name, "int8", (name, form), no_inf=NO_TABLE_INF if form == "fp16" else (), taken=taken)
