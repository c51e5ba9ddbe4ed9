"""Training-step cases outside the train goldens' one model family, a float64 autograd reference and the checks both
device legs share (tests/test_train_variants.py: the host kernels; tests/test_gpu_train_variants.py: the HIP kernels).

The goldens and test_gpu_train's sweeps train `use_fwfm=1`, numerical=13, QR "mult" only.  CASES walks the branches the
backward carries beside that: FM (R = 1, no field_cov gradient), logistic regression (no per-tile backward), QR "add",
fwlw with lw, shallow models, EmbeddingBag tables, and the shapes where the numerical / categorical split changes the
kernels' layouts (numerical = 0, = F, > 16, and F = 64, the field limit).

The reference is oracle/torch_port.forward_graph on float64 leaves (the fp32 port's own error against it is the
yardstick: test_train_variants.test_fp32_port_within_quarter_bar)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import table_cases
from conftest import logit_close, logit_close_scaled, model_kwargs
from oracle import torch_port

G_TOL = 2e-5  # test_gpu_train.G_TOL / test_cpu_kernel.G_TOL: of a tensor's (here also: a row's) largest entry


def edge_rows(cfg, xi):
    """xi with its first three rows forced to the ends of every table's index range: row 0 all 0, row 1 n - 1 per
    field, row 2 the last index a QR field accepts, ceil(n / c) c - 1 (>= n when c does not divide n: the quotient
    table's last row; QREmbeddingBag rejects only i // c >= ceil(n / c)), and n - 1 for a plain field."""
    num, c = cfg["numerical"], cfg["qr_collisions"]
    n = np.asarray(cfg["feature_sizes"][num:], np.int64)
    isqr = (n > cfg["qr_threshold"]) & bool(cfg["qr_flag"])
    xi = xi.copy()
    xi[0], xi[1], xi[2] = 0, n - 1, np.where(isqr, -(-n // c) * c - 1, n - 1)
    return xi


def train_case(F, num, D, N, H, kind="fwfm", deep=1, lw=1, fwlw=0, qr=0, op="mult", embbag=0, B=37, seed=11,
               sizes=None, c=4, threshold=200, edges=False):
    """(cfg, params, xi, xv, y): test_gpu_parity._sweep_case over the model kinds.  B = 37 is two full 16-row tiles
    and a ragged 5; the tables (50 .. 449 rows) are small enough that a batch hits some rows twice and leaves most
    untouched.  sizes: the categorical tables' row counts instead; c, threshold: qr_collisions, qr_threshold;
    edges: rows 0 .. 2 are edge_rows' (tests/table_cases.py: the table zoo)."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    cat = [int(x) for x in 50 + (np.arange(F - num) * 37) % 400] if sizes is None else [int(x) for x in sizes]
    assert len(cat) == F - num
    sizes = [1] * num + cat
    cfg = dict(field_size=F, feature_sizes=sizes, embedding_size=D, use_fwfm=int(kind == "fwfm"),
               use_fm=int(kind == "fm"), use_logit=int(kind == "logit"), use_deep=int(deep), use_lw=int(lw),
               use_fwlw=int(fwlw), h_depth=H, deep_nodes=N, numerical=num, embedding_bag=int(embbag), qr_flag=int(qr),
               qr_operation=op, qr_collisions=int(c), qr_threshold=int(threshold))
    m = DeepFMs(**model_kwargs(cfg))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    params = synth.synth_state(shapes, F, D, N, kind in ("fwfm", "fm"), bool(deep), seed=seed)
    xi, xv = synth.synth_inputs(sizes, num, B, seed=seed)
    if edges:
        xi = edge_rows(cfg, xi)
    y = (np.arange(B) % 3 == 0).astype(np.float32)
    return cfg, params, xi, xv, y


def port_xi(xi):
    """Xi as oracle/torch_port takes it: its reshape(B, -1) cannot infer a width from a [B, 0] array (a model without
    categorical fields), so that one gets a column nobody reads."""
    return xi if xi.shape[1] else np.zeros((len(xi), 1), np.int64)


def ref_step64(cfg, params, xi, xv, y, masks=None, drop_p=0.0):
    """(logits, loss, grads) of one training step in float64: torch_port.forward_graph on float64 leaves, BCE with
    logits (mean), autograd.  A parameter autograd leaves without a gradient gets zeros."""
    leaf = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    out = torch_port.forward_graph(cfg, leaf, torch.as_tensor(port_xi(xi)),
                                   torch.as_tensor(xv, dtype=torch.float64), masks, drop_p)
    loss = F.binary_cross_entropy_with_logits(out, torch.as_tensor(y, dtype=torch.float64))
    loss.backward()
    grads = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(params[k].shape, np.float64))
             for k, v in leaf.items()}
    return out.detach().numpy(), float(loss.item()), grads


def port_step(cfg, params, xi, xv, y, lr, l2, masks=None, drop_p=0.0):
    """torch_port.train_step (the fp32 port with torch.optim.Adam) on a case's inputs."""
    return torch_port.train_step(cfg, params, port_xi(xi), xv, y, lr, l2, masks, drop_p)


def table_rows(cfg, xi):
    """{parameter name: bool mask of the rows this batch reads} for every categorical table of both families (plain
    tables: xi[:, f]; QR tables: quotient rows xi // c, remainder rows xi % c); a model has one or both families."""
    num, c, out = cfg["numerical"], cfg["qr_collisions"], {}
    for j in range(cfg["field_size"] - num):
        n, idx = cfg["feature_sizes"][num + j], xi[:, j]
        for fam in ("fm_1st_embeddings", "fm_2nd_embeddings"):
            if cfg["qr_flag"] and n > cfg["qr_threshold"]:
                for suffix, rows, size in (("weight_q", idx // c, -(-n // c)), ("weight_r", idx % c, c)):
                    mask = np.zeros(size, bool)
                    mask[rows] = True
                    out[f"{fam}.{num + j}.{suffix}"] = mask
            else:
                mask = np.zeros(n, bool)
                mask[idx] = True
                out[f"{fam}.{num + j}.weight"] = mask
    return out


def grad_stats(cfg, xi, got_grads, ref_grads):
    """(worst per-tensor ratio, worst per-row ratio, offending names): |g - g64|.max() over |g64|.max() per
    parameter, and per touched row of the categorical tables over that row's largest reference entry."""
    worst_t, worst_r, where_t, where_r = 0.0, 0.0, None, None
    for k, r in ref_grads.items():
        sc = np.abs(r).max(initial=0.0)
        if sc == 0.0 or got_grads.get(k) is None:
            continue
        e = float(np.abs(got_grads[k].astype(np.float64) - r).max() / sc)
        if e > worst_t:
            worst_t, where_t = e, k
    for k, mask in table_rows(cfg, xi).items():
        if k not in ref_grads:
            continue
        r = ref_grads[k][mask]
        g = got_grads[k].astype(np.float64)[mask]
        sc = np.abs(r).max(axis=1)
        ok = sc > 0
        if ok.any():
            e = float((np.abs(g - r).max(axis=1)[ok] / sc[ok]).max())
            if e > worst_r:
                worst_r, where_r = e, k
    return worst_t, worst_r, where_t, where_r


def check_step(cfg, params, xi, xv, got_logits, got_loss, got_grads, ref, per_row=True):
    """One step's logits, loss and every gradient against ref = ref_step64(...); returns (per-tensor, per-row) worst
    gradient ratios for the record.  per_row=False (tests/dense_edge_cases.py: batches of hundreds of rows, where the
    fp32 port itself misses it) leaves out the bar on each touched table row, nothing else."""
    ref_logits, ref_loss, ref_grads = ref
    shallow2 = cfg["use_fwfm"] or cfg["use_fm"]
    if cfg["use_lw"] and shallow2:
        assert logit_close(got_logits, ref_logits) < 1e-5
    else:  # no lw, or logistic regression: first-order terms of size ~1e2 cancel
        assert logit_close_scaled(got_logits, ref_logits, cfg, params, port_xi(xi), xv) < 1e-5
    assert abs(got_loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    assert set(got_grads) == set(ref_grads)
    for k, r in ref_grads.items():
        g = got_grads[k]
        sc = np.abs(r).max(initial=0.0)
        if sc == 0.0:  # autograd leaves it without a gradient, or with an exact zero one
            assert g is None or not np.any(g), k
            continue
        assert g is not None and g.shape == r.shape, k
        assert np.abs(g.astype(np.float64) - r).max() <= G_TOL * sc, (k, np.abs(g - r).max() / sc)
    rows = {k: mask for k, mask in table_rows(cfg, xi).items() if k in ref_grads}  # the families the model has
    assert {k for k in ref_grads if "embeddings" in k and int(k.split(".")[1]) >= cfg["numerical"]} == set(rows)
    for k, mask in rows.items():
        g = got_grads[k]
        if g is None:  # only where the reference is identically zero (checked above)
            continue
        assert np.all(g[~mask] == 0.0), (k, "gradient in a row the batch did not touch")
        r = ref_grads[k][mask]
        err = np.abs(g.astype(np.float64)[mask] - r).max(axis=1)
        assert not per_row or np.all(err <= G_TOL * np.abs(r).max(axis=1)), (k, "per-row")
    wt, wr, _, _ = grad_stats(cfg, xi, got_grads, ref_grads)
    return wt, wr


_V = dict(F=39, num=13, D=10, N=64, H=2)
CASES = {
    # model variants at the goldens' field split
    "fm_deep": dict(_V, kind="fm"),
    "fm_deep_nolw": dict(_V, kind="fm", lw=0),
    "fm_shallow": dict(_V, kind="fm", deep=0),
    "logit": dict(_V, kind="logit", deep=0),
    "fwfm_shallow_lw": dict(_V, deep=0, lw=1),
    "fwlw_lw": dict(_V, fwlw=1, lw=1),
    "qr_add": dict(_V, qr=1, op="add"),
    "qr_add_fwlw": dict(_V, qr=1, op="add", fwlw=1, lw=0),
    "embbag": dict(_V, embbag=1, qr=0),
    # shapes (fwfm + deep + lw): the smallest at which each layout branch is taken
    "num0": dict(F=20, num=0, D=8, N=128, H=2),        # no numerical field: xv stride 0
    "allnum": dict(F=39, num=39, D=4, N=64, H=1),      # no categorical field; 16 num = 624 > 256 threads
    "num20": dict(F=24, num=20, D=8, N=64, H=1),       # num > 16 and num D = 160 > 144
    "f64": dict(F=64, num=16, D=10, N=256, H=2),       # the field limit: 4 Gram tiles; 136 tensors for Adam
    "logit_num20": dict(F=39, num=20, D=10, N=64, H=2, kind="logit", deep=0),  # reduce_kernel's num > 16 staging
}
# A seed per case (weights and inputs), chosen among 1 .. 60 as one on which the fp32 port's own error stays under
# G_TOL / 4 per tensor AND per touched row (test_train_variants.test_fp32_port_within_quarter_bar).  Most seeds miss
# the per-row figure, and not through any kernel: a table row read by one sample carries that sample's
# dlogit = (sigmoid(z) - y) / B, whose relative error is |dz| (1 - sigmoid(z)) for y = 0 -- with first-order terms of
# size ~1e2 (Xv up to 63 times weights ~ N(0, 1)) one fp32 ulp of z is already 8e-6 -- and a row read by a y = 0 and
# a y = 1 sample can cancel to a few per cent of either.  The seeds below put every sample on the side where
# sigmoid(z) - y is well conditioned, or saturate it to an exact 0 in float64 too (then the row must be exactly 0).
SEEDS = {"fm_deep": 16, "fm_deep_nolw": 33, "fm_shallow": 16, "logit": 33, "fwfm_shallow_lw": 16, "fwlw_lw": 3,
         "qr_add": 16, "qr_add_fwlw": 5, "embbag": 16, "num0": 22, "allnum": 2, "num20": 16, "f64": 25,
         "logit_num20": 33}


# The table zoo (tests/table_cases.py): tables at the row counts where the scatter kernels switch paths, QR collision
# counts c that put the remainder table at the same switch points, the forced edge rows included.  Seeds by the same
# rule, forced rows included (and for c <= 7 every remainder row read by the 37 samples: table_cases.check_inputs).
CASES.update({table_cases.name(op, c): table_cases.train_kwargs(op, c)
              for op in table_cases.OPS for c in table_cases.C_ALL})
# 14 to 29 of the seeds 1 .. 60 qualify per (c, op); 20 is the one that does for all sixteen.
SEEDS.update({name: 20 for name in CASES if name.startswith("zoo_")})
# The 39-field zoo (table_cases.WIDE: the smallest shape the helper-wave training forward takes) over C_FEW: 2 to 17
# seeds qualify per case and none for all six; each case gets its own with the smallest per-row figure.
CASES.update({table_cases.name(op, c, True): table_cases.train_kwargs(op, c, True)
              for op in table_cases.OPS for c in table_cases.C_FEW})
SEEDS.update({"zoo39_mult_c1": 36, "zoo39_mult_c7": 44, "zoo39_mult_c129": 47, "zoo39_add_c1": 9, "zoo39_add_c7": 12,
              "zoo39_add_c129": 25})

RAGGED = [(name, B) for name in ("num0", "allnum", "logit") for B in (1, 16, 17)]
DROPOUT_RATES = (0.1, 0.9)
FUSED = ("fm_deep", "qr_add", "num0", "allnum") + tuple(table_cases.name(op, c) for c in table_cases.C_FEW
                                                       for op in table_cases.OPS)


@functools.lru_cache(maxsize=None)
def case(name, B=37):
    """The case's (cfg, params, xi, xv, y); shared between tests: read, never written."""
    return train_case(B=B, seed=SEEDS[name], **CASES[name])


def ragged_case(name, B):
    """Rows 1 .. B of the case (row 1 is a y = 0 sample: at B = 1 a saturated y = 1 row alone would leave every
    gradient exactly 0); the samples stay the ones the case's seed was chosen for."""
    cfg, params, xi, xv, y = case(name)
    return cfg, params, xi[1:1 + B], xv[1:1 + B], y[1:1 + B]


def dropout_case(seed, p, B=37):
    """The train_small_mlp golden's model and its first B rows labelled 0, with the kernels' counter-hash masks of
    `seed` at rate p: (cfg, params, xi, xv, y, masks).  (The golden's logits reach 40: on a row labelled 1
    sigmoid(z) - 1 is below fp32's resolution of 1, and a table row only such a sample reads has no fp32 gradient to
    compare per row -- the fp32 port itself is off by 100 % there.)"""
    from conftest import load_train_golden
    cfg, params, xi, xv, y, *_ = load_train_golden("train_small_mlp")
    rows = np.flatnonzero(y == 0)[:B]
    widths = [cfg["field_size"] * cfg["embedding_size"]] + [cfg["deep_nodes"]] * cfg["h_depth"]
    return cfg, params, xi[rows], xv[rows], y[rows], torch_port.dropout_masks(seed, p, B, widths)


def dropout_seed():
    """What train_forward draws next after torch.manual_seed(99), which the caller then sets again
    (test_gpu_train.test_train_step_with_dropout_matches_oracle_masks)."""
    torch.manual_seed(99)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
    torch.manual_seed(99)
    return seed


@functools.lru_cache(maxsize=None)
def reference(name, B=None):
    """(ref_step64, port_step at lr 1e-3, l2 3e-7) of a case (B None) or of its ragged slice, computed once."""
    cfg, params, xi, xv, y = case(name) if B is None else ragged_case(name, B)
    return ref_step64(cfg, params, xi, xv, y), port_step(cfg, params, xi, xv, y, 1e-3, 3e-7)
