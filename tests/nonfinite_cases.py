"""Helper (no tests): the models, the poison sites and the expected masks of the non-finite tests.

Two models over small tables (50 to 449 rows, the recipe of bf16_emul.sweep_case) and 40 input rows (two 16-row tiles
and a ragged 8, or a 32-row tile and 8):
  criteo   F = 39, 13 numerical, D = 10, 3 x 400, lw -- the static 25-chunk f32 kernel's only shape, inside the
           supported set of the fused bf16 and int8 forwards, N = 400 with its split 25th tile; also without a deep
           tower, with pruned hidden layers (the sparse MLP) and with a pruned field_cov (the pair list), and each of
           these again with QR tables (the quotient-row site);
  generic  F = 20, no numerical field, D = 8, N = 128, H = 2 -- the generic kernel forms, Xv of stride 0.
A site is one element of a parameter (or of Xv) that gets NaN, and +Inf where `inf` says so.  What a forward must give
comes from a CPU reference run on the poisoned model (expected): for NaN the reference's isnan mask, for +Inf its
non-finite mask.  Every case is built once, shared and never modified: poison() copies."""
import collections
import contextlib
import functools

import numpy as np

from conftest import model_kwargs

ROWS = 40
READERS = (3, 17, 38)  # the rows whose index reads the poisoned table row; no other row does
XV_ROW, XV_FIELD = 5, 3  # the Xv site
CAT, CAT_ROW, CAT_D = 2, 7, 4  # the plain table site: categorical field CAT (124 rows), row 7, element 4
QR_CAT, QR_Q = 5, 9  # the QR site: categorical field 5 (235 rows > qr_threshold), quotient row 9 = indices 36..39
NUM_F, NUM_D = 1, 2  # the numerical field whose v_f[0][d] is poisoned

SHAPES = dict(criteo=(39, 13, 10, 400, 3), generic=(20, 0, 8, 128, 2))

# scope: "row" (XV_ROW alone), "reads" (READERS), "all"
Site = collections.namedtuple("Site", "name key index scope inf")


@functools.lru_cache(maxsize=None)
def case(shape="criteo", deep=True, qr=False, seed=77):
    """(cfg, params, xi, xv) of SHAPES[shape]; deep=False: the same model without its deep tower; qr: QR tables
    (mult, 4 collisions) for the tables above 200 rows, as the golden deepfwfm_qr_mult has them."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    F, num, D, N, H = SHAPES[shape]
    sizes = [1] * num + [int(x) for x in 50 + (np.arange(F - num) * 37) % 400]
    cfg = dict(field_size=F, feature_sizes=sizes, embedding_size=D, use_fwfm=1, use_fm=0, use_logit=0,
               use_deep=int(deep), use_lw=1, use_fwlw=0, h_depth=H, deep_nodes=N, numerical=num,
               embedding_bag=int(qr), qr_flag=int(qr), qr_operation="mult", qr_collisions=4, qr_threshold=200)
    shapes = {k: tuple(v.shape) for k, v in DeepFMs(**model_kwargs(cfg)).state_dict().items()}
    params = synth.synth_state(shapes, F, D, N, True, bool(deep), seed=seed)
    xi, xv = synth.synth_inputs(sizes, num, ROWS, seed=seed)
    xi = xi.copy()
    for cat, hit in ((CAT, [CAT_ROW] * 3), (QR_CAT, [4 * QR_Q, 4 * QR_Q + 1, 4 * QR_Q + 3])):
        poisoned = set(range(4 * QR_Q, 4 * QR_Q + 4)) if cat == QR_CAT else {CAT_ROW}
        for b in range(ROWS):
            if int(xi[b, cat]) in poisoned:
                xi[b, cat] = 0
        xi[list(READERS), cat] = hit
    for v in params.values():
        v.setflags(write=False)
    xi.setflags(write=False)
    xv.setflags(write=False)
    return cfg, params, xi, xv


@functools.lru_cache(maxsize=None)
def pruned_mlp_case(qr=False):
    """case('criteo', qr=qr) with its hidden layers magnitude-pruned to a tenth, one row of each left empty and one of
    layer 1 dense, as test_gpu_sparse._pruned_case prunes them: the sparse MLP's lists run from 0 to the full width."""
    cfg, params, xi, xv = case("criteo", qr=qr)
    params = {k: v.copy() for k, v in params.items()}
    rng = np.random.default_rng(0)
    for h in range(1, cfg["h_depth"] + 1):
        w = params[f"net_1_linear_{h}.weight"]
        w[np.abs(w) < np.quantile(np.abs(w), 0.9)] = 0.0
        w[rng.integers(1, cfg["deep_nodes"] - 1)] = 0.0
    params["net_1_linear_1.weight"][5] = 0.5
    for v in params.values():
        v.setflags(write=False)
    return cfg, params, xi, xv


@functools.lru_cache(maxsize=None)
def pruned_pairs_case(qr=False):
    """case('criteo', deep=False, qr=qr) with field_cov pruned to 8 % of its pairs by the reference's symmetric mask,
    as test_gpu_shallow._prune_r prunes it, and the pairs that the sites need kept."""
    cfg, params, xi, xv = case("criteo", deep=False, qr=qr)
    params = {k: v.copy() for k, v in params.items()}
    W = params["field_cov.weight"]
    sym = np.abs(0.5 * (W + W.T))
    iu = np.triu_indices(W.shape[0], 1)
    W[sym < np.quantile(sym[iu], 0.92)] = 0.0
    f = cfg["numerical"] + CAT
    for k, l in ((NUM_F, f), (XV_FIELD, f), (NUM_F, cfg["numerical"] + QR_CAT)):  # the poisoned fields meet in kept pairs
        W[k, l] = W[l, k] = 0.25
    for v in params.values():
        v.setflags(write=False)
    return cfg, params, xi, xv


def sites(cfg):
    """The sites of a model, NaN each; +Inf too where .inf."""
    F, num, D, N, H = (cfg[k] for k in ("field_size", "numerical", "embedding_size", "deep_nodes", "h_depth"))
    f = num + CAT
    out = []
    if num:
        out.append(Site("Xv", "Xv", (XV_ROW, XV_FIELD), "row", True))
    out.append(Site("table2", f"fm_2nd_embeddings.{f}.weight", (CAT_ROW, CAT_D), "reads", True))
    if cfg["qr_flag"]:
        out.append(Site("table2_qr", f"fm_2nd_embeddings.{num + QR_CAT}.weight_q", (QR_Q, CAT_D), "reads", True))
    out.append(Site("table1", f"fm_1st_embeddings.{f}.weight", (CAT_ROW, 0), "reads", True))
    if num:
        out.append(Site("v_num", f"fm_2nd_embeddings.{NUM_F}.weight", (0, NUM_D), "all", False))
    out.append(Site("field_cov", "field_cov.weight", (NUM_F if num else 1, f), "all", False))
    out.append(Site("lw", "fm_1st.weight", (0, 6), "all", True))
    if cfg["use_deep"]:
        for l in sorted({1, (H + 1) // 2, H}):
            K = F * D if l == 1 else N
            for n in (0, N - 1):
                for k in (0, K - 1):
                    out.append(Site(f"W{l}[{n},{k}]", f"net_1_linear_{l}.weight", (n, k), "all", False))
            out.append(Site(f"b{l}", f"net_1_linear_{l}.bias", (N - 1 if l > 1 else 1,), "all", l == H))
        out.append(Site("fc", "net_1_fc.weight", (0, N - 1), "all", True))
    out.append(Site("bias", "bias", (0,), "all", True))
    return out


def site_values(site):
    return [np.float32(np.nan)] + ([np.float32(np.inf)] if site.inf else [])


def site_rows(site):
    """The rows a site may touch (bool [ROWS])."""
    m = np.zeros(ROWS, dtype=bool)
    if site.scope == "row":
        m[XV_ROW] = True
    elif site.scope == "reads":
        m[list(READERS)] = True
    else:
        m[:] = True
    return m


def poison(params, xv, site, value):
    """(params, xv) with the site's element set to value: copies, the rest shared."""
    if site.key == "Xv":
        xv = np.array(xv, dtype=np.float32)
        xv[site.index] = value
        return params, xv
    params = dict(params)
    w = np.array(params[site.key], dtype=np.float32)
    w[site.index] = value
    params[site.key] = w
    return params, xv


def expected(ref, cfg, params, xi, xv, site, value):
    """The mask a forward must show for this site and value, from the CPU reference ref(cfg, params, xi, xv) alone:
    isnan for a NaN, not-finite for +Inf."""
    p2, xv2 = poison(params, xv, site, value)
    with np.errstate(all="ignore"):
        out = np.asarray(ref(cfg, p2, xi, xv2))
    return np.isnan(out) if np.isnan(value) else ~np.isfinite(out)


def reaches_logit(cfg, params, xi, xv, site, value):
    """Whether the poison reaches every row of its scope when a value is read only through nonzero entries (a NaN is
    itself nonzero): the sparse MLP's lists, then the pruned FwFM pair list -- bool [ROWS] of rows reached.  The
    first order, lw, fc and bias are dense on every path."""
    F, num, D, N, H = (cfg[k] for k in ("field_size", "numerical", "embedding_size", "deep_nodes", "h_depth"))
    p2, xv2 = poison(params, xv, site, value)
    from oracle import dfwfm_oracle
    with np.errstate(all="ignore"):
        _, parts = dfwfm_oracle.forward(cfg, p2, xi, xv2, return_parts=True)
        hit = ~np.isfinite(parts["first"])
        bad = ~np.isfinite(parts["E"])  # [B, F, D]
        R = np.asarray(p2["field_cov.weight"], dtype=np.float64)
        kept = np.triu((0.5 * (R + R.T)) != 0, 1)  # a NaN compares unequal to 0: kept
        kept = kept | kept.T
        hit = hit | (bad.any(axis=2)[:, :, None] & kept[None]).any(axis=(1, 2))
        hit = hit | (np.isnan(0.5 * (R + R.T))[np.triu_indices(F, 1)]).any()
        if cfg["use_deep"]:
            t = bad.reshape(ROWS, F * D)
            for l in range(1, H + 1):
                W = np.asarray(p2[f"net_1_linear_{l}.weight"])
                b = np.asarray(p2[f"net_1_linear_{l}.bias"])
                nz = (W != 0).astype(np.int64)
                t = ((t.astype(np.int64) @ nz.T) > 0) | ~np.isfinite(W).all(axis=1)[None, :] | ~np.isfinite(b)[None, :]
            fc = np.asarray(p2["net_1_fc.weight"])[0]
            hit = hit | (t & (fc != 0)[None, :]).any(axis=1) | ~np.isfinite(fc).all()
        hit = hit | ~np.isfinite(np.asarray(p2["bias"], dtype=np.float64)[0])
    return hit


# -- running a path over every site ----------------------------------------------------------------------------------
CASES = dict(criteo=lambda: case("criteo"), generic=lambda: case("generic"), criteo_qr=lambda: case("criteo", qr=True),
             criteo_shallow=lambda: case("criteo", deep=False), generic_shallow=lambda: case("generic", deep=False),
             criteo_pruned_mlp=pruned_mlp_case, criteo_pruned_pairs=pruned_pairs_case,
             criteo_qr_shallow=lambda: case("criteo", deep=False, qr=True),
             criteo_qr_pruned_mlp=lambda: pruned_mlp_case(qr=True),
             criteo_qr_pruned_pairs=lambda: pruned_pairs_case(qr=True))


def reference(name):
    """The CPU reference of a family of paths: f32 (the float64 oracle), bf16, bf16_fold, int8 (the contracts)."""
    import bf16_emul
    import bf16_fold_emul
    import int8_emul
    from oracle import dfwfm_oracle
    return dict(f32=dfwfm_oracle.forward, bf16=bf16_emul.forward, bf16_fold=bf16_fold_emul.forward,
                int8=int8_emul.forward)[name]


@functools.lru_cache(maxsize=None)
def expected_masks(case_name, ref_name):
    """{(site name, 'nan' | 'inf'): mask} of a case under a reference; computed once, shared, never modified."""
    cfg, params, xi, xv = CASES[case_name]()
    ref = reference(ref_name)
    return {(s.name, "nan" if np.isnan(v) else "inf"): expected(ref, cfg, params, xi, xv, s, v)
            for s in sites(cfg) for v in site_values(s)}


@contextlib.contextmanager
def poisoned_module(m, site, value):
    """The module's own parameter edited in place (under no_grad: its version moves, the engines follow it), and
    restored."""
    import torch
    if site.key == "Xv":
        yield
        return
    p = m.get_parameter(site.key)
    with torch.no_grad():
        old = p[site.index].clone()
        p[site.index] = float(value)
    try:
        yield
    finally:
        with torch.no_grad():
            p[site.index] = old


def check_path(forward, m, case_name, ref_name, what, no_inf=(), taken=None):
    """forward(xi, xv) -> the float32 logits of module m on one path.  Every site and value: the mask is the
    reference's, row by row, and the rows outside the site's scope keep the clean model's bits; afterwards the clean
    logits are back.  no_inf: site names that get no +Inf on this path.  taken() -> whether the engine took the path
    meant, asked after every forward while its poison is still in place (a poisoned parameter must not send the
    forward quietly down another route).  Every miss is reported, not the first."""
    cfg, params, xi, xv = CASES[case_name]()
    masks = expected_masks(case_name, ref_name)
    clean = np.asarray(forward(xi, xv))
    assert clean.dtype == np.float32 and clean.shape == (ROWS,) and np.isfinite(clean).all(), what
    assert taken is None or taken(), what
    missed, cells = [], 0
    for s in sites(cfg):
        rows = site_rows(s)
        for v in site_values(s):
            kind = "nan" if np.isnan(v) else "inf"
            if kind == "inf" and s.name in no_inf:
                continue
            want = masks[s.name, kind]
            assert want.any() and not want[~rows].any(), (what, s.name, kind)  # the reference itself: live and local
            _, xv2 = poison(params, xv, s, v)
            with poisoned_module(m, s, v):
                got = np.asarray(forward(xi, xv2))
                on = taken is None or bool(taken())
            mask = np.isnan(got) if kind == "nan" else ~np.isfinite(got)
            cells += 1
            if not on:
                missed.append((s.name, kind, "another route was taken"))
            elif not np.array_equal(mask, want):
                missed.append((s.name, kind, "mask differs in rows", np.flatnonzero(mask != want).tolist()))
            elif not np.array_equal(got[~rows], clean[~rows]):
                missed.append((s.name, kind, "untouched rows moved", np.flatnonzero(~rows & (got != clean)).tolist()))
    assert not missed, (what, missed)
    assert np.array_equal(np.asarray(forward(xi, xv)), clean), what  # restored
    return cells
