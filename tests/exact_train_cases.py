"""Exact-arithmetic witness of the training step: models and batches on which every float32 product and every partial
sum of the forward AND of the backward is a float32, whatever the order of summation.  On them the logits and every
element of every gradient must equal a float64 reference bit for bit -- atomic sums included -- so one dropped,
duplicated or misplaced term of any size fails (tests/test_exact_train_cases.py: the CPU leg -- certificate,
non-degeneracy, mutations, host kernels; tests/test_gpu_exact_train.py: every HIP route).

The backward is fed a dlogit we choose (no loss in front of it), so nothing here is conditioned by sigmoid(z) - y.

Values.  Tables and Xv are small integers; R (not symmetric), lw, fwfm_linear, fc come from {0, +-1, +-0.5}; hidden
layers have NNZ nonzeros per row from {+-1, +-0.5} (magnitudes grow by a bounded factor per layer) and nonzero biases;
dlogit comes from a few signed powers of two and 0.  Dropout at p = 0.5 scales by 2 and stays exact.

Certificate.  Every output (logit, gradient element) is a multilinear form in the parameters, Xv and dlogit.  Run on
the absolute values of all of them (masks and the x2 kept; the second-order term as the full, unhalved Gram sum with
its diagonal kept in: _full_gram_excess), the same graph bounds every partial sum of every factorisation of those
forms.  Every such partial sum is a multiple of the output's quantum q, a
power of two derived from the operands' own quanta (quantum(): the largest power of two <= 1 that divides a tensor's
values).  bound / q < 2^24 then says that every partial sum is an integer multiple of q below 2^24 q: a float32.

The saturated variant (saturated()) puts the loss back for the fused-loss routes without giving up exactness: one
first-order table (and its lw weight) is scaled so that every |z| >= 128, where any float32 formulation of the
sigmoid gives exactly 0 or 1 and log1p(exp(-|z|)) exactly 0; with denom = B = 128 dlogit is in {0, +-2^-7} and the
per-sample loss is max(z, 0) - z y."""
import functools
from typing import NamedTuple, Optional

import numpy as np
import torch

import train_cases as tc
from oracle import torch_port

NNZ = 6  # nonzeros per hidden row
# row b takes entry b % len: ordered so that no batch size in use sums to 0 (the bias gradient) and that the last row
# of every batch (a ragged tile's, a one-row last split's) carries a gradient
DL_FULL = (2.0 ** -3, 2.0 ** -2, -2.0 ** -3, 0.0, -2.0 ** -4, 2.0 ** -4, -2.0 ** -2)
DL_FEW = (2.0 ** -3, -2.0 ** -3, 0.0, 2.0 ** -3)  # the 4097-row case: a hot row sums 1400 samples
LIMIT = 2.0 ** 24
CHUNK = 512  # the reference runs the port's [F, F, B, D] outer product over slices of the batch (sums stay exact)
SAT_Z, SAT_B, SAT_LW = 128.0, 128, 128.0
SGD_LR = 2.0 ** -6


class Case(NamedTuple):
    cfg: dict
    params: dict
    xi: np.ndarray
    xv: np.ndarray
    dlogit: np.ndarray
    masks: Optional[list]  # torch bool [B, width] per layer 0 .. H, or None (no dropout)
    seed: int              # the counter-hash seed of the masks


def drop_p(case):
    return 0.5 if case.masks is not None else 0.0


def widths(cfg):
    return [cfg["field_size"] * cfg["embedding_size"]] + [cfg["deep_nodes"]] * cfg["h_depth"]


def _pick(rng, values, shape, p=None):
    return rng.choice(np.asarray(values, np.float32), size=shape, p=p).astype(np.float32)


def fill_params(params, cfg, rng, emax=2, nnz=NNZ):
    """The case's parameter values, by name, over train_case's shapes."""
    ints = np.arange(-emax, emax + 1)
    out = {}
    for k, v in params.items():
        if "embeddings" in k:
            w = rng.choice(ints, size=v.shape).astype(np.float32)
            if k.startswith("fm_1st_embeddings") or k.endswith("weight_r"):
                w[w == 0] = 1.0  # a first-order weight / a remainder row of 0 would silence its sample
        elif k == "field_cov.weight":
            w = _pick(rng, (0.0, 1.0, -1.0, 0.5, -0.5), v.shape)
            w[0, 1], w[1, 0] = 1.0, -0.5  # not symmetric, whatever the draw
        elif k in ("fwfm_linear.weight", "fm_1st.weight", "net_1_fc.weight"):
            w = _pick(rng, (1.0, -1.0, 0.5, -0.5), v.shape)
        elif k == "bias":
            w = np.full(v.shape, 1.5, np.float32)
        elif k.endswith(".bias"):
            w = _pick(rng, (1.0, -1.0, 0.5, -0.5), v.shape)
        elif k.startswith("net_1_linear_"):
            w = np.zeros(v.shape, np.float32)
            for r in range(v.shape[0]):
                cols = rng.choice(v.shape[1], size=min(nnz, v.shape[1]), replace=False)
                w[r, cols] = _pick(rng, (1.0, -1.0, 0.5, -0.5), len(cols))
        else:
            raise AssertionError(f"exact_train_cases: no value set for parameter {k}")
        out[k] = w
    return out


def fill_indices(cfg, B, rng):
    """Xi [B, ncat]: uniform over the lower three fifths of each table (the rest stays untouched), then per field a row
    read by three samples (row 0, at rows j .. j + 2 of the batch) and the table's last row read once (row j + 3), and
    on the first categorical field a hot row (row 1) read by every second sample."""
    num = cfg["numerical"]
    n = np.asarray(cfg["feature_sizes"][num:], np.int64)
    xi = np.zeros((B, len(n)), np.int64)
    for j, m in enumerate(n):
        xi[:, j] = rng.integers(0, m if m <= 7 else -(-3 * m // 5), B)  # (a tiny table: every row)
        if B >= 8:
            xi[(j + np.arange(3)) % B, j] = 0
            xi[(j + 3) % B, j] = m - 1
    if len(n) and n[0] > 1:
        xi[::2, 0] = 1
    return xi


@functools.lru_cache(maxsize=None)
def exact_case(F, num, D, N, H, kind="fwfm", deep=1, lw=1, fwlw=0, qr=0, op="mult", embbag=0, B=129, seed=1,
               drop=False, sizes=None, c=4, threshold=200, dl=DL_FULL, emax=2, xvmax=3, nnz=NNZ, drop_seed=None):
    """A Case in train_cases.train_case's vocabulary; shared between tests: read, never written.  drop_seed None:
    train_cases.dropout_seed(), what the autograd route's train_forward draws after torch.manual_seed(99)."""
    if drop_seed is None:
        drop_seed = tc.dropout_seed()
    cfg, shapes, _, xv0, _ = tc.train_case(F, num, D, N, H, kind=kind, deep=deep, lw=lw, fwlw=fwlw, qr=qr, op=op,
                                           embbag=embbag, B=B, seed=seed, sizes=sizes, c=c, threshold=threshold)
    rng = np.random.default_rng(1000 + seed)
    params = fill_params(shapes, cfg, rng, emax, nnz)
    xi = fill_indices(cfg, B, rng)
    xv = rng.integers(0, xvmax + 1, xv0.shape).astype(np.float32)
    dlogit = np.asarray([dl[b % len(dl)] for b in range(B)], np.float32)
    for f in np.flatnonzero(dlogit.astype(np.float64) @ xv == 0):
        xv[0, f] += 1.0  # sum_b dlogit_b Xv_bf is the field's first-order gradient: not 0 by chance (dlogit_0 != 0)
    masks = torch_port.dropout_masks(drop_seed, 0.5, B, widths(cfg)) if (drop and deep) else None
    for a in list(params.values()) + [xi, xv, dlogit]:
        a.setflags(write=False)
    return Case(cfg, params, xi, xv, dlogit, masks, drop_seed)


def head(case, B):
    """The first B rows of a case (the dropout masks are a function of the row, so they are the first B rows' too)."""
    masks = None if case.masks is None else [m[:B] for m in case.masks]
    return case._replace(xi=case.xi[:B], xv=case.xv[:B], dlogit=case.dlogit[:B], masks=masks)


# ------------------------------------------------------------------------------------------------- the named cases
BASE = dict(F=39, num=13, D=10, N=400, H=3)  # Criteo-39: FwFM + deep + lw, 13 numerical fields
BASE_B = (1, 16, 17, 129)                    # the tile edges; 129: two split-K slices with a 1-row last split
VARIANTS = {k: tc.CASES[k] for k in ("fm_deep", "logit", "fwfm_shallow_lw", "fwlw_lw", "qr_add", "embbag", "num0",
                                     "allnum", "f64")}
VARIANTS["qr_mult"] = dict(tc.CASES["qr_add"], op="mult")
VARIANTS["h1"] = dict(BASE, H=1)  # one hidden layer of 400: the smallest shape the helper-wave training forward takes
VARIANT_B = 37
# the 4097-row case: the smallest model the scatter takes; one field whose every sample hits one of 3 rows, one with
# all-distinct rows; a second pass of the sorted scatter (4096 samples a pass) that holds one sample
HOT = dict(F=39, num=13, D=4, N=64, H=2)
HOT_B = 4097
HOT_SIZES = (3, 5000, 7, 60, 500) + (5000,) * 21


@functools.lru_cache(maxsize=None)
def base_case(B=129, drop=False):
    return head(exact_case(B=129, drop=drop, **BASE), B)


def variant_case(name, drop=False):
    return exact_case(B=VARIANT_B, drop=drop, **VARIANTS[name])


@functools.lru_cache(maxsize=None)
def hot_case():
    case = exact_case(B=HOT_B, sizes=HOT_SIZES, dl=DL_FEW, emax=1, xvmax=1, **HOT)
    xi = case.xi.copy()
    xi[:, 1] = np.arange(HOT_B)  # every sample its own row
    xi.setflags(write=False)
    return case._replace(xi=xi)


def all_cases():
    """{name: Case} of everything the legs run (the ragged heads of the base case are prefixes of base-129)."""
    out = {"base-129": base_case(), "base-129-drop": base_case(drop=True), "hot-4097": hot_case(),
           "sat-128": saturated().case}
    out.update({f"{k}-37": variant_case(k) for k in VARIANTS})
    return out


# ------------------------------------------------------------------------------------------------- the reference
def _leaves(params, dtype, absolute=False):
    return {k: torch.tensor(np.abs(v) if absolute else v, dtype=dtype, requires_grad=True) for k, v in params.items()}


def _run(case, dtype, absolute=False, rows=None):
    """(logits, grads) of forward_graph + out.backward(dlogit) at dtype, over the batch in slices of CHUNK rows
    (the gradients of the slices are added: exact where the whole is), optionally on absolute values, optionally over
    the rows `rows` only (an index array: the batch in another order)."""
    cfg, params = case.cfg, case.params
    B = len(case.xi)
    order = np.arange(B) if rows is None else np.asarray(rows)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    logits = np.zeros(B, npdt)
    grads = {k: np.zeros(v.shape, npdt) for k, v in params.items()}
    for lo in range(0, len(order), CHUNK):
        r = order[lo:lo + CHUNK]
        leaf = _leaves(params, dtype, absolute)
        xv = np.abs(case.xv[r]) if absolute else case.xv[r]
        dl = np.abs(case.dlogit[r]) if absolute else case.dlogit[r]
        masks = None if case.masks is None else [m[torch.as_tensor(r)] for m in case.masks]
        xi_t, xv_t = torch.as_tensor(tc.port_xi(case.xi[r])), torch.as_tensor(xv, dtype=dtype)
        out = torch_port.forward_graph(cfg, leaf, xi_t, xv_t, masks, drop_p(case))
        if absolute:
            out = out + _full_gram_excess(cfg, leaf, xi_t, xv_t)
        out.backward(torch.as_tensor(dl, dtype=dtype))
        logits[r] = out.detach().numpy()
        for k, v in leaf.items():
            if v.grad is not None:
                grads[k] += v.grad.numpy()
    return logits, grads


def _full_gram_excess(cfg, leaf, xi, xv):
    """What the absolute-value graph adds to the port's second-order term so that the bound is the FULL, unhalved
    Gram sum S = sum_{k, l} Rsym[k][l] <e_k, e_l>, diagonal kept in.  The port forms (S - diag) / 2, but it sums all
    of S first (outer.sum(0).sum(0)), and a kernel may form (sum e)^2 - sum e^2: S itself is a partial sum of some
    factorisations, and its gradient 2 Rsym e (diagonal included) of the embedding gradients'.  S - (S - diag) / 2 =
    (S + diag) / 2."""
    if not (cfg["use_fwfm"] or cfg["use_fm"]):
        return 0.0
    E = torch.stack(torch_port._field_embeddings(cfg, leaf, xi.reshape(xi.shape[0], -1), xv, "fm_2nd_embeddings"))
    if cfg["use_fwfm"]:
        W = leaf["field_cov.weight"]
        rs = (W.t() + W) * 0.5
        full = torch.einsum("kbd,lbd,kl->b", E, E, rs)
        diag = torch.einsum("kbd,kbd,k->b", E, E, torch.diagonal(rs))
    else:
        full = (E.sum(0) ** 2).sum(1)
        diag = (E ** 2).sum((0, 2))
    return (full + diag) * 0.5


def ref64(case):
    """(logits, {name: gradient}) in float64: torch_port.forward_graph on float64 leaves, then out.backward(dlogit).
    A parameter autograd leaves without a gradient gets zeros."""
    return _cached_ref(_key(case))


_CASES = {}


def _key(case):
    k = tuple(id(x) for x in (case.cfg, case.params, case.xi, case.xv, case.dlogit, case.masks)) + (case.seed,)
    _CASES[k] = case  # (keeps the arrays alive, so the ids stay theirs)
    return k


@functools.lru_cache(maxsize=None)
def _cached_ref(key):
    return _run(_CASES[key], torch.float64)


def port32(case, reverse=False):
    """The float32 port on the same graph; reverse: the batch in reverse order (logits returned in case order)."""
    rows = np.arange(len(case.xi))[::-1].copy() if reverse else None
    logits, grads = _run(case, torch.float32, rows=rows)
    return logits.astype(np.float32), {k: np.asarray(g, np.float32) for k, g in grads.items()}


def ref32(case):
    """ref64 cast to float32 (exact by the certificate): what every kernel route must return, bit for bit."""
    z, g = ref64(case)
    z32, g32 = z.astype(np.float32), {k: v.astype(np.float32) for k, v in g.items()}
    assert np.array_equal(z32.astype(np.float64), z) and all(np.array_equal(g32[k].astype(np.float64), g[k]) for k in g)
    return z32, g32


# ------------------------------------------------------------------------------------------------- the certificate
def quantum(*arrays):
    """The largest power of two <= 1 that divides every value of the arrays (all of them dyadic)."""
    q = 1.0
    for a in arrays:
        a = np.abs(np.asarray(a, np.float64)).ravel()
        a = a[a != 0]
        while a.size and np.any(a / q != np.floor(a / q)):
            q /= 2.0
            assert q >= 2.0 ** -40, "not dyadic"
    return q


def quanta(case, lr=None):
    """{output: quantum}: 'logits' and every parameter's gradient (with lr: 'sgd:' + name for p - lr g too).  Tables
    and Xv are integers (asserted), so an embedding has quantum 1 and a part's quantum is the product of its dense
    operands' quanta; a gradient's is q(dlogit) x the finest part its parameter feeds / the parameter's own quantum."""
    cfg, P = case.cfg, case.params
    for k, v in P.items():
        if "embeddings" in k:
            assert quantum(v) == 1.0, k
    assert quantum(case.xv) == 1.0
    q = {k: quantum(v) for k, v in P.items()}
    q_dl = quantum(case.dlogit)
    shallow2 = cfg["use_fwfm"] or cfg["use_fm"]
    q_lw = q["fm_1st.weight"] if (cfg["use_lw"] and shallow2) else 1.0
    q_first = (q["fwfm_linear.weight"] if (cfg["use_fwlw"] and shallow2) else 1.0) * q_lw
    parts = {"first": q_first}
    if shallow2:  # (R + R^T) / 2, then the halved sum
        parts["second"] = (q["field_cov.weight"] / 4.0) if cfg["use_fwfm"] else 0.5
    if cfg["use_deep"]:
        qh = 1.0
        for i in range(1, cfg["h_depth"] + 1):
            qh = min(qh * q[f"net_1_linear_{i}.weight"], q[f"net_1_linear_{i}.bias"])
        parts["deep"] = qh * q["net_1_fc.weight"]
    q_bias = quantum(P["bias"])
    out = {"logits": min(min(parts.values()), q_bias)}
    for k in P:
        if k == "bias":
            feeds = [1.0]
        elif k.startswith("fm_1st_embeddings"):
            feeds = [parts["first"]]
        elif k.startswith("fm_2nd_embeddings"):
            feeds = [parts[p] for p in ("second", "deep") if p in parts]
            feeds += [parts["first"]] if cfg["use_fwlw"] else []
        elif k in ("fm_1st.weight", "fwfm_linear.weight"):
            feeds = [parts["first"]]
        elif k == "field_cov.weight":
            feeds = [parts["second"]]
        else:
            feeds = [parts["deep"]]
        # (dividing by the parameter's own quantum: the form is linear in it, or quadratic in an integer table)
        out[k] = q_dl if k == "bias" else q_dl * min(feeds) / q[k]
        if lr is not None:
            out["sgd:" + k] = min(q[k], lr * out[k])
    return out


def bounds(case):
    """{output: bound}: the graph on the absolute values of every parameter, of Xv and of dlogit, with the second-order
    term as the full unhalved Gram sum, diagonal kept in (_full_gram_excess)."""
    z, g = _run(case, torch.float64, absolute=True)
    out = {"logits": float(z.max())}
    out.update({k: float(v.max(initial=0.0)) for k, v in g.items()})
    return out


def certificate(case, lr=None):
    """{output: bound / quantum}, each of which must stay below 2^24 (LIMIT)."""
    b, q = bounds(case), quanta(case, lr)
    out = {k: b[k] / q[k] for k in b}
    if lr is not None:
        for k, v in case.params.items():
            out["sgd:" + k] = (float(np.abs(v).max()) + lr * b[k]) / q["sgd:" + k]
    return out


# ------------------------------------------------------------------------------------------------- saturated variant
class Saturated(NamedTuple):
    case: Case            # dlogit is the exact (sigmoid(z) - y) / B
    y: np.ndarray         # labels
    loss_sum: float       # sum of max(z, 0) - z y
    field: int            # the field whose first-order table is scaled
    big: float


@functools.lru_cache(maxsize=None)
def saturated():
    """The base model at B = 128 with one categorical field's first-order table set to +-big by row parity, big the
    power of two that exceeds the rest of the logit's bound by SAT_Z; every third sample is labelled against its
    logit (both signs occur), so dlogit is in {0, +-1/128}."""
    base = exact_case(B=SAT_B, emax=1, xvmax=1, nnz=4, seed=2, **BASE)
    f = base.cfg["numerical"] + 1
    k = f"fm_1st_embeddings.{f}.weight"
    params = dict(base.params)
    params[k] = np.zeros_like(base.params[k])
    # the logits' signs are the scaled table's (+ on even rows), so dlogit is known before the logits are
    up = base.xi[:, f - base.cfg["numerical"]] % 2 == 0
    flip = np.arange(SAT_B) % 3 == 1  # rows 1, 4 .. 127: the last row too
    y = np.where(flip, ~up, up).astype(np.float32)
    dl = (up.astype(np.float64) - y) / SAT_B
    xv = base.xv.copy()
    for col in np.flatnonzero(dl @ xv == 0):
        xv[1, col] += 1.0  # a numerical field's first-order gradient, sum_b dlogit_b Xv_bf, not 0 by chance
    xv.setflags(write=False)
    base = base._replace(xv=xv)
    rest = bounds(base._replace(params=params))["logits"]
    big = 2.0 ** np.ceil(np.log2(rest + SAT_Z))
    # the factor is split between the table (+-big / SAT_LW) and its lw weight (SAT_LW): p - lr g of a table entry of
    # size big itself, whose gradient's quantum is 2^-7, would need 28 bits at lr = 2^-6
    rows = np.arange(len(params[k]))
    params[k] = (big / SAT_LW * np.where(rows % 2 == 0, 1.0, -1.0)).astype(np.float32).reshape(-1, 1)
    lwk = np.array(base.params["fm_1st.weight"])
    lwk[0, f] = SAT_LW
    params["fm_1st.weight"] = lwk
    for a in (params[k], lwk):
        a.setflags(write=False)
    case = base._replace(params=params)
    z, _ = _run(case, torch.float64)
    assert np.all(np.abs(z) >= SAT_Z) and np.array_equal(z > 0, up)
    loss = float(np.sum(np.maximum(z, 0.0) - z * y))
    dl32 = dl.astype(np.float32)
    dl32.setflags(write=False)
    y.setflags(write=False)
    return Saturated(case._replace(dlogit=dl32), y, loss, f, float(big))


def saturated_certificate(sat, lr=SGD_LR):
    """certificate() of the saturated case with p - lr g, and the loss sum's: sum |z| over the samples labelled
    against their logit, over the logits' quantum."""
    cert = certificate(sat.case, lr)
    z, _ = ref64(sat.case)
    cert["loss_sum"] = float(np.abs(z)[sat.case.dlogit != 0].sum()) / quanta(sat.case)["logits"]
    return cert


def sgd_ref(sat, lr=SGD_LR):
    """{name: p - lr g} in float64 cast to float32 (exact by saturated_certificate)."""
    _, g = ref64(sat.case)
    out = {}
    for k, p in sat.case.params.items():
        v = p.astype(np.float64) - lr * g[k]
        out[k] = v.astype(np.float32)
        assert np.array_equal(out[k].astype(np.float64), v), k
    return out


# ------------------------------------------------------------------------------------------------- mutations
def _embeddings(case):
    """The second-order field embeddings [B, F, D] in float64 (numpy)."""
    cfg, P = case.cfg, case.params
    num, c = cfg["numerical"], cfg["qr_collisions"]
    out = []
    for f in range(cfg["field_size"]):
        pre = f"fm_2nd_embeddings.{f}."
        if f < num:
            e = P[pre + "weight"][0][None, :].astype(np.float64) * case.xv[:, f:f + 1]
        elif pre + "weight" in P:
            e = P[pre + "weight"][case.xi[:, f - num]].astype(np.float64)
        else:
            eq = P[pre + "weight_q"][case.xi[:, f - num] // c].astype(np.float64)
            er = P[pre + "weight_r"][case.xi[:, f - num] % c].astype(np.float64)
            e = eq * er if cfg["qr_operation"] == "mult" else eq + er
        out.append(e)
    return np.stack(out, 1)


def deep_tower64(case, skip_x2_bwd=None, relu_from_prev_width=None, drop_last_row_of=None, no_mask_bwd=False):
    """The deep tower's weight and bias gradients by hand in float64 (numpy), with a kernel's plausible slips:
    skip_x2_bwd = h: the backward leaves out dropout layer h's x2; no_mask_bwd: the backward applies no dropout at
    all (masks and x2 in the forward only); relu_from_prev_width = h: layer h's ReLU mask is
    read from the flat [B, width] pre-activations with layer h - 1's width as the row stride; drop_last_row_of = h:
    dW_h without the batch's last row.  Without a slip it reproduces ref64 (asserted by the CPU leg)."""
    cfg, P = case.cfg, case.params
    H, B = cfg["h_depth"], len(case.xi)
    m = [np.ones((B, w)) for w in widths(cfg)] if case.masks is None else [2.0 * x.numpy() for x in case.masks]
    mb = [x if skip_x2_bwd != i else x / 2.0 for i, x in enumerate(m)]
    if no_mask_bwd:
        mb = [np.ones_like(x) for x in m]
    h = [_embeddings(case).reshape(B, -1) * m[0]]
    live = []
    for i in range(1, H + 1):
        W, b = P[f"net_1_linear_{i}.weight"].astype(np.float64), P[f"net_1_linear_{i}.bias"].astype(np.float64)
        z = h[-1] @ W.T + b
        on = z > 0
        if relu_from_prev_width == i:
            flat = on.ravel()
            idx = np.arange(B)[:, None] * h[-1].shape[1] + np.arange(z.shape[1])[None, :]
            on = flat[np.minimum(idx, flat.size - 1)]
        live.append(on)  # what the backward reads; the forward below is the true ReLU
        h.append(np.maximum(z, 0.0) * m[i])
    dh = case.dlogit.astype(np.float64)[:, None] * P["net_1_fc.weight"].astype(np.float64)
    grads = {"net_1_fc.weight": (case.dlogit.astype(np.float64)[:, None] * h[-1]).sum(0, keepdims=True)}
    for i in range(H, 0, -1):
        dz = dh * mb[i] * live[i - 1]
        rows = slice(0, B - 1) if drop_last_row_of == i else slice(0, B)
        grads[f"net_1_linear_{i}.weight"] = dz[rows].T @ h[i - 1][rows]
        grads[f"net_1_linear_{i}.bias"] = dz.sum(0)
        dh = dz @ P[f"net_1_linear_{i}.weight"].astype(np.float64)
    return grads


def shared_row(case):
    """(parameter name, row, sample) of a second-order table row that several samples read."""
    num = case.cfg["numerical"]
    for j in range(case.xi.shape[1]):
        k = f"fm_2nd_embeddings.{num + j}.weight"
        rows, counts = np.unique(case.xi[:, j], return_counts=True)
        if k in case.params and counts.max() >= 2:
            r = int(rows[np.argmax(counts)])
            b = [int(x) for x in np.flatnonzero(case.xi[:, j] == r) if case.dlogit[x] != 0][0]
            return k, r, b
    raise AssertionError("no shared row")


def mutations(case):
    """{name: gradients (float64) of a reference that slips the way a kernel plausibly could}; each applies where the
    model has the part it slips in."""
    cfg = case.cfg
    _, g = ref64(case)
    out = {}
    if case.xi.shape[1] and any(k.startswith("fm_2nd_embeddings") for k in g):
        k, r, b = shared_row(case)
        dl1 = np.zeros_like(case.dlogit)
        dl1[b] = case.dlogit[b]
        _, g1 = _run(case._replace(dlogit=dl1), torch.float64)
        mut = dict(g)
        mut[k] = g[k].copy()
        mut[k][r] -= g1[k][r]
        out["one sample dropped from a shared table row"] = mut
    if cfg["use_fwfm"]:
        R = case.params["field_cov.weight"]
        raw = dict(case.params, **{"field_cov.weight": 2.0 * np.triu(R, 1)})  # pair (k, l), k < l, weighted R[k][l]
        out["R instead of (R + R^T) / 2"] = _run(case._replace(params=raw), torch.float64)[1]
    if cfg["use_deep"]:
        H = cfg["h_depth"]
        if case.masks is not None:
            out["x2 of one dropout layer skipped in the backward"] = dict(g, **deep_tower64(case, skip_x2_bwd=H))
            out["dropout in the forward only"] = dict(g, **deep_tower64(case, no_mask_bwd=True))
        out["ReLU mask taken at the previous layer's width"] = dict(g, **deep_tower64(case, relu_from_prev_width=1))
        out["last row of a ragged tile dropped from one dW"] = dict(g, **deep_tower64(case, drop_last_row_of=1))
    if cfg["qr_flag"] and cfg["qr_operation"] == "mult":
        k = next(k for k in g if k.startswith("fm_2nd_embeddings") and k.endswith("weight_r"))
        out["remainder-table half of a QR mult gradient dropped"] = dict(g, **{k: np.zeros_like(g[k])})
    return out


def differs(ga, gb):
    """Names of the tensors on which two gradient sets differ in at least one float32 bit."""
    return [k for k in ga if not np.array_equal(np.asarray(ga[k], np.float32), np.asarray(gb[k], np.float32))]
