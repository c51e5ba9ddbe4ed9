"""Shard plans of the data-parallel step on the exact-arithmetic witness (tests/exact_train_cases.py), and a host
emulation of its touched-row exchange (tests/test_dp_cases.py: the CPU leg; tests/test_gpu_dp_worlds.py: the kernels
on 1, 3, 4 and 8 emulated ranks through the C ABI, and FusedTrainStep on 3, 4 and 8 gloo ranks).

On a witness case every float32 sum is exact in any order, so W ranks' gradients on the shards of a batch, each
normalised by the global batch, add up to the float64 reference of the whole batch bit for bit -- whatever order the
lists are applied in and whatever order the all-reduce sums in.  One dropped, duplicated or misplaced list entry, one
skipped rank, one stale list applied again fails.

A shard plan is (world, per-rank batch): the shards are fit()'s (training._fit_loop: lo = min(end, offset + rank bs),
hi = min(end, lo + bs)), so trailing ranks of a last global batch hold fewer rows, or none."""
import functools

import numpy as np
import torch

import exact_train_cases as xc
import train_cases as tc

# ---- A: emulated ranks through the C ABI, on the 129-row cases: {plan: (world, per-rank batch)} and the sizes meant
A_B = 129
A_PLANS = {"w1": (1, 129), "w3": (3, 43), "w4-tail": (4, 64), "w8": (8, 17), "w8-front": (8, 129)}
A_SIZES = {"w1": [129], "w3": [43, 43, 43], "w4-tail": [64, 64, 1, 0], "w8": [17] * 7 + [10],
           "w8-front": [129] + [0] * 7}
A_MODELS = ("base", "qr_mult", "qr_add", "embbag", "fwlw_lw")  # plain, QR mult, QR add, EmbeddingBag, fwlw

# ---- B1: gloo ranks on the saturated case (128 rows): {plan: (world, per-rank batch)}
B1_PLANS = {"w3": (3, 43), "w4-even": (4, 32), "w4-front": (4, 64), "w4-middle": (4, 48), "w8-even": (8, 16),
            "w8-front": (8, 64)}
B1_SIZES = {"w3": [43, 43, 42], "w4-even": [32] * 4, "w4-front": [64, 64, 0, 0], "w4-middle": [48, 48, 32, 0],
            "w8-even": [16] * 8, "w8-front": [64, 64] + [0] * 6}

# ---- B2: gloo ranks on the train goldens: {world: (global batch, per-rank batch)}; then a 20-row global batch
B2_WORLDS = {3: (63, 21), 4: (64, 16), 8: (64, 8)}
B2_PARTIAL = 20
B2_PARTIAL_SIZES = {3: [20, 0, 0], 4: [16, 4, 0, 0], 8: [8, 8, 4, 0, 0, 0, 0, 0]}


def fit_shards(n_global, bs, world, offset=0):
    """[(lo, hi)] per rank of the global batch [offset, offset + n_global): training._fit_loop's rule."""
    end = offset + n_global
    out = []
    for rank in range(world):
        lo = min(end, offset + rank * bs)
        out.append((lo, min(end, lo + bs)))
    return out


def rate0_rows(rank, bs, n):
    """The rows a rank is fed in the two rate-0 steps of a B1 plan: bs rows of the batch taken cyclically from
    rank bs, so every rank holds a full batch (and a nonzero touched-row list in its send buffer) before the measured
    step, in which fit()'s shards leave some ranks partial or empty.  On an even plan they are the rank's own shard."""
    return (rank * bs + np.arange(bs)) % n


@functools.lru_cache(maxsize=None)
def a_case(name):
    """The 129-row witness case of a model of A_MODELS, without dropout (the masks are a function of the local row
    index: a shard's rows would draw other masks than the whole batch's)."""
    if name == "base":
        return xc.base_case(A_B, False)
    return xc.exact_case(B=A_B, **xc.VARIANTS[name])


def rows_of(case, rows):
    """The case on the rows `rows` (a slice or an index array); dlogit stays the global batch's."""
    assert case.masks is None
    return case._replace(xi=case.xi[rows], xv=case.xv[rows], dlogit=case.dlogit[rows])


def shard_grads64(case, lo, hi):
    """(logits, grads) of the float64 reference on rows lo .. hi - 1 (an empty shard: no logits, zero gradients)."""
    if hi == lo:
        return np.zeros(0), {k: np.zeros(v.shape) for k, v in case.params.items()}
    return xc._run(rows_of(case, slice(lo, hi)), torch.float64)


def table_names(case):
    """The categorical tables' parameter names that carry a gradient (both families, QR halves)."""
    _, g = xc.ref64(case)
    return [k for k in tc.table_rows(case.cfg, case.xi) if k in g]


def touched(case, lo, hi):
    """{table: sorted rows that the shard lo .. hi - 1 reads}."""
    names = set(table_names(case))
    return {k: np.flatnonzero(m) for k, m in tc.table_rows(case.cfg, case.xi[lo:hi]).items() if k in names}


# ---- the exchange on the host: what training._apply_sparse and dfwfm_sparse_grads_local do, in float64 -------------
MUTATIONS = ("skip the last rank's slot", "apply rank 1's slot twice", "no count reset on an empty shard")


def emulate_exchange(case, shards, stale=None, mutation=None):
    """{table: gradient} of the tables after the exchange over `shards`: every rank turns its shard's dense table
    gradients into one list per table of (row, gradient row) over the rows it touched -- into a slot that still holds
    the list of a previous step on the rows stale[rank] (index arrays; None: the first shard's rows on every rank) --
    and every slot is applied in rank order into zero.  An empty shard resets its slot's count and writes nothing
    else.  mutation: one of MUTATIONS."""
    assert mutation in (None,) + MUTATIONS
    names = table_names(case)
    slots = []
    for rank, (lo, hi) in enumerate(shards):
        before = rows_of(case, np.arange(*shards[0]) if stale is None else stale[rank])
        _, g_stale = xc._run(before, torch.float64)
        rows_stale = {k: np.flatnonzero(m) for k, m in tc.table_rows(case.cfg, before.xi).items() if k in names}
        slot = {k: (rows_stale[k], g_stale[k][rows_stale[k]]) for k in names}  # the previous step's list
        if hi > lo:
            _, g = shard_grads64(case, lo, hi)
            rows = touched(case, lo, hi)
            slot = {k: (rows[k], g[k][rows[k]]) for k in names}
        elif mutation != MUTATIONS[2]:
            slot = {k: (rows_stale[k][:0], g_stale[k][:0]) for k in names}
        slots.append(slot)
    order = list(range(len(slots)))
    if mutation == MUTATIONS[0]:
        order = order[:-1]
    if mutation == MUTATIONS[1] and len(slots) > 1:
        order.insert(2, 1)
    out = {k: np.zeros(case.params[k].shape) for k in names}
    for r in order:
        for k, (rows, vals) in slots[r].items():
            out[k][rows] += vals  # (destinations unique within a list)
    return out


def exchange_caps(cfg, bs):
    """The two families' list capacities at per-rank batch bs as dfwfm_sparse_grads_size reports them for a model
    with both families: the sum over the categorical tables (QR: quotient and remainder table) of min(bs, rows)."""
    num, c = cfg["numerical"], cfg["qr_collisions"]
    cap = 0
    for n in cfg["feature_sizes"][num:]:
        parts = [-(-n // c), c] if (cfg["qr_flag"] and n > cfg["qr_threshold"]) else [n]
        cap += sum(min(bs, rows) for rows in parts)
    return [dict(cap=cap, w=cfg["embedding_size"]), dict(cap=cap, w=1)]
