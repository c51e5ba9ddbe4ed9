"""Shard plans of the data-parallel step on the exact-arithmetic witness (tests/exact_train_cases.py), and a host
emulation of its touched-row exchange (tests/test_dp_cases.py: the CPU leg; tests/test_gpu_dp_worlds.py: the kernels
on 1, 3, 4 and 8 emulated ranks through the C ABI, and FusedTrainStep on 3, 4 and 8 gloo ranks).

On a witness case every float32 sum is exact in any order, so W ranks' gradients on the shards of a batch, each
normalised by the global batch, add up to the float64 reference of the whole batch bit for bit -- whatever order the
lists are applied in and whatever order the all-reduce sums in.  One dropped, duplicated or misplaced list entry, one
skipped rank, one stale list applied again fails.  With dropout on, the masks are free boolean arrays of the case and
0.5 an exact x2: shard_masks rebuilds what every rank draws (its seed, the device counter, its local rows) and the
reference of the whole batch under them is held to the same bits.

A shard plan is (world, per-rank batch): the shards are fit()'s (training._fit_loop: lo = min(end, offset + rank bs),
hi = min(end, lo + bs)), so trailing ranks of a last global batch hold fewer rows, or none."""
import functools

import numpy as np
import torch

import exact_train_cases as xc
import train_cases as tc
from oracle import torch_port

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
def a_case(name, drop=False):
    """The 129-row witness case of a model of A_MODELS.  drop: with the masks one process draws for the whole batch
    (rows 0 .. 128 of the case's seed).  A shard's rows draw other masks -- a function of the rank's seed and of the
    LOCAL row index -- which a_drop_case concatenates per shard plan."""
    if name == "base":
        return xc.base_case(A_B, drop)
    return xc.exact_case(B=A_B, drop=drop, **xc.VARIANTS[name])


def rows_of(case, rows):
    """The case on the rows `rows` (a slice or an index array); dlogit stays the global batch's, and so do the masks'
    rows (shard_masks: one row of masks per global row)."""
    masks = None if case.masks is None else [m[torch.as_tensor(np.arange(len(case.xi))[rows])] for m in case.masks]
    return case._replace(xi=case.xi[rows], xv=case.xv[rows], dlogit=case.dlogit[rows], masks=masks)


# ---- dropout under data parallelism: every rank draws its shard's masks from its own seed, the device counter and
# ---- the LOCAL row index; the global batch's masks are the shards' masks one after the other
# the seeds of the emulated ranks of leg A and of the CPU leg (distinct, fixed; the gloo ranks report their own)
SEEDS = (1791095845, 905835641, 1313127977, 2110101477, 64728819, 1434271551, 320925017, 1884873390)
B1_DROP_PLANS = ("w3", "w4-middle", "w8-even")
B1_WORLD1 = {"w1": (1, 128)}  # one rank on the whole batch: the RCCL world-size-1 group, and one process
MASK_MUTATIONS = ("global row", "counter - 1", "counter + 1", "rank 0's seed on every rank", "layer + 1")


def rank_masks(cfg, seed, counter, rows, row0=0, layer0=0):
    """One rank's keep masks over `rows` local rows: the kernels' dropout_masks at step_seed(seed, counter) -- counter
    None: no step source attached, the seed itself (the C ABI without dfwfm_set_step_source).  row0, layer0: the
    slips of MASK_MUTATIONS (the first row's index, the first layer's)."""
    s = seed if counter is None else torch_port.step_seed(seed, counter)
    w = xc.widths(cfg)
    return torch_port.dropout_masks(s, 0.5, rows, [1] * layer0 + w, row0)[layer0:]


def shard_masks(cfg, shards, seeds, counter, mutation=None):
    """[bool [sum of the shards' rows, width] per layer]: per layer the ranks' masks concatenated in rank order,
    rank r's from seeds[r] at the device counter `counter` (its value when the step's kernels run: 2 for the third
    step) over hi - lo local rows from 0.  An empty shard contributes zero rows.  mutation: one of MASK_MUTATIONS,
    what a kernel or a trainer that slipped would draw instead."""
    assert mutation in (None,) + MASK_MUTATIONS and len(seeds) == len(shards)
    per_rank = []
    for r, (lo, hi) in enumerate(shards):
        seed, c, row0, layer0 = seeds[r], counter, 0, 0
        if mutation == MASK_MUTATIONS[0]:
            row0 = lo - shards[0][0]
        elif mutation in MASK_MUTATIONS[1:3]:
            c = (0 if counter is None else counter) + (-1 if mutation == MASK_MUTATIONS[1] else 1)
        elif mutation == MASK_MUTATIONS[3]:
            seed = seeds[0]
        elif mutation == MASK_MUTATIONS[4]:
            layer0 = 1
        per_rank.append(rank_masks(cfg, seed, c, hi - lo, row0, layer0))
    return [torch.cat(layer) for layer in zip(*per_rank)]


def with_masks(case, masks):
    """The Case with the keep masks `masks` (dropout 0.5: an exact x2).  A Saturated likewise, its loss sum recomputed
    from the float64 logits; its labels and dlogit stay, which is right as long as the logits keep their signs and
    stay saturated (asserted)."""
    if isinstance(case, xc.Saturated):
        new = case.case._replace(masks=masks)
        z, _ = xc.ref64(new)
        z0, _ = xc.ref64(case.case)
        assert np.all(np.abs(z) >= xc.SAT_Z) and np.array_equal(z > 0, z0 > 0), "no longer saturated under the masks"
        return case._replace(case=new, loss_sum=float(np.sum(np.maximum(z, 0.0) - z * case.y)))
    assert all(len(m) == len(case.xi) for m in masks)
    return case._replace(masks=masks)


@functools.lru_cache(maxsize=None)
def a_drop_case(name, plan, mutation=None):
    """a_case(name) under the masks of plan's emulated ranks: rank r draws SEEDS[r] with no step source attached."""
    world, bs = A_PLANS[plan]
    case = a_case(name)
    return with_masks(case, shard_masks(case.cfg, fit_shards(A_B, bs, world), SEEDS[:world], None, mutation))


def b1_plan(plan):
    return B1_WORLD1[plan] if plan in B1_WORLD1 else B1_PLANS[plan]


@functools.lru_cache(maxsize=None)
def b1_certificate(plan, seeds, counter=2):
    """The largest entry of saturated_certificate under the ranks' masks (it must stay below xc.LIMIT)."""
    return max(xc.saturated_certificate(b1_drop_case(plan, seeds, counter)).values())


@functools.lru_cache(maxsize=None)
def b1_drop_case(plan, seeds, counter=2, mutation=None):
    """The saturated case under the masks of plan's ranks at the device counter `counter`; seeds: a tuple."""
    world, bs = b1_plan(plan)
    sat = xc.saturated()
    return with_masks(sat, shard_masks(sat.case.cfg, fit_shards(xc.SAT_B, bs, world), seeds, counter, mutation))


@functools.lru_cache(maxsize=None)
def rate0_logits(plan, rank, seed, counter):
    """float32 logits of the rows a rank is fed in a rate-0 step of a B1 plan (rate0_rows) under the rank's own masks
    at `counter` (0: the eager step, 1: the captured one); exact where the witness's bound holds for these rows
    (asserted: the float64 logits are float32s)."""
    world, bs = b1_plan(plan)
    case = xc.saturated().case
    sub = rows_of(case, rate0_rows(rank, bs, xc.SAT_B))
    z, _ = xc._run(with_masks(sub, rank_masks(case.cfg, seed, counter, bs)), torch.float64)
    z32 = z.astype(np.float32)
    assert np.array_equal(z32.astype(np.float64), z)
    return z32


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
