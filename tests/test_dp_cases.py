"""CPU: the shard plans of tests/dp_cases.py stand on their own -- the plans are fit()'s shards, the 129-row variant
cases carry the witness's certificate, the float64 reference over the shards (normalised by the global batch) adds up
to the global reference exactly, the host emulation of the touched-row exchange returns it and fails under each slip
of the exchange, the rate-0 batches are finite, and eight ranks' slots of the packed buffer stay 16-byte aligned.  With dropout on, the
cases under the ranks' concatenated per-shard masks keep the certificate (and the saturated case its saturation), the
float32 port returns the float64 bits, five slips of the mask rebuild and a backward without dropout each change what
the GPU leg compares with, and training.rank_seed gives the ranks distinct seeds whose masks are uncorrelated.
tests/test_gpu_dp_worlds.py holds the kernels and FusedTrainStep to the same reference."""
import numpy as np
import pytest
import torch

import dp_cases as dc
import exact_train_cases as xc
from oracle import torch_port

PLANS = [("A", k) for k in dc.A_PLANS] + [("B1", k) for k in dc.B1_PLANS]


def _plan(leg, key):
    """(case, world, bs, n_global, the sizes the issue names) of a plan; leg A on the plain 129-row case."""
    if leg == "A":
        return dc.a_case("base"), *dc.A_PLANS[key], dc.A_B, dc.A_SIZES[key]
    return xc.saturated().case, *dc.B1_PLANS[key], xc.SAT_B, dc.B1_SIZES[key]


@pytest.mark.parametrize("leg,key", PLANS)
def test_plans_are_fit_shards(leg, key):
    """Sizes, zero-row ranks, and every global row in exactly one shard -- at an offset too (a later global batch)."""
    _, world, bs, n, sizes = _plan(leg, key)
    for offset in (0, 3 * world * bs):
        shards = dc.fit_shards(n, bs, world, offset)
        assert [hi - lo for lo, hi in shards] == sizes and len(shards) == world
        assert [r for r, (lo, hi) in enumerate(shards) if hi == lo] == [r for r, s in enumerate(sizes) if s == 0]
        seen = np.concatenate([np.arange(lo, hi) for lo, hi in shards])
        assert np.array_equal(seen, np.arange(offset, offset + n))


@pytest.mark.parametrize("world", sorted(dc.B2_WORLDS))
def test_golden_plans_are_fit_shards(world):
    g, bs = dc.B2_WORLDS[world]
    assert [hi - lo for lo, hi in dc.fit_shards(g, bs, world)] == [bs] * world
    part = dc.fit_shards(dc.B2_PARTIAL, bs, world, 3 * g)
    assert [hi - lo for lo, hi in part] == dc.B2_PARTIAL_SIZES[world]
    assert part[0][0] == 3 * g and max(hi for _, hi in part) == 3 * g + dc.B2_PARTIAL <= 256  # the goldens' rows


@pytest.mark.parametrize("name", [m for m in dc.A_MODELS if m != "base"])  # (base-129: test_exact_train_cases)
def test_certificate_holds_on_the_129_row_variants(name):
    case = dc.a_case(name)
    cert = xc.certificate(case)
    worst = max(cert, key=cert.get)
    print(f"{name}-129: worst {cert[worst]:.3g} ({worst}); limit 2^24 = {xc.LIMIT:.3g}")
    assert all(v < xc.LIMIT for v in cert.values()), {k: v for k, v in cert.items() if v >= xc.LIMIT}
    z, g = xc.port32(case)  # and float32 arithmetic alone returns the float64 bits
    z32, g32 = xc.ref32(case)
    assert np.array_equal(z, z32) and not xc.differs(g, g32)
    assert len(dc.table_names(case)) >= 26 and all(np.any(g32[k]) for k in dc.table_names(case)
                                                   if not (name == "fwlw_lw" and k.startswith("fm_1st")))


def _shards_add_up(case, shards):
    z, g = xc.ref64(case)
    total = {k: np.zeros(v.shape) for k, v in g.items()}
    for lo, hi in shards:
        zs, gs = dc.shard_grads64(case, lo, hi)
        assert np.array_equal(zs, z[lo:hi])
        for k in total:
            total[k] += gs[k]
    assert xc.differs(total, g) == [] and all(np.array_equal(total[k], g[k]) for k in g)


@pytest.mark.parametrize("leg,key", PLANS)
def test_reference_over_the_shards_adds_up_to_the_global_reference(leg, key):
    """The witness's certificate restated for shards: dlogit carries the global normaliser (B1: 1 / 128), the
    shards' float64 gradients summed are the global batch's, exactly, and so are the shards' logits."""
    case, world, bs, n, _ = _plan(leg, key)
    _shards_add_up(case, dc.fit_shards(n, bs, world))


@pytest.mark.parametrize("name", [m for m in dc.A_MODELS if m != "base"])
def test_reference_over_the_shards_adds_up_on_the_variants(name):
    for key in ("w4-tail", "w8"):
        _shards_add_up(dc.a_case(name), dc.fit_shards(dc.A_B, dc.A_PLANS[key][1], dc.A_PLANS[key][0]))


@pytest.mark.parametrize("leg,key", PLANS)
def test_emulated_exchange_returns_the_reference_and_fails_under_each_slip(leg, key):
    """Lists per touched row, applied in rank order into zero, give the global reference's table gradients exactly;
    a skipped last slot, rank 1's slot applied twice and an empty shard that keeps its previous list each change a
    bit wherever the plan has what the slip needs (more than one rank; an empty shard)."""
    case, world, bs, n, sizes = _plan(leg, key)
    shards = dc.fit_shards(n, bs, world)
    _, g = xc.ref64(case)
    stale = None if leg == "A" else [dc.rate0_rows(r, bs, n) for r in range(world)]  # what the GPU legs leave there
    got = dc.emulate_exchange(case, shards, stale)
    assert set(got) == set(dc.table_names(case)) and xc.differs(got, {k: g[k] for k in got}) == []
    for mutation in dc.MUTATIONS:
        changed = xc.differs(dc.emulate_exchange(case, shards, stale, mutation), {k: g[k] for k in got})
        if mutation == dc.MUTATIONS[0]:
            applies = sizes[-1] > 0  # (an empty last slot adds nothing: the stale-list slip covers it)
        elif mutation == dc.MUTATIONS[1]:
            applies = world > 1 and sizes[1] > 0
        else:
            applies = 0 in sizes
        print(f"{leg} {key}: {mutation}: {len(changed)} tables differ")
        assert bool(changed) == applies, (mutation, changed[:3])


@pytest.mark.parametrize("key", list(dc.B1_PLANS))
def test_rate0_batches_are_finite_and_fill_every_rank(key):
    """The rows of the two rate-0 steps: a full per-rank batch on every rank (so every send buffer holds a list
    before the measured step), finite float64 logits and gradients at the global normaliser."""
    case = xc.saturated().case
    world, bs = dc.B1_PLANS[key]
    for rank in range(world):
        rows = dc.rate0_rows(rank, bs, xc.SAT_B)
        assert len(rows) == bs and rows.min() >= 0 and rows.max() < xc.SAT_B
        z, g = xc._run(dc.rows_of(case, rows), torch.float64)
        assert np.all(np.isfinite(z)) and all(np.all(np.isfinite(v)) for v in g.values())
        assert any(np.any(g[k]) for k in dc.table_names(case))  # (a nonzero list)
        if dc.B1_SIZES[key] == [bs] * world:
            lo, hi = dc.fit_shards(xc.SAT_B, bs, world)[rank]
            assert np.array_equal(rows, np.arange(lo, hi))


@pytest.mark.parametrize("bs", [8, 16, 17, 64, 129])
def test_eight_slots_of_the_packed_buffer_stay_aligned(bs):
    """Every section of every rank's slice of the all-gathered [8, nbytes] buffer starts 16-byte aligned (the int64
    destination lists need 8), at the capacities of the plain and the QR models, and no two sections overlap."""
    from xsdeepfwfm_deprecated_amd.training import packed_layout
    for name in ("base", "qr_mult"):
        fams = dc.exchange_caps(dc.a_case(name).cfg, bs)
        nbytes = packed_layout(fams)
        assert nbytes % 16 == 0 and all(f["cap"] > 0 for f in fams)
        spans = sorted([(f["o_dest"], 8 * f["cap"]) for f in fams] + [(f["o_rows"], 4 * f["cap"] * f["w"]) for f in fams]
                       + [(fams[0]["o_cnt"], 4 * len(fams))])
        assert [f["o_cnt"] - fams[0]["o_cnt"] for f in fams] == [0, 4]
        for (a, n), (b, _) in zip(spans, spans[1:] + [(nbytes, 0)]):
            assert a + n <= b
        for r in range(8):
            assert all((r * nbytes + o) % 16 == 0 for o, _ in spans)


# =========================================================================== dropout under data parallelism
A_DROP = [(m, p) for m in dc.A_MODELS for p in dc.A_PLANS]


def _seeds(world):
    return dc.SEEDS[:world]


def _nonempty(sizes):
    return sum(1 for s in sizes if s > 0)


def test_shard_masks_are_the_ranks_own_local_rows():
    """Per layer the ranks' masks one after the other, each over its local rows from 0 at its own seed and counter; an
    empty shard adds no row; without a counter the seed itself (no step source attached)."""
    cfg = xc.saturated().case.cfg
    shards = dc.fit_shards(xc.SAT_B, 48, 4)  # 48 / 48 / 32 / 0
    masks = dc.shard_masks(cfg, shards, _seeds(4), 2)
    assert [tuple(m.shape) for m in masks] == [(xc.SAT_B, w) for w in xc.widths(cfg)]
    for r, (lo, hi) in enumerate(shards):
        own = torch_port.dropout_masks(torch_port.step_seed(dc.SEEDS[r], 2), 0.5, hi - lo, xc.widths(cfg))
        assert all(torch.equal(m[lo:hi], o) for m, o in zip(masks, own)), r
    raw = dc.shard_masks(cfg, shards[:1], _seeds(1), None)
    assert all(torch.equal(m, o) for m, o in zip(raw, torch_port.dropout_masks(dc.SEEDS[0], 0.5, 48, xc.widths(cfg))))


@pytest.mark.parametrize("plan", list(dc.B1_PLANS))
def test_saturated_case_stays_exact_under_shard_masks(plan):
    """Every B1 plan's concatenated per-rank masks at counter 2: the case stays saturated with its signs, the
    certificate (p - 2^-6 g and the loss sum included) stays below 2^24 and sgd_ref is exact; the float32 port returns
    the float64 bits forwards and with the batch reversed."""
    world, _ = dc.B1_PLANS[plan]
    sat0, sat = xc.saturated(), dc.b1_drop_case(plan, _seeds(world))
    z, _ = xc.ref64(sat.case)
    assert np.all(np.abs(z) >= xc.SAT_Z) and np.array_equal(z > 0, xc.ref64(sat0.case)[0] > 0)
    assert sat.loss_sum == float(np.sum(np.maximum(z, 0.0) - z * sat.y)) and sat.loss_sum != sat0.loss_sum
    cert = xc.saturated_certificate(sat)
    worst = max(cert, key=cert.get)
    print(f"sat-128 {plan} under shard masks: min |z| {np.abs(z).min():.0f}; worst {cert[worst] / xc.LIMIT:.3f} "
          f"x 2^24 ({worst})")
    assert all(v < xc.LIMIT for v in cert.values()), {k: v for k, v in cert.items() if v >= xc.LIMIT}
    xc.sgd_ref(sat)  # asserts p - lr g is a float32
    z32, g32 = xc.ref32(sat.case)
    for reverse in (False, True):
        zp, gp = xc.port32(sat.case, reverse)
        assert np.array_equal(zp, z32) and not xc.differs(gp, g32), reverse


@pytest.mark.parametrize("plan", dc.B1_DROP_PLANS)
def test_rate0_logits_are_exact_under_each_ranks_masks(plan):
    """The rate-0 steps' rows under each rank's masks at counters 0 and 1: the logits' bound over their quantum stays
    below 2^24, and float32 arithmetic returns the float64 bits; the two counters' logits differ (the GPU leg can tell
    the eager step's seed from the captured step's)."""
    world, bs = dc.B1_PLANS[plan]
    case = xc.saturated().case
    q = xc.quanta(case)["logits"]
    for rank in range(world):
        z = []
        for counter in (0, 1):
            sub = dc.with_masks(dc.rows_of(case, dc.rate0_rows(rank, bs, xc.SAT_B)),
                                dc.rank_masks(case.cfg, dc.SEEDS[rank], counter, bs))
            assert xc.bounds(sub)["logits"] / q < xc.LIMIT
            z.append(dc.rate0_logits(plan, rank, dc.SEEDS[rank], counter))
            assert np.array_equal(xc.port32(sub)[0], z[-1]) and np.array_equal(xc.port32(sub, True)[0], z[-1])
        assert not np.array_equal(z[0], z[1]), rank


@pytest.mark.parametrize("model,plan", A_DROP)
def test_129_row_cases_stay_exact_under_shard_masks(model, plan):
    """Every A plan on every A model under its emulated ranks' masks (no step source): the certificate stays below
    2^24, and the float32 port returns the float64 bits forwards and with the batch reversed."""
    case = dc.a_drop_case(model, plan)
    cert = xc.certificate(case)
    worst = max(cert, key=cert.get)
    print(f"{model}-129 {plan} under shard masks: worst {cert[worst]:.3g} ({worst}); limit 2^24 = {xc.LIMIT:.3g}")
    assert all(v < xc.LIMIT for v in cert.values()), {k: v for k, v in cert.items() if v >= xc.LIMIT}
    z32, g32 = xc.ref32(case)
    for reverse in (False, True):
        zp, gp = xc.port32(case, reverse)
        assert np.array_equal(zp, z32) and not xc.differs(gp, g32), reverse
    if plan != "w1":  # the shards' masks are not one process's on the whole batch
        assert xc.differs(g32, xc.ref32(dc.a_case(model, True))[1])


def _applies(mutation, sizes):
    """Whether a slip of dc.MASK_MUTATIONS changes any mask: the global row and rank 0's seed only where a rank other
    than rank 0 holds rows."""
    return _nonempty(sizes[1:]) > 0 or mutation not in (dc.MASK_MUTATIONS[0], dc.MASK_MUTATIONS[3])


def _sgd64(sat):
    _, g = xc.ref64(sat.case)
    return {k: p.astype(np.float64) - xc.SGD_LR * g[k] for k, p in sat.case.params.items()}


@pytest.mark.parametrize("plan", dc.B1_DROP_PLANS)
def test_each_mask_slip_changes_what_the_gloo_ranks_are_compared_with(plan):
    """A reference that rebuilt the masks wrongly -- by the global row, at the counter before or after, from rank 0's
    seed on every rank, at the next layer's index -- or left dropout out of the backward differs from the right one in
    a float32 bit of some p - 2^-6 g, of some gradient and of the logits: what test_gpu_dp_worlds compares the ranks'
    parameters and logits with would fail them."""
    world, _ = dc.B1_PLANS[plan]
    sat = dc.b1_drop_case(plan, _seeds(world))
    (z, g), want = xc.ref64(sat.case), _sgd64(sat)
    for mutation in dc.MASK_MUTATIONS:
        mut = dc.b1_drop_case(plan, _seeds(world), 2, mutation)
        zm, gm = xc.ref64(mut.case)
        changed = xc.differs(_sgd64(mut), want)
        print(f"B1 {plan}: {mutation}: {len(changed)} tensors of p - lr g differ, {int(np.sum(zm != z))} logits")
        assert _applies(mutation, dc.B1_SIZES[plan])
        assert changed and xc.differs(gm, g) and not np.array_equal(zm.astype(np.float32), z.astype(np.float32))
        assert mut.loss_sum != sat.loss_sum
    fwd_only = xc.mutations(sat.case)["dropout in the forward only"]
    lr = {k: p.astype(np.float64) - xc.SGD_LR * fwd_only[k] for k, p in sat.case.params.items()}
    assert xc.differs(fwd_only, g) and xc.differs(lr, want)


@pytest.mark.parametrize("model,plan", A_DROP)
def test_each_mask_slip_changes_what_the_emulated_ranks_are_compared_with(model, plan):
    """The same slips on the 129-row models and the A plans (the 1-row and 0-row shards, QR, EmbeddingBag, fwlw): a
    gradient bit and a logit change wherever the plan has what the slip needs (a second rank with rows)."""
    case = dc.a_drop_case(model, plan)
    z, g = xc.ref64(case)
    for mutation in dc.MASK_MUTATIONS:
        zm, gm = xc.ref64(dc.a_drop_case(model, plan, mutation))
        changed = xc.differs(gm, g)
        applies = _applies(mutation, dc.A_SIZES[plan])
        assert bool(changed) == applies, (mutation, changed[:3])
        assert (not np.array_equal(zm.astype(np.float32), z.astype(np.float32))) == applies, mutation
    assert xc.differs(xc.mutations(case)["dropout in the forward only"], g)


def test_hand_written_tower_is_the_reference_under_shard_masks():
    """deep_tower64, in which the forward-only slip is made, reproduces ref64 under concatenated per-shard masks."""
    for case in (dc.a_drop_case("base", "w4-tail"), dc.b1_drop_case("w4-middle", _seeds(4)).case):
        _, g = xc.ref64(case)
        for k, v in xc.deep_tower64(case).items():
            assert np.array_equal(v, g[k]), k


# ---- the ranks' seeds (training.rank_seed)
BASES = (0, 1, 99, 1791095845, 2 ** 31 - 2, 2 ** 32 - 1)


def test_rank_seed_keeps_rank_0_and_separates_the_ranks():
    from xsdeepfwfm_deprecated_amd.training import rank_seed
    for base in BASES:
        seeds = [rank_seed(base, r) for r in range(8)]
        assert seeds[0] == base and len(set(seeds)) == 8, (base, seeds)
        assert all(isinstance(s, int) and 0 <= s < 2 ** 32 for s in seeds)
        assert seeds == [rank_seed(base, r) for r in range(8)]  # a pure function
    assert rank_seed(2 ** 32 + 5, 3) == rank_seed(5, 3)  # 32 bits, as dfwfm_train_forward takes the seed


def _agreement(a, b):
    """(fraction of equal entries, number of entries) of two lists of masks."""
    n = sum(m.numel() for m in a)
    return sum(int((x == y).sum()) for x, y in zip(a, b)) / n, n


def test_rank_seeds_draw_uncorrelated_masks():
    """Any two ranks' masks over 43 rows x the base model's widths agree on 0.5 +- 6 sigma of their entries (sigma =
    0.5 / sqrt(n) for n independent fair bits; n = 43 x 1590 = 68 370: +- 0.0115), and so do one rank's masks at two
    consecutive counters.  With one seed on every rank the agreement is 1."""
    from xsdeepfwfm_deprecated_amd.training import rank_seed
    cfg = xc.saturated().case.cfg
    worst = 0.0
    for base in BASES:
        masks = [dc.rank_masks(cfg, rank_seed(base, r), 2, 43) for r in range(8)]
        nxt = [dc.rank_masks(cfg, rank_seed(base, r), 3, 43) for r in range(8)]
        pairs = [(masks[a], masks[b]) for a in range(8) for b in range(a + 1, 8)] + list(zip(masks, nxt))
        for x, y in pairs:
            frac, n = _agreement(x, y)
            assert n == 43 * sum(xc.widths(cfg)) == 68370
            worst = max(worst, abs(frac - 0.5))
            assert abs(frac - 0.5) <= 6 * 0.5 / np.sqrt(n), (base, frac)
        keep, n = _agreement(masks[0], [torch.ones_like(m) for m in masks[0]])
        assert abs(keep - 0.5) <= 6 * 0.5 / np.sqrt(n)  # (and each mask keeps half)
    print(f"worst |agreement - 0.5| = {worst:.4f}; bound {6 * 0.5 / np.sqrt(68370):.4f}")
    assert _agreement(dc.rank_masks(cfg, 7, 2, 43), dc.rank_masks(cfg, 7, 2, 43))[0] == 1.0
