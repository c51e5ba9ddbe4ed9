"""CPU: the shard plans of tests/dp_cases.py stand on their own -- the plans are fit()'s shards, the 129-row variant
cases carry the witness's certificate, the float64 reference over the shards (normalised by the global batch) adds up
to the global reference exactly, the host emulation of the touched-row exchange returns it and fails under each slip
of the exchange, the rate-0 batches are finite, and eight ranks' slots of the packed buffer stay 16-byte aligned.
tests/test_gpu_dp_worlds.py holds the kernels and FusedTrainStep to the same reference."""
import numpy as np
import pytest
import torch

import dp_cases as dc
import exact_train_cases as xc

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
