"""CPU: the relocation cases of tests/big_table_cases.py are what they claim (which probed rows straddle or start at
2^31 B, 2^32 B, 2^33 B and 2^31 floats, in the plain table, the serving copies and the flat gradient layout; the row
map; the batches), the twin is a sound reference (the float64 oracle at the golden tests' bars), and the host kernels
(libdfwfm_cpu.so) on G1 give the twin's bits from a table of 107,374,200 rows."""
import numpy as np
import pytest
import torch

import big_table_cases as bt
import train_cases as tc
from conftest import logit_close
from oracle import dfwfm_oracle
from test_cpu_kernel import G_TOL, cpu_model, run

P31, P32, P33 = 2 ** 31, 2 ** 32, 2 ** 33


def _rows(geo, mask):
    return [int(r) for r in geo.probed[mask]]


def test_the_edges_are_what_they_claim_g1():
    for name in ("g1", "g1qr_mult", "g1qr_add"):
        geo = bt.GEOS[name]
        off, later = bt.offsets(geo)
        assert geo.rows == 107_374_200 and geo.K == 22 <= 64 and geo.rows * 40 == 4_294_968_000 > P32
        assert {0, 1, geo.rows - 2, geo.rows - 1} <= set(geo.probed.tolist())
        # the plain table: one row straddles byte 2^31, one byte 2^32, both neighbours probed
        assert _rows(geo, bt.straddles(off["emb2_bytes"], P31)) == [53_687_091]
        assert _rows(geo, bt.straddles(off["emb2_bytes"], P32)) == [107_374_182]
        assert {53_687_090, 53_687_092, 107_374_181, 107_374_183} <= set(geo.probed.tolist())
        assert off["emb2_elems"].max() < P31  # no element offset past 2^31 in G1: that is G2
        # the copies: a row starts exactly at the crossing, its predecessor ends right below it
        assert _rows(geo, bt.starts_at(off["copy64"], P31)) == [33_554_432] and 33_554_431 in geo.probed
        assert _rows(geo, bt.starts_at(off["copy64"], P32)) == [67_108_864] and 67_108_863 in geo.probed
        assert _rows(geo, bt.starts_at(off["copy32"], P31)) == [67_108_864]
        assert off["copy32"].max() < P32
        assert (off["copy64"][:, 0] > P32).sum() >= 5 and (off["copy32"][:, 0] > P31).sum() >= 5
        # not crossed, and said so: the int8 copy and the first-order table
        assert off["copy16"].max() < P31 and off["emb1_bytes"].max() < P31
        # the flat gradient layout, huge field first: every later table starts past 2^30 floats (2^32 bytes)
        assert later == geo.rows * 11 > 2 ** 30 and later * 4 > P32
    qr = bt.GEOS["g1qr_mult"]
    assert qr.keys == 429_496_800 < P31 and qr.c == 4 and qr.twin_keys == 88 > bt.QR_THRESHOLD


def test_the_edges_are_what_they_claim_g2():
    geo = bt.GEOS["g2"]
    off, later = bt.offsets(geo)
    assert geo.rows == 67_108_900 and geo.K == 14 and geo.D == 32 and geo.rows * 32 == 2_147_484_800 > P31
    assert _rows(geo, bt.starts_at(off["emb2_elems"], P31)) == [67_108_864]
    assert _rows(geo, bt.starts_at(off["emb2_bytes"], P33)) == [67_108_864]
    assert _rows(geo, bt.starts_at(off["emb2_bytes"], P32)) == [33_554_432]
    assert {67_108_863, 67_108_865, 33_554_431, 33_554_433, 0, 1, geo.rows - 2, geo.rows - 1} <= set(geo.probed.tolist())
    assert (off["emb2_elems"][:, 0] > P31).sum() >= 3  # 67,108,865 and the last two rows
    assert later == geo.rows * 33 > P31
    # the shape trains: the backward's LDS tile (bwd_layout, csrc/dfwfm_train.hip, restated) fits 160 KiB at F = 28
    # and not with one more field; the forward sweep's F = 39 is far over
    assert geo.F == 28 and _bwd_lds_bytes(28, 32, 400) == 161_792 <= 160 * 1024 < _bwd_lds_bytes(29, 32, 400)
    assert _bwd_lds_bytes(39, 32, 400) > 160 * 1024 and geo.N % 4 == 0


def _bwd_lds_bytes(F, D, N):
    """backward_lds_bytes of csrc/dfwfm_train.hip with dfwfm_model_create's MT, S, SX, SY (16-row tiles)."""
    r4 = lambda x: (x + 3) & ~3  # noqa: E731
    NT, NC0, MT, S = (N + 15) // 16, (F * D + 15) // 16, (F + 15) // 16, (F + 3) // 4
    SX, SY = r4(max(NC0 * 16, 4 * S * D, NT * 16)) + 4, NT * 16 + 4
    floats = (r4(F) + r4(F * D) + MT * S * 64 + 16 * max(SX, SY) + 16 * SX + max(16 * SY, 2 * MT * MT * 256) + 16 + SY
              + 8 * 64 * 4 + 2 * 16 * r4(F))
    return 4 * r4(floats)


@pytest.mark.parametrize("name", list(bt.GEOS))
def test_row_map_and_batches(name):
    geo = bt.GEOS[name]
    assert np.all(np.diff(geo.probed) > 0) and geo.probed[0] == 0 and geo.probed[-1] == geo.rows - 1
    assert np.array_equal(bt.rank_of(geo, geo.probed), np.arange(geo.K))  # monotone: ascending rows, ascending ranks
    cfg, _ = bt.twin(name)
    assert cfg["feature_sizes"][bt.NUM + bt.FIELD] == geo.twin_keys and bt.FIELD != geo.F - bt.NUM - 1
    for kind in ("dup", "dup_rev", "once"):
        xi_h, xi_t, xv, y, dl = bt.batch(name, kind)
        col_h, col_t = xi_h[:, bt.FIELD], xi_t[:, bt.FIELD]
        assert 0 <= col_h.min() and col_h.max() < geo.keys < P31 and col_t.max() < geo.twin_keys
        rows_h = col_h // geo.c if geo.qr else col_h
        rows_t = col_t // geo.c if geo.qr else col_t
        assert np.array_equal(geo.probed[rows_t], rows_h)
        # the map keeps the order of any two samples' rows (the sorted scatter's (row, sample) order)
        assert np.array_equal(np.argsort(rows_h, kind="stable"), np.argsort(rows_t, kind="stable"))
        hits = np.bincount(rows_t, minlength=geo.K)
        if kind == "once":
            assert len(col_h) == geo.K and np.all(hits == 1)
        else:
            assert len(col_h) == bt.B_DUP and np.all(hits >= 1) and (hits >= 2).sum() >= 3
            hot = {int(r) for r in geo.probed[hits >= 2]}
            if kind == "dup":  # the rows at the crossings are hit twice or more (dup_rev: the other end of the cycle)
                assert {e for e, _ in geo.edges} <= hot
        if geo.qr:
            assert np.array_equal(col_h % 4, col_t % 4) and set((col_h % 4).tolist()) == {0, 1, 2, 3}
        keep = np.arange(geo.F - bt.NUM) != bt.FIELD
        assert np.array_equal(xi_h[:, keep], xi_t[:, keep]) and np.all(dl != 0)


@pytest.mark.parametrize("name", list(bt.GEOS))
def test_twin_forward_matches_oracle(name):
    cfg, params = bt.twin(name)
    for kind in ("dup", "once"):
        _, xi, xv, _, _ = bt.batch(name, kind)
        got = run(cpu_model(cfg, params), xi, xv)
        assert logit_close(got, dfwfm_oracle.forward(cfg, params, xi, xv)) < 1e-5


@pytest.mark.parametrize("name", list(bt.GEOS))
def test_twin_training_step_matches_oracle(name):
    """One training step of the twin (host kernels through autograd) against the float64 step at the golden tests'
    bars: logits 1e-5, loss 1e-5, every gradient tensor G_TOL of its largest entry."""
    cfg, params = bt.twin(name)
    _, xi, xv, y, _ = bt.batch(name, "dup")
    m = cpu_model(cfg, params, is_deep_dropout=False).train()
    out = m(torch.from_numpy(xi), torch.from_numpy(xv))
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out, torch.from_numpy(y))
    loss.backward()
    grads = {k: p.grad.numpy().copy() for k, p in m.named_parameters()}
    assert G_TOL == tc.G_TOL
    tc.check_step(cfg, params, xi, xv, out.detach().numpy(), float(loss.item()), grads,
                  tc.ref_step64(cfg, params, xi, xv, y), per_row=False)


def _huge_cpu_model(geo, cfg, params):
    """The twin's module with the huge field's tables replaced by torch.empty tables of geo.rows rows, only the probed
    rows written: untouched pages are never committed.  Skips when the host cannot give the address space."""
    m = cpu_model(cfg, params, is_deep_dropout=False)
    idx = torch.from_numpy(geo.probed)
    for fam, width in ((m.fm_2nd_embeddings, geo.D), (m.fm_1st_embeddings, 1)):
        mod = fam[bt.NUM + bt.FIELD]
        small = mod.weight.detach()
        try:  # nothing of the project's runs in here: an allocation and an indexed write
            big = torch.empty(geo.rows, width)
            big[idx] = small
        except (MemoryError, RuntimeError) as e:  # torch reports a failed host allocation as RuntimeError
            pytest.skip(f"no address space for a {geo.rows * width * 4} byte host table: {e}")
        mod.weight = torch.nn.Parameter(big)
    return m


def test_host_kernels_on_g1_equal_the_twin():
    """Forward and backward of the host kernels on a 107,374,200-row table at 1 and 4 threads: the twin's bits on the
    logits, on every small parameter's gradient and on the probed rows' gradients; no gradient outside them."""
    geo = bt.GEOS["g1"]
    cfg, params = bt.twin("g1")
    huge = _huge_cpu_model(geo, cfg, params)
    twin = cpu_model(cfg, params, is_deep_dropout=False)
    names = bt.table_names(geo)
    idx = torch.from_numpy(geo.probed)
    prev = torch.get_num_threads()
    try:
        for threads in (1, 4):
            torch.set_num_threads(threads)
            for kind in ("dup", "once")[:1 if threads == 1 else 2]:
                xi_h, xi_t, xv, _, dl = bt.batch("g1", kind)
                assert np.array_equal(run(huge, xi_h, xv), run(twin, xi_t, xv)), (threads, kind, "eval logits")
                res = []
                for m, xi in ((huge, xi_h), (twin, xi_t)):
                    m.train().zero_grad(set_to_none=True)
                    out = m(torch.from_numpy(xi), torch.from_numpy(xv))
                    out.backward(torch.from_numpy(dl))
                    res.append((out.detach().numpy(), dict(m.named_parameters())))
                (out_h, ph), (out_t, pt) = res
                assert np.array_equal(out_h, out_t), (threads, kind, "train logits")
                for k, p in pt.items():
                    gh = ph[k].grad[idx] if k in names else ph[k].grad
                    assert torch.equal(gh, p.grad), (threads, kind, k)
                if threads == 4 and kind == "dup":  # the complement, once: a write to a wrong row
                    for k in names:
                        g = ph[k].grad
                        g[idx] = 0.0
                        assert not bool(g.any()), (k, "gradient outside the probed rows")
    finally:
        torch.set_num_threads(prev)
