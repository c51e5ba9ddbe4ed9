"""GPU: the HIP training kernels on the table zoo (tests/table_cases.py) and on two tables large enough for the sorted
scatter's 64-bit keys, against the float64 step (train_cases.ref_step64 through check_step: per tensor and per touched
row at G_TOL, untouched rows exactly zero).

The scatter kernels choose their path by a table's row count -- one bucket per row up to 64 rows, eight sorted buckets
above; privatised LDS sums up to 128 rows, global atomics above; 32-bit sort keys while ceil(rows / 8) < 2^20 -- and a
QR field's remainder table has c rows, so the collision count picks the path too.  The one-step autograd test of every
(c, op), sorted and atomic, is test_gpu_train_variants.test_train_variant_matches_float64 over train_cases.CASES; the
fused step and the row-lazy Adam run over train_cases.FUSED, which holds the zoo's C_FEW cases.  Here: the sorted leg's
bits, a batch across sort passes, the touched-row lists and their capacity, and the 64-bit keys.

Worst gradient error measured on an MI355X, in the format of tests/test_gpu_train_variants.py's table: |g - g64|.max()
over the float64 reference's largest entry of the tensor / of the touched table row, B = 37, bar 2e-5 for both (evidence
of margin, not thresholds).  "same": the atomic leg gave the sorted leg's figures.

    case              port tensor / row    host tensor / row    HIP sorted tensor / row    HIP atomic
    zoo_mult_c1       3.5e-7 / 2.8e-6      4.2e-7 / 1.7e-6      2.9e-7 / 2.1e-6            same
    zoo_mult_c2       3.0e-7 / 3.2e-6      3.6e-7 / 1.5e-6      3.7e-7 / 1.6e-6            same
    zoo_mult_c3       2.9e-7 / 3.3e-6      3.2e-7 / 1.8e-6      2.8e-7 / 4.5e-6            2.5e-7 / 4.5e-6
    zoo_mult_c7       3.4e-7 / 2.1e-6      2.5e-7 / 4.9e-6      2.9e-7 / 1.8e-6            same
    zoo_mult_c64      3.0e-7 / 2.4e-6      3.5e-7 / 2.1e-6      2.1e-7 / 2.1e-6            same
    zoo_mult_c65      2.9e-7 / 2.3e-6      3.3e-7 / 1.2e-6      2.9e-7 / 2.8e-6            same
    zoo_mult_c129     2.8e-7 / 1.8e-6      4.8e-7 / 1.2e-6      2.2e-7 / 3.2e-6            same
    zoo_mult_c5000    3.2e-7 / 2.1e-6      4.0e-7 / 1.9e-6      4.7e-7 / 2.6e-6            3.7e-7 / 2.6e-6
    zoo_add_c1        2.6e-7 / 3.4e-6      3.2e-7 / 2.2e-6      3.0e-7 / 2.1e-6            same
    zoo_add_c2        2.2e-7 / 2.4e-6      2.6e-7 / 1.4e-6      3.6e-7 / 2.2e-6            same
    zoo_add_c3        2.3e-7 / 2.2e-6      4.0e-7 / 1.3e-6      2.8e-7 / 1.3e-6            same
    zoo_add_c7        2.5e-7 / 2.0e-6      2.7e-7 / 1.3e-6      3.3e-7 / 1.4e-6            same
    zoo_add_c64       2.5e-7 / 2.2e-6      2.8e-7 / 1.5e-6      3.3e-7 / 1.7e-6            same
    zoo_add_c65       3.0e-7 / 3.6e-6      3.4e-7 / 2.0e-6      2.6e-7 / 1.7e-6            same
    zoo_add_c129      2.7e-7 / 2.9e-6      2.5e-7 / 1.6e-6      2.9e-7 / 2.7e-6            same
    zoo_add_c5000     3.4e-7 / 2.6e-6      3.4e-7 / 1.2e-6      3.3e-7 / 2.8e-6            same
    zoo39_mult_c1     7.3e-7 / 1.7e-6      1.3e-6 / 9.5e-7      8.2e-7 / 1.5e-6            same
    zoo39_mult_c7     2.9e-7 / 3.2e-6      3.8e-7 / 2.2e-6      3.1e-7 / 3.6e-6            3.3e-7 / 3.6e-6
    zoo39_mult_c129   4.8e-7 / 2.6e-6      3.9e-7 / 1.8e-6      5.6e-7 / 2.7e-6            4.7e-7 / 2.7e-6
    zoo39_add_c1      2.8e-7 / 1.5e-6      4.3e-7 / 1.5e-6      4.3e-7 / 3.5e-6            same
    zoo39_add_c7      3.1e-7 / 1.7e-6      4.0e-7 / 1.2e-6      3.4e-7 / 2.5e-6            same
    zoo39_add_c129    2.5e-7 / 1.1e-6      4.4e-7 / 1.1e-6      3.9e-7 / 1.5e-6            same
    key64 (B = 4133)  1.6e-6 / 1.2e-6      -                    2.1e-7 / 1.4e-6            2.4e-7 / 1.4e-6
    key32 (B = 4133)  1.7e-6 / 1.2e-6      -                    1.9e-7 / 1.4e-6            1.9e-7 / 1.4e-6

B = 4133 on the zoo, per tensor only (sorted / atomic): mult c = 1 6.3e-7 / 3.8e-7, add c = 1 7.1e-7 / 2.9e-7, mult
c = 65 4.4e-7 / 3.4e-7, add c = 65 3.8e-7 / 2.9e-7.  The two big-table cases take 0.5 s and 0.4 s (2.2 s for the first,
which also pays the float64 references' first call) with the table built on the host and filled on the device."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import table_cases as zc
import train_cases as tc
from conftest import logit_close, model_kwargs
from test_gpu_train import G_TOL, _local_lists_step, _sparse_step, build, hip_step
from test_train_variants import port_within_quarter_bar

pytestmark = pytest.mark.gpu

LR, L2 = 1e-3, 3e-7
CASES_ALL = [(c, op) for c in zc.C_ALL for op in zc.OPS]
CASES_FEW = [(c, op) for c in zc.C_FEW for op in zc.OPS]


def test_zoo_cases_run_with_the_fused_step_and_the_lazy_adam():
    assert {zc.name(op, c) for c in zc.C_FEW for op in zc.OPS} <= set(tc.FUSED)


@pytest.mark.parametrize("c,op", CASES_ALL)
def test_zoo_sorted_step_is_bit_identical_and_matches_float64(gpu, c, op):
    """Two sorted (deterministic) steps from the same start: equal bits in the logits and in every gradient; the first
    against the float64 step."""
    name = zc.name(op, c)
    cfg, params, xi, xv, y = tc.case(name)
    runs = []
    for _ in range(2):
        m = build(cfg, params, gpu, is_deep_dropout=False)
        m.deterministic = True
        runs.append(hip_step(m, xi, xv, y, gpu, LR, L2))
    assert np.array_equal(runs[0][0], runs[1][0])
    for k in runs[0][2]:
        assert np.array_equal(runs[0][2][k], runs[1][2][k]), k
    wt, wr = tc.check_step(cfg, params, xi, xv, *runs[0][:3], tc.reference(name)[0])
    print(f"{name} sorted: HIP, gradient error over the tensor's max {wt:.2e}, over the row's max {wr:.2e}")


@pytest.mark.parametrize("c,op", CASES_FEW)
def test_wide_zoo_helper_wave_forward_equals_plain(gpu, monkeypatch, c, op):
    """The 39-field zoo is the smallest shape the helper-wave training forward (ftrain_kernel) takes -- the library has
    no query, so the shape rule of csrc/dfwfm_ftrain.hip is asserted here.  It clamps and saves the scatter's keys with
    its own copy of the range check: against fwd_kernel<TRAIN> (DFWFM_DIAG ftrain=0) the logits and every gradient are
    the same bits, and both match the float64 step."""
    name = zc.name(op, c, True)
    cfg, params, xi, xv, y = tc.case(name)
    F_, D_, N_ = cfg["field_size"], cfg["embedding_size"], cfg["deep_nodes"]
    assert D_ == 10 and F_ <= 48 and -(-F_ * D_ // 16) == 25 and N_ == 400 and cfg["h_depth"] >= 1  # ftrain_supported
    zc.check_inputs(cfg, xi)
    runs = {}
    for ft in ("0", "1"):
        monkeypatch.setenv("DFWFM_DIAG", f"ftrain={ft}")
        m = build(cfg, params, gpu, is_deep_dropout=False)
        m.deterministic = True
        runs[ft] = hip_step(m, xi, xv, y, gpu, LR, L2)
        tc.check_step(cfg, params, xi, xv, *runs[ft][:3], tc.reference(name)[0])
    assert np.array_equal(runs["0"][0], runs["1"][0])
    for k in runs["0"][2]:
        assert np.array_equal(runs["0"][2][k], runs["1"][2][k]), k


def per_tensor(got, ref_grads, what):
    """Every gradient within G_TOL of its tensor's largest float64 entry; returns the worst ratio."""
    worst = 0.0
    for k, r in ref_grads.items():
        sc = np.abs(r).max(initial=0.0)
        if sc == 0.0:
            assert got[k] is None or not np.any(got[k]), (what, k)
            continue
        e = float(np.abs(got[k].astype(np.float64) - r).max() / sc)
        assert e <= G_TOL, (what, k, e)
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("c,op", [(1, "mult"), (1, "add"), (65, "mult"), (65, "add")])
def test_zoo_batch_across_sort_passes(gpu, c, op):
    """B = 4096 + 37: two passes of the sorted scatter (kSortSeg = 4096 samples each), and with c = 1 one remainder row
    -- with c = 65 one of 65 rows' eight buckets, and the 1- and 2-row tables their one bucket -- takes all 4133
    samples across both passes and every chunk carry between.  Gradients per tensor at G_TOL against float64, rows the
    batch did not read exactly zero, two sorted runs equal bits, the atomic scatter within the same per-tensor bar.
    The per-row bar applies at B = 37 only: a row that sums thousands of mixed-sign terms is conditioned by its
    absolute sum, not by its value, so its own largest entry is no scale for an fp32 sum's error."""
    name = zc.name(op, c)
    cfg, params, xi, xv, y = tc.case(name, 4096 + 37)
    zc.check_inputs(cfg, xi)
    ref_logits, ref_loss, ref_grads = tc.ref_step64(cfg, params, xi, xv, y)
    runs = {}
    for leg, det in (("sorted", True), ("sorted again", True), ("atomic", False)):
        m = build(cfg, params, gpu, is_deep_dropout=False)
        m.deterministic = det
        out, loss, grads, _ = hip_step(m, xi, xv, y, gpu, LR, L2)
        assert logit_close(out, ref_logits) < 1e-5, leg
        assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), leg
        print(f"{name} B=4133 {leg}: HIP, gradient error over the tensor's max {per_tensor(grads, ref_grads, leg):.2e}")
        for k, mask in tc.table_rows(cfg, xi).items():
            assert not grads[k][~mask].any(), (leg, k)
        runs[leg] = grads
    for k in runs["sorted"]:
        assert np.array_equal(runs["sorted"][k], runs["sorted again"][k]), k


@pytest.mark.parametrize("c,op", CASES_FEW)
def test_zoo_touched_row_lists(gpu, c, op):
    """dfwfm_sparse_grads_size / _local / _apply on the zoo, by the contract of
    test_gpu_train.test_local_row_lists_equal_dense_table_grads: the lists give the dense table gradients back, one
    entry per touched row, the local buffer is left zero; and the capacity is the sum over tables of min(B, rows),
    a QR field counting ceil(n / c) quotient rows and c remainder rows."""
    from xsdeepfwfm_deprecated_amd import _lib
    cfg, params, xi, xv, y = tc.case(zc.name(op, c))
    m = build(cfg, params, gpu, is_deep_dropout=False)
    B = len(xi)
    want = 0
    for n in zc.ROWS:
        want += min(B, -(-n // c)) + min(B, c) if n > zc.THRESHOLD else min(B, n)
    for fam, width in ((0, zc.D), (1, 1)):
        cap, w, ws = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        _lib.check(_lib.lib().dfwfm_sparse_grads_size(m._sync_engine(gpu).handle, fam, B, ctypes.byref(cap),
                                                      ctypes.byref(w), ctypes.byref(ws)), "size")
        assert cap.value == want and w.value == width, (fam, cap.value, want)
    gd, _, _ = _sparse_step(m, gpu, xi, xv, y, sparse=False)
    touched = sum(int(mask.sum()) for k, mask in tc.table_rows(cfg, xi).items() if k.startswith("fm_2nd"))
    for rep in range(2):
        gl, lists, local, stamp = _local_lists_step(m, gpu, xi, xv, y)
        assert float(local.abs().max()) == 0.0
        for k in gd:
            sc = np.abs(gd[k]).max()
            assert np.abs(gl[k] - gd[k]).max() <= G_TOL * sc + 1e-12, (k, rep)
        assert len(lists) == 2
        for fam, w, od, orow, cnt in lists:
            n = int(cnt.item())
            assert len(np.unique(od[:n].cpu().numpy())) == n
            assert n == touched, (fam, n, touched)  # one entry per row the batch read, in either family


# ---------------------------------------------------------------------------------------------- 64-bit sort keys
BIG_B = 4096 + 37
BIG = {"key64": 2 ** 23 + 4099,   # ceil(rows / 8) >= 2^20: 64-bit keys
       "key32": 8388600}          # the largest count that still sorts with 32-bit keys
BIG_N2 = 100003                   # the second table: large enough that the batch reads most of its rows once
# seeds by train_cases.SEEDS' rule (of 1 .. 19, seeds 6, 17 and 19 keep the fp32 port under G_TOL / 4 per touched row on
# both compact models; 6 by the widest margin: 1.7e-6 per tensor, 1.2e-6 per row)
BIG_SEED = {"key64": 6, "key32": 6}


def big_keys(which, seed):
    """B keys into the big table: rows 0 and n - 1; for 2^23 + 4099 rows, 300 pairs (r, r + 2^23), r < 4099 -- the
    same bucket (r % 8), and sort keys (row / 8) << 12 | sample that differ only in bit 32, so a key cut to 32 bits
    merges the two rows' runs; the rest drawn from 1500 random rows, so most repeat."""
    n = BIG[which]
    rng = np.random.default_rng(1000 + seed)
    keys = [0, n - 1]
    if n > 2 ** 23:
        r = rng.choice(4099, 300, replace=False)
        keys += list(r) + list(r + 2 ** 23)
    pool = rng.integers(0, n, 1500)
    keys += list(pool[rng.integers(0, len(pool), BIG_B - len(keys))])
    keys = np.asarray(keys, np.int64)
    assert len(keys) == BIG_B and keys.min() == 0 and keys.max() == n - 1
    return keys[rng.permutation(BIG_B)]


@functools.lru_cache(maxsize=None)
def big_case(which, seed):
    """(rows, compact case): the touched rows of the big table in index order, and the case of the compact model --
    the big table replaced by those rows, the keys relabelled by rank -- with synthetic weights for every tensor."""
    keys = big_keys(which, seed)
    rows, rank = np.unique(keys, return_inverse=True)
    cfg, params, xi, xv, y = tc.train_case(F=4, num=2, D=10, N=64, H=1, sizes=[len(rows), BIG_N2], B=BIG_B, seed=seed)
    xi = xi.copy()
    xi[:, 0] = rank
    return rows, (cfg, params, xi, xv, y)


def big_model(which, seed, gpu):
    """The model with the big table: zero but for the touched rows, which hold the compact model's; built on the host
    (nn.Embedding's own init) and filled on the device."""
    from xsdeepfwfm_deprecated_amd import DeepFMs
    rows, (cfg_c, params, xi_c, xv, y) = big_case(which, seed)
    cfg = dict(cfg_c, feature_sizes=[1, 1, BIG[which], BIG_N2])
    m = DeepFMs(**model_kwargs(cfg), is_deep_dropout=False)
    small = {k: torch.from_numpy(v) for k, v in params.items() if not k.endswith("embeddings.2.weight")}
    missing, unexpected = m.load_state_dict(small, strict=False)
    assert sorted(missing) == ["fm_1st_embeddings.2.weight", "fm_2nd_embeddings.2.weight"] and not unexpected
    m = m.to(gpu).train()
    r = torch.from_numpy(rows).to(gpu)
    with torch.no_grad():
        for fam in ("fm_1st_embeddings", "fm_2nd_embeddings"):
            w = getattr(m, fam)[2].weight
            w.zero_()
            w[r] = torch.from_numpy(params[f"{fam}.2.weight"]).to(gpu)
    xi = xi_c.copy()
    xi[:, 0] = rows[xi_c[:, 0]]
    return m, xi, r


def big_step(m, xi, xv, y, rows_d, gpu):
    """Forward, BCE, backward.  The big tables' gradients come back compacted to the touched rows, after the rest of
    them was found all zero on the device."""
    m.zero_grad()
    out = m(torch.from_numpy(xi).to(gpu), torch.from_numpy(xv).to(gpu))
    loss = F.binary_cross_entropy_with_logits(out, torch.from_numpy(y).to(gpu))
    loss.backward()
    torch.cuda.synchronize()
    grads = {}
    for k, p in m.named_parameters():
        g = p.grad.detach()
        if k.endswith("embeddings.2.weight"):
            rest = g.clone()
            rest[rows_d] = 0
            assert not bool(rest.any()), (k, "gradient in a row the batch did not touch")
            g = g[rows_d]
        grads[k] = g.cpu().numpy().copy()
    return out.detach().cpu().numpy(), float(loss.item()), grads


@pytest.mark.parametrize("which", list(BIG))
def test_big_table_sort_keys(gpu, which):
    """A table of 2^23 + 4099 rows (64-bit sort keys) and one of 8,388,600 (the last with 32-bit keys), B = 4133.  The
    reference is the float64 step of the compact model; every other tensor's gradient, the logits and the loss must
    match as they are.  Touched rows per tensor and per row at G_TOL (check_step), every untouched row exactly zero
    (on the device), two sorted runs equal bits, the atomic leg within the same bars.  The fp32 port stays under
    G_TOL / 4 on the compact model (the seed's precondition)."""
    t0 = time.perf_counter()
    seed = BIG_SEED[which]
    rows, (cfg_c, params, xi_c, xv, y) = big_case(which, seed)
    ref = tc.ref_step64(cfg_c, params, xi_c, xv, y)
    port = tc.port_step(cfg_c, params, xi_c, xv, y, LR, L2)
    port_within_quarter_bar(which, cfg_c, xi_c, port[2], ref[2])
    t1 = time.perf_counter()
    m, xi, rows_d = big_model(which, seed, gpu)
    assert m.fm_2nd_embeddings[2].weight.shape == (BIG[which], 10)
    assert (-(-BIG[which] // 8) >= 2 ** 20) is (which == "key64")
    t2 = time.perf_counter()
    runs = {}
    for leg, det in (("sorted", True), ("sorted again", True), ("atomic", False)):
        m.deterministic = det
        out, loss, grads = big_step(m, xi, xv, y, rows_d, gpu)
        wt, wr = tc.check_step(cfg_c, params, xi_c, xv, out, loss, grads, ref)
        print(f"{which} {leg}: HIP, gradient error over the tensor's max {wt:.2e}, over the row's max {wr:.2e}")
        runs[leg] = grads
    for k in runs["sorted"]:
        assert np.array_equal(runs["sorted"][k], runs["sorted again"][k]), k
    del m
    torch.cuda.empty_cache()
    t3 = time.perf_counter()
    print(f"{which}: references {t1 - t0:.1f} s, model {t2 - t1:.1f} s, three steps {t3 - t2:.1f} s")
