"""CPU: the structured pruned cases of tests/pruned_cases.py are what tests/test_gpu_pruned_exact.py needs them to be.

Exact: every sum of the forward stays below 2^24 quanta, so the float64 oracle cast to float32 is the answer of any
float32 kernel that adds the right terms, in any order (checked against oracle/torch_port's float32 forward).
Structured: the row lengths, group patterns, k coverage, pair counts and placements are there.  Not degenerate: the
logits differ from row to row and the deep / second-order parts are not zero.  Sensitive: the numpy emulation of each
list equals the oracle bit for bit, and stops doing so as soon as one entry is dropped, duplicated or misplaced."""
import numpy as np
import pytest
import torch

import pruned_cases as pc
from oracle import dfwfm_oracle, torch_port

SPARSE = [s + (v,) for s in pc.SPARSE_SHAPES for v in ("A", "B")] + [(8, 96, 2, 39, "density")]
PAIRS = [(s, n) for s in pc.PAIR_SHAPES for n in pc.pair_counts(s)]
_sid = lambda c: "-".join(str(x) for x in c)


def _assert_sum_exact(terms, q, what, extra=0.0):
    """terms [B, ..., n]: multiples of q whose absolute sum (plus |extra|) over the last axis is at most 2^24 q, so
    that every partial sum in any order is a float32."""
    t = np.asarray(terms, dtype=np.float64)
    assert np.array_equal(t / q, np.round(t / q)), what
    worst = (np.abs(t).sum(-1) + np.abs(extra)).max(initial=0.0)
    assert worst <= 2.0 ** 24 * q, (what, worst / (2.0 ** 24 * q))
    return worst / (2.0 ** 24 * q)


def _assert_exact(cfg, params, xi, xv):
    total, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    E = parts["E"]
    B, F, D = E.shape
    assert np.array_equal(E, np.round(E)) and np.abs(E).max() < 2 ** 12  # integers (QR: products of integers)
    ratios = []
    # first order
    if cfg["use_fwlw"]:
        wfl = params["fwfm_linear.weight"].astype(np.float64)
        ratios.append(_assert_sum_exact(E * wfl[None], 0.5, "fwlw dot"))
        fo = np.einsum("bfd,fd->bf", E, wfl)
    else:
        fo = dfwfm_oracle.embeddings(cfg, params, xi, xv, prefix="fm_1st_embeddings")[:, :, 0]
    lw = params["fm_1st.weight"][0].astype(np.float64) if cfg["use_lw"] else np.ones(F)
    ratios.append(_assert_sum_exact(fo * lw[None], 0.25, "first order"))
    # second order: w_kl E_kd E_ld over every pair and d (the Gram path also adds the pairs of weight zero)
    R = params["field_cov.weight"].astype(np.float64)
    Rs = (R + R.T) * 0.5
    assert np.array_equal(Rs.astype(np.float32), Rs) and np.array_equal(Rs * 4, np.round(Rs * 4))
    iu = np.triu_indices(F, 1)
    prod = E[:, iu[0], :] * E[:, iu[1], :]                        # [B, P, D]
    ratios.append(_assert_sum_exact(prod.reshape(B, -1), 1.0, "Gram"))
    ratios.append(_assert_sum_exact((prod * Rs[iu][None, :, None]).reshape(B, -1), 0.25, "second order"))
    # torch_port's form: the whole [F, F] outer product with the diagonal, halved
    full = np.einsum("bkd,bld->bkld", E, E) * Rs[None, :, :, None]
    ratios.append(_assert_sum_exact(full.reshape(B, -1), 0.25, "second order, reference form"))
    q = 0.25
    deep = np.zeros(B)
    if cfg["use_deep"]:
        h = E.reshape(B, -1)
        q = 1.0
        for l in range(1, cfg["h_depth"] + 1):
            W = params[f"net_1_linear_{l}.weight"].astype(np.float64)
            b = params[f"net_1_linear_{l}.bias"].astype(np.float64)
            if (W != np.round(W)).any():
                q *= 0.5
            # per neuron sum_k |w_k x_k| + |b| <= 2^24 q (|W| and |h| separate the absolute sum)
            worst = (np.abs(h) @ np.abs(W).T + np.abs(b)[None]).max()
            assert worst <= 2.0 ** 24 * q, (l, worst / (2.0 ** 24 * q))
            ratios.append(worst / (2.0 ** 24 * q))
            h = np.maximum(h @ W.T + b, 0.0)
            assert np.array_equal(h / q, np.round(h / q))
        fc = params["net_1_fc.weight"][0].astype(np.float64)
        q *= 0.5
        ratios.append(_assert_sum_exact(h * fc[None], q, "net_1_fc"))
        # the folded layer 1: W1'[n, f] = sum_d W1[n, f D + d] v_f[d], then W1'[n, f] Xv[f] -- the same absolute sums
        W1 = params["net_1_linear_1.weight"].astype(np.float64)
        for f in range(cfg["numerical"]):
            v = params[f"fm_2nd_embeddings.{f}.weight"][0].astype(np.float64)
            ratios.append(_assert_sum_exact(W1[:, f * D:(f + 1) * D] * v[None], 0.5, "fold"))
        deep = h @ fc
    q = min(q, 0.25)
    comb = np.stack([parts["first"], parts["second"], deep, np.full(B, float(params["bias"][0]))], axis=1)
    ratios.append(_assert_sum_exact(comb, q, "combine"))
    assert np.array_equal(comb.sum(1), total)
    # ... and so the float32 reference forward gives the oracle's bits
    tp = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()}
    ref32 = torch_port.forward(cfg, tp, torch.from_numpy(xi), torch.from_numpy(xv)).numpy()
    assert ref32.dtype == np.float32
    assert np.array_equal(ref32, total.astype(np.float32))
    assert np.array_equal(total.astype(np.float32).astype(np.float64), total)
    return max(ratios)


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("case", SPARSE, ids=_sid)
def test_sparse_cases_are_exact(case):
    worst = _assert_exact(*pc.sparse_case(*case))
    print(case, "worst absolute sum / (2^24 q):", worst)


@pytest.mark.parametrize("case", PAIRS, ids=_sid)
def test_pair_cases_are_exact(case):
    worst = _assert_exact(*pc.pairs_case(*case))
    print(case, "worst absolute sum / (2^24 q):", worst)


# ------------------------------------------------------------------------------------------------ structure
def _lens(params, l):
    return (params[f"net_1_linear_{l}.weight"] != 0).sum(1)


@pytest.mark.parametrize("shape", pc.SPARSE_SHAPES, ids=_sid)
def test_sparse_case_has_the_promised_structure(shape):
    D, N, H, F = shape
    cfg, params, xi, xv = pc.sparse_case(D, N, H, F, "A")
    assert xi.shape[0] == xv.shape[0] == pc.ROWS == max(pc.SPARSE_BATCHES)
    seen = set()
    for l in range(1, H + 1):
        W = params[f"net_1_linear_{l}.weight"]
        K = F * D if l == 1 else N
        assert W.shape == (N, K)
        vals = {1.0, -1.0, 0.5, -0.5} if l == 1 else {1.0, -1.0}
        assert set(np.unique(W[W != 0]).tolist()) == vals
        lens = _lens(params, l)
        assert np.array_equal(lens, pc.row_lengths(K, N, l))
        # full and near-full rows in every layer; the last neuron is full
        assert (lens == K).any() and (lens == K - 1).any() and lens[N - 1] == K
        # the cycle, wherever the patterns leave twenty neurons for it
        if N - 4 * len(pc.pattern_groups(N, l)) - 2 >= len(pc.CYCLE):
            assert {min(c, K) for c in pc.CYCLE} <= set(lens.tolist())
        # group patterns
        for name, g in pc.pattern_groups(N, l).items():
            got = lens[4 * g:4 * g + 4].tolist()
            seen.add(name)
            if name == "0000":
                assert got == [0, 0, 0, 0]
            elif name == "equal":
                assert len(set(got)) == 1 and got[0] > 0
            elif name in ("kk", "kk_top"):
                assert [x - got[0] for x in got] == [0, 1, 7, 8]
            else:
                assert got == [K if c == "F" else 0 for c in name] and got[name.index("F")] == K
        # k coverage
        used = np.abs(W).sum(0) > 0
        assert used[0] and used[K - 1] and all(used[c:c + 32].any() for c in range(0, K, 32))
        if N >= 96:  # not only through the full rows
            short = W[(lens > 1) & (lens < K - 9)]
            assert (short[:, 0] != 0).any() and (short[:, K - 1] != 0).any()
        # ReLU of the bias alone, both ways
        b = params[f"net_1_linear_{l}.bias"]
        assert (b[lens == 0] < 0).any() and (b[lens == 0] > 0).any()
        assert np.array_equal(b, np.round(b)) and np.abs(b).max() <= 3
    assert seen == set(pc.PATTERNS)  # every pattern in every layer, or (N = 20) in the layers together
    if N >= 96:
        assert all(set(pc.pattern_groups(N, l)) == set(pc.PATTERNS) for l in range(1, H + 1))
    assert set(np.unique(params["net_1_fc.weight"]).tolist()) <= {0.0, 0.5, -0.5, 1.0, -1.0}
    R = params["field_cov.weight"]
    assert np.array_equal(R, R.T) and np.array_equal(R * 2, np.round(R * 2)) and R.any()


def test_sparse_shapes_reach_what_they_are_for():
    """The figures of the table in the issue: staging units, waves without a group, a wave with a fifth group."""
    cap = {s: pc.ecap(s[3] * s[0], s[1]) for s in pc.SPARSE_SHAPES}
    assert cap[(16, 512, 2, 39)] == 8 and cap[(16, 400, 3, 36)] == 56
    assert all(cap[s] == 64 for s in [(10, 400, 3, 39), (4, 130, 4, 39), (8, 96, 2, 39), (10, 20, 2, 39)])
    assert (39 * 10) % 8 != 0 and 130 % 4 == 2 and (130 + 3) // 4 == 33 and (20 + 3) // 4 == 5
    for D, N, H, F in pc.SPARSE_SHAPES:
        cfg, params, _, _ = pc.sparse_case(D, N, H, F, "A")
        for l in range(1, H + 1):  # groups of more than one staging unit in every layer
            lens = _lens(params, l)
            if (N if l > 1 else F * D) > cap[(D, N, H, F)]:
                assert (lens > cap[(D, N, H, F)]).any()
    # every group of the ecap = 8 shape with a row of nine or more nonzeros is multi-unit: most of them
    lens = _lens(pc.sparse_case(16, 512, 2, 39, "A")[1], 2)
    assert (lens.reshape(-1, 4).max(1) > 8).mean() > 0.7


@pytest.mark.parametrize("shape", pc.SPARSE_SHAPES, ids=_sid)
def test_pattern_b_turns_full_rows_empty_and_back(shape):
    D, N, H, F = shape
    a = pc.sparse_case(D, N, H, F, "A")[1]
    b = pc.sparse_case(D, N, H, F, "B")[1]
    for k in a:
        same = np.array_equal(a[k], b[k])
        if k.startswith("net_1_linear_"):  # the hidden layers are B's own (the biases keep B's rows alive)
            assert not same or k.endswith(".bias"), k
        else:
            assert same, k
    for l in range(1, H + 1):
        la, lb = _lens(a, l), _lens(b, l)
        K = a[f"net_1_linear_{l}.weight"].shape[1]
        assert np.array_equal(np.sort(la), np.sort(lb))
        assert (lb[la == K] == 0).all()
        nfull = int((la == K).sum())
        assert (lb[la == 0] == K).sum() == nfull > 0


def test_density_case_is_exactly_a_quarter():
    cfg, params, _, _ = pc.sparse_case(8, 96, 2, 39, "density")
    l1, l2 = _lens(params, 1), _lens(params, 2)
    assert (l1 == 78).all() and (l2 == 24).all() and params["net_1_linear_1.weight"].shape == (96, 312)
    assert float(l1.sum() + l2.sum()) / float(96 * 312 + 96 * 96) == 0.25
    assert np.nextafter(0.25, 0) < 0.25


@pytest.mark.parametrize("shape", list(pc.PAIR_SHAPES))
def test_pair_cases_have_the_promised_structure(shape):
    c = pc.PAIR_SHAPES[shape]
    F = c["F"]
    counts = pc.pair_counts(shape)
    assert counts[:2] == [0, 1]
    assert counts == [0, 1, 15, 16, 17, 31, 32, 33] or (F == 5 and counts == [0, 1, 10] and F * (F - 1) // 2 == 10)
    placed = set()
    for n in counts:
        cfg, params, xi, xv = pc.pairs_case(shape, n)
        assert len(xi) == pc.PAIR_ROWS == max(pc.PAIR_BATCHES)
        R = params["field_cov.weight"]
        lst = pc.pair_list(R)
        assert len(lst) == n
        assert [(k, l) for k, l, _ in lst] == sorted((k, l) for k, l, _ in lst) and all(k < l for k, l, _ in lst)
        listed, anti = pc.pair_plan(shape, n)
        assert sorted(listed) == [(k, l) for k, l, _ in lst]
        placed |= set(listed)
        # a nonzero diagonal everywhere; antisymmetric pairs wherever the list leaves a pair free
        assert np.diag(R).all()
        assert len(anti) == min(2, F * (F - 1) // 2 - n)
        for k, l in anti:
            assert R[k, l] == 1 and R[l, k] == -1
        if n == 0:
            assert R.any() and len(anti) >= 1 and (np.diag(R) != 0).sum() >= 1
        # the kinds of symmetrisation, by their place in the plan
        for i, (k, l) in enumerate(listed):
            a, b, w = pc.PAIR_KINDS[i % len(pc.PAIR_KINDS)]
            assert (R[k, l], R[l, k]) == (a, b) and dict(((p, q), x) for p, q, x in lst)[(k, l)] == w
        if n >= 15:
            kinds = {(R[k, l], R[l, k]) for k, l in listed}
            assert {(1.0, 0.0), (1.5, -0.5), (0.0, -1.0)} <= kinds
    want = pc.pair_placements(shape)
    assert set(want.values()) <= placed
    num = c["num"]
    if F >= 20:
        assert {"first", "corner", "last", "row_seam", "row15_col19", "row16", "col_seam"} <= set(want)
        assert want["row_seam"] == (15, 16) and want["row15_col19"] == (15, 19) and want["row16"] == (16, 17)
        assert want["col_seam"] == (3, 4) and want["corner"] == (0, F - 1) and want["last"] == (F - 2, F - 1)
    if num >= 2:
        k, l = want["num_num"]
        assert k < l < num
    if 0 < num < F:
        k, l = want["num_cat"]
        assert k < num <= l
    if c.get("qr"):
        k, l = want["qr_qr"]
        cfg = pc.pairs_case(shape, 33)[0]
        assert cfg["feature_sizes"][k] > cfg["qr_threshold"] and cfg["feature_sizes"][l] > cfg["qr_threshold"]
        assert f"fm_2nd_embeddings.{k}.weight_q" in pc.pairs_case(shape, 33)[1]
    # a one-pair list is not the same pair in every shape
    assert len({pc.pair_plan(s, 1)[0][0] for s in pc.PAIR_SHAPES}) >= 4


# ------------------------------------------------------------------------------------------- not degenerate
@pytest.mark.parametrize("case", SPARSE, ids=_sid)
def test_sparse_cases_are_not_degenerate(case):
    cfg, params, xi, xv = pc.sparse_case(*case)
    total, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    assert (parts["deep"] != 0).mean() >= 0.5
    assert len(np.unique(total.astype(np.float32))) >= 0.9 * len(total)
    assert (parts["second"] != 0).mean() >= 0.5


@pytest.mark.parametrize("case", PAIRS, ids=_sid)
def test_pair_cases_are_not_degenerate(case):
    cfg, params, xi, xv = pc.pairs_case(*case)
    total, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    assert len(np.unique(total.astype(np.float32))) >= 0.9 * len(total)
    if case[1] > 0:
        assert (parts["second"] != 0).all()
    else:
        assert (parts["second"] == 0).all()


# ------------------------------------------------------------------------------------------------ witnesses
def test_ell_emulation_layout():
    """The emulated build on a hand-made layer: k order, [j][u] interleave, (0, 0) pads up to the group's longest row
    rounded up to 8, a last group with missing neurons."""
    W = np.zeros((6, 20), dtype=np.float32)
    W[0, [3, 17]] = [1, -1]
    W[2, :9] = 0.5
    W[5, 19] = 2
    ek, ew, gcnt, cnt = pc.ell_build(W)
    assert gcnt.tolist() == [16, 8] and cnt.tolist() == [[2, 0, 9, 0], [0, 1, 0, 0]]
    assert ek[0, :2, 0].tolist() == [3, 17] and ew[0, :2, 0].tolist() == [1, -1]
    assert ek[0, :9, 2].tolist() == list(range(9)) and not ek[0, 9:, 2].any() and not ew[0, 9:, 2].any()
    assert (ek[1, 0, 1], ew[1, 0, 1]) == (19, 2) and not ew[1, 1:].any()
    x = np.arange(40, dtype=np.float32).reshape(2, 20)
    b = np.array([1, -1, 0, 5, 0, -100], dtype=np.float32)
    ref = np.maximum(x @ W.T + b, 0)
    assert np.array_equal(pc.ell_walk(x, (ek, ew, gcnt, cnt), b)[:, :6], ref)
    assert np.array_equal(pc.ell_walk(x, (ek, ew, gcnt, cnt), b, [1])[:, :2], ref[:, 4:6])


@pytest.mark.parametrize("case", SPARSE, ids=_sid)
def test_ell_emulation_equals_the_oracle(case):
    args = pc.sparse_case(*case)
    assert np.array_equal(pc.sparse_emul(*args), pc.sparse_ref(*case))


@pytest.mark.parametrize("shape", pc.SPARSE_SHAPES, ids=_sid)
def test_every_ell_mutation_changes_a_logit(shape):
    """One dropped, duplicated, shifted or misplaced entry, at every place the case promises, shows in at least one
    row's float32 logit: the bit equality of the GPU leg cannot hold for a kernel that makes that mistake."""
    D, N, H, F = shape
    args = pc.sparse_case(D, N, H, F, "A")
    cfg, params = args[:2]
    ref = pc.sparse_ref(D, N, H, F, "A")
    _, parts = dfwfm_oracle.forward(*args, return_parts=True)
    sites = pc.sparse_sites(D, N, H, F)
    cap = pc.ecap(F * D, N)
    todo = [(l, n // 4, m, n % 4) for (l, n) in sites["rows"] for m in pc.ROW_MUTATIONS]
    todo += [(l, n // 4, m, n % 4) for (l, n) in sites["seams"] for m in pc.SEAM_MUTATIONS]
    for l, g in sites["groups"]:
        lens = _lens(params, l)[4 * g:4 * g + 4]
        u = int(np.argmax(lens))  # the longest row changes places with its neighbour
        if 4 * g + (u + 1) % 4 >= N:
            u -= 1
        todo += [(l, g, "swap_neurons", u), (l, g, "stop_short", None), (l, g, "skip_bias", None)]
    todo += [(l, g, "skip_bias", None) for l, g in pc.bias_groups(N, H)]
    assert {l for l, *_ in todo} == set(range(1, H + 1))
    for l in range(1, H + 1):  # every layer has every kind of site; the seams where a layer is wider than a unit
        kinds = {m for ll, _, m, _ in todo if ll == l}
        K = F * D if l == 1 else N
        assert set(pc.ROW_MUTATIONS + pc.GROUP_MUTATIONS) <= kinds
        assert (set(pc.SEAM_MUTATIONS) <= kinds) == (K > cap)
    blind = [m for m in todo if np.array_equal(pc.sparse_emul(*args, mutation=m, parts=parts), ref)]
    assert not blind, blind


@pytest.mark.parametrize("case", PAIRS, ids=_sid)
def test_pair_emulation_equals_the_oracle_and_every_mutation_shows(case):
    shape, n = case
    args = pc.pairs_case(shape, n)
    ref = pc.pairs_ref(shape, n)
    _, parts = dfwfm_oracle.forward(*args, return_parts=True)
    assert np.array_equal(pc.pairs_emul(*args, parts=parts), ref)
    F = pc.PAIR_SHAPES[shape]["F"]
    for m in pc.PAIR_MUTATIONS:
        got = pc.pairs_emul(*args, mutation=m, parts=parts)
        if got is None:  # nothing to drop in an empty list; no free pair for an antisymmetric one
            assert (n == 0 and m in ("drop_first", "drop_last", "halve_twice")) or \
                (m == "keep_antisymmetric" and n == F * (F - 1) // 2), (case, m)
            continue
        assert not np.array_equal(got, ref), (case, m)
