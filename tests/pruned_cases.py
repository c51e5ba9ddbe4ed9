"""Helper (no tests): structured pruned models on which every operation of the forward is exact in float32, for the
two list-walking inference paths -- the sparse deep tower (csrc/dfwfm_spmlp.hip) and the FwFM pair list
(dfwfm_model_build_fwfm_pairs, fwd_kernel PART 3) -- and numpy emulations of both lists that take one mutation at a
time (a dropped, duplicated or misplaced entry).

Shared by tests/test_pruned_cases.py (the cases are exact, have the structure they promise, are not degenerate, and
every mutation of the lists changes a logit) and tests/test_gpu_pruned_exact.py (the kernels give the float64 oracle's
float32 bits).

Random magnitude pruning leaves every row of a 390/400-wide layer with 25 to 55 nonzeros; these cases set each row's
length by position instead: the lengths around the padding unit (8), the staging unit (64 entries, or 56 / 8 where the
x tile leaves less LDS) and the layer width, groups of four neurons with one full and three empty rows, and pair
lists whose lengths sit at the lanes-per-sample boundaries of the kernel (16 and 32).

Exactness: tables and Xv are small integers, weights come from {+-1, +-0.5}, so every term is a multiple of a
quantum q and every sum of absolute terms stays below 2^24 q: any partial sum in any order is a float32 (the CPU
leg asserts the bound; nothing here relies on it silently)."""
import functools

import numpy as np

from conftest import model_kwargs
from oracle import dfwfm_oracle

# ---------------------------------------------------------------------------------------------- sparse tower
CYCLE = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 56, 63, 64, 65, 71, 72, 127, 128, 129]
# (D, N, H, F); 13 numerical fields
SPARSE_SHAPES = [(10, 400, 3, 39), (4, 130, 4, 39), (8, 96, 2, 39), (16, 512, 2, 39), (16, 400, 3, 36), (10, 20, 2, 39)]
SPARSE_BATCHES = [1, 64, 65, 129]
ROWS = 129
PATTERNS = ["F000", "0F00", "00F0", "000F", "0000", "equal", "kk", "kk_top"]
ELL_PAD = 8      # kEllPad
SP_CAP = 64      # kSpCap
SP_WAVES = 8     # kSpW
SP_ROWS = 64     # kSpS


def ecap(K0, N):
    """Entries of a group the sparse kernel stages at once (sparse_mlp_cap): 64, or what 160 KiB of LDS leave beside
    the x tile [max(K0p, N)][64] and the reduction rows, rounded down to a multiple of 8.  K0p: K0 padded to 16."""
    K0p = (K0 + 15) // 16 * 16
    XK = max(K0p, N)
    room = (160 * 1024 - 4 * (XK * SP_ROWS + SP_WAVES * SP_ROWS)) // (16 * 2 * SP_WAVES)
    return SP_CAP if room >= SP_CAP else room // 8 * 8


def pattern_groups(N, layer):
    """{pattern name: group index} of hidden layer `layer` (1-based).  The groups of N-2 and N-1 are kept for the
    near-full and full last rows; a layer with at least eight other groups holds every pattern (at a start that moves
    with the layer, so that the patterns meet other waves and other positions of a wave's group list), a smaller one
    the next slice of PATTERNS, so that the layers together hold them all."""
    free = (N - 2) // 4
    if free >= len(PATTERNS):
        start = min(5 * (layer - 1), free - len(PATTERNS))
        return {p: start + i for i, p in enumerate(PATTERNS)}
    return {PATTERNS[((layer - 1) * free + i) % len(PATTERNS)]: i for i in range(free)}


def pattern_lengths(name, K):
    if name == "0000":
        return [0, 0, 0, 0]
    if name == "equal":
        return [min(65, K - 3)] * 4
    if name == "kk":
        return [1, 2, 8, 9]
    if name == "kk_top":
        return [K - 9, K - 8, K - 2, K - 1]
    return [K if c == "F" else 0 for c in name]


def row_lengths(K, N, layer):
    """Nonzeros per row of a hidden layer with K inputs and N neurons, set by position: the pattern groups, CYCLE
    (clipped to K) over the other neurons in order, then row N-2 with K-1 and the last row, N-1, with K nonzeros."""
    lens = np.full(N, -1, dtype=np.int64)
    for name, g in pattern_groups(N, layer).items():
        lens[4 * g:4 * g + 4] = pattern_lengths(name, K)
    rest = np.flatnonzero(lens < 0)
    lens[rest] = [min(CYCLE[i % len(CYCLE)], K) for i in range(len(rest))]
    lens[N - 2] = K - 1
    lens[N - 1] = K
    return lens


def permuted_lengths(lens):
    """The lengths mirrored by rank: the i-th shortest row gets the i-th longest row's length, so every full row
    becomes empty and the empty rows become the longest."""
    order = np.argsort(lens, kind="stable")
    out = np.empty_like(lens)
    out[order] = lens[order[::-1]]
    return out


def _hidden_layer(rs, lens, x, vals):
    """(W, b) of a hidden layer with the given row lengths over the inputs x [rows, K] (float64, this case's own).
    A list entry that only ever multiplies zeros, or a row that ReLU always clips, could be dropped without a trace,
    so: short rows read live inputs only (columns of x that are nonzero on a quarter of the rows), every row with entries is drawn again
    until its sum is positive on a quarter of the rows and each of its live inputs is nonzero on four of those, and the
    empty rows get a positive bias -- but the second of
    them, whose bias is negative (ReLU of the bias alone, both ways).  Biases are nonzero."""
    N, K = len(lens), x.shape[1]
    live = np.flatnonzero((x != 0).mean(0) >= 0.25)
    dead = np.setdiff1d(np.arange(K), live)
    W = np.zeros((N, K), dtype=np.float32)
    b = np.zeros(N, dtype=np.float32)
    empties = np.flatnonzero(lens == 0)
    for n, L in enumerate(lens):
        L = int(L)
        if L == 0:
            b[n] = -2 if (len(empties) > 1 and n == empties[1]) else 1 + (n % 3)
            continue
        for attempt in range(200):
            if L == 1:
                pos = live[[(n * 37 + attempt) % len(live)]]
            elif L == K:
                pos = np.arange(K)
            elif L > len(live):
                pos = np.concatenate([live, rs.choice(dead, size=L - len(live), replace=False)])
            else:
                pos = rs.choice(live, size=L, replace=False)
                must = {0: 0, 1: K - 1}.get(n % 5)  # k = 0 and k = K-1 also in short rows
                if must is not None and must not in pos:
                    pos[0] = must
            w = rs.choice(vals, size=L)
            bias = rs.choice([-1, 1, 2]) if attempt < 20 else 2
            z = x[:, pos] @ w + bias
            seen = (x[z > 0][:, pos] != 0).sum(0)  # per entry: the rows where it counts and ReLU lets it through
            if (z > 0).mean() >= 0.25 and z.std() > 0 and (seen[np.isin(pos, live)] >= 4).all():
                break
        else:
            raise AssertionError(f"row {n} of length {L} stays dead")
        W[n, pos] = w
        b[n] = bias
    return W, b


def _exact_shallow(rs, shapes, params, positive_tables=False):
    """The tables and the shallow parameters: small integers and multiples of 0.5."""
    for k, shp in shapes.items():
        if k.startswith("fm_2nd_embeddings") or k.startswith("fm_1st_embeddings"):
            if positive_tables and k.startswith("fm_2nd"):
                v = rs.randint(1, 8, size=shp)
            elif positive_tables:  # (first order: spread, so that the few rows of a pair case have their own logits)
                v = rs.randint(-60, 61, size=shp)
            else:
                v = rs.randint(-1, 2, size=shp)
                if shp[0] == 1:  # a numerical field's single row: nonzero, and no two neighbours equal (columns k and
                    s0 = rs.randint(4)  # k + 1 of E are that row times the same Xv: an entry shifted by one must show)
                    v = np.array([[1, -1, 2, -2][(d + s0) % 4] for d in range(shp[1])]).reshape(shp)
            params[k] = v.astype(np.float32)
        elif k == "fm_1st.weight":
            params[k] = rs.choice([0.5, -0.5, 1.0, -1.0], size=shp).astype(np.float32)
        elif k == "fwfm_linear.weight":
            params[k] = rs.choice([0.5, -0.5, 1.0, -1.0], size=shp).astype(np.float32)
        elif k == "bias":
            params[k] = np.full(shp, 2.0, dtype=np.float32)


def _inputs(rs, sizes, num, rows, xv_low):
    xi = np.stack([rs.randint(0, s, size=rows) for s in sizes[num:]], axis=1).astype(np.int64) if len(sizes) > num \
        else np.zeros((rows, 0), dtype=np.int64)
    xv = rs.randint(xv_low, xv_low + 3, size=(rows, num)).astype(np.float32)
    return xi, xv


@functools.lru_cache(maxsize=None)
def sparse_case(D, N, H, F=39, variant="A"):
    """(cfg, params, xi, xv) with ROWS rows; computed once, shared, never modified.  variant "A": the structured row
    lengths of row_lengths(); "B": the same model with A's lengths mirrored by rank (permuted_lengths) and fresh
    positions and signs; "density": every row of layer l holds exactly K_l / 4 nonzeros (K_l divisible by 4), so the
    hidden layers' density is exactly 0.25 in double."""
    from xsdeepfwfm_deprecated_amd import DeepFMs
    num = 13
    sizes = [1] * num + [int(x) for x in 50 + (np.arange(F - num) * 37) % 400]
    cfg = dict(field_size=F, feature_sizes=sizes, embedding_size=D, use_fwfm=1, use_fm=0, use_logit=0,
               use_deep=1, use_lw=1, use_fwlw=0, h_depth=H, deep_nodes=N, numerical=num, embedding_bag=0,
               qr_flag=0, qr_operation="mult", qr_collisions=4, qr_threshold=200)
    shapes = {k: tuple(v.shape) for k, v in DeepFMs(**model_kwargs(cfg)).state_dict().items()}
    rs = np.random.RandomState(1000 * D + N + H + F)
    params = {}
    _exact_shallow(rs, shapes, params)
    r = rs.choice([0.0, 0.0, 0.0, 0.5, -0.5, 1.0, -1.0], size=(F, F))
    params["field_cov.weight"] = (np.triu(r, 1) + np.triu(r, 1).T).astype(np.float32)
    rw = np.random.RandomState(77 + 1000 * D + N + H + F + {"A": 0, "B": 1, "density": 2}[variant])
    sites = sparse_sites(D, N, H, F)
    xi, xv = _inputs(rs, sizes, num, ROWS, 0)
    x = dfwfm_oracle.embeddings(cfg, params, xi, xv).reshape(ROWS, -1)
    for l in range(1, H + 1):
        K = F * D if l == 1 else N
        if variant == "density":
            assert K % 4 == 0
            lens = np.full(N, K // 4, dtype=np.int64)
        else:
            lens = row_lengths(K, N, l)
            if variant == "B":
                lens = permuted_lengths(lens)
        vals = [1.0, -1.0, 0.5, -0.5] if l == 1 else [1.0, -1.0]
        W, b = _hidden_layer(rw, lens, x, vals)
        params[f"net_1_linear_{l}.weight"], params[f"net_1_linear_{l}.bias"] = W, b
        x = np.maximum(x @ W.T.astype(np.float64) + b.astype(np.float64), 0.0)
    fc = rs.choice([0.5, -0.5, 1.0, -1.0], size=N)
    # zeros only where no witness looks; the four neurons of a witnessed group get four different weights, or two of
    # them could change places unseen
    site_groups = [g for (l, g) in sites["groups"] + bias_groups(N, H) if l == H]
    keep = {n for (l, n) in sites["rows"] + sites["seams"] if l == H} | {4 * g + u for g in site_groups for u in range(4)}
    fc[[n for n in range(N) if n % 7 == 3 and n not in keep]] = 0.0
    emptyH = np.flatnonzero(row_lengths(F * D if H == 1 else N, N, H) == 0)  # (variant A's, whatever the variant)
    bH = np.array([1 + n % 3 if (n in emptyH and n != emptyH[1]) else 0 for n in range(N)])
    for g in site_groups:
        sl = slice(4 * g, min(4 * g + 4, N))
        fc[sl] = rs.permutation([1.0, -1.0, 0.5, -0.5])[:sl.stop - sl.start]
        for _ in range(50):  # the biases of a group's empty rows must not cancel in the output
            if not bH[sl].any() or fc[sl] @ bH[sl] != 0:
                break
            fc[sl] = rs.permutation([1.0, -1.0, 0.5, -0.5])[:sl.stop - sl.start]
    params["net_1_fc.weight"] = fc.reshape(1, N).astype(np.float32)
    assert set(params) == set(shapes), set(shapes) ^ set(params)
    return cfg, params, xi, xv


def sparse_sites(D, N, H, F=39):
    """Where the witnesses mutate variant A's lists: `rows` (layer, neuron) -- per layer the first row of each pinned
    length and every full row; `groups` (layer, group) -- the pattern groups that hold entries and the last group;
    `seams` (layer, neuron) -- the first rows longer than the staging unit."""
    cap = ecap(F * D, N)
    rows, groups, seams = [], [], []
    for l in range(1, H + 1):
        K = F * D if l == 1 else N
        lens = row_lengths(K, N, l)
        for L in sorted({min(c, K) for c in (1, 7, 8, 9, 63, 64, 65)} | {K - 1}):
            if (lens == L).any():  # (N = 20 has room for few of them)
                rows.append((l, int(np.flatnonzero(lens == L)[0])))
        rows += [(l, int(n)) for n in np.flatnonzero(lens == K)]
        pg = pattern_groups(N, l)
        groups += [(l, g) for p, g in pg.items() if p != "0000"] + [(l, (N - 1) // 4)]
        long_rows = np.flatnonzero(lens > cap)
        seams += [(l, int(n)) for n in long_rows[:6]]
    return dict(rows=sorted(set(rows)), groups=sorted(set(groups)), seams=seams)


def bias_groups(N, H):
    """(layer, group) of the all-empty groups: ReLU of the bias alone."""
    return [(l, pattern_groups(N, l)["0000"]) for l in range(1, H + 1) if "0000" in pattern_groups(N, l)]


# ---- the ELL of dfwfm_spmlp.hip in numpy: build, then walk -----------------------------------------------------
def ell_build(W):
    """ell_build_kernel: neurons in groups of four; a group's slot holds each row's nonzero (k, w) in k order,
    interleaved [entry j][neuron u], the shorter rows padded with (0, 0) up to the group's longest row rounded up to
    a multiple of 8.  Returns (ek [G, Wd, 4] int, ew [G, Wd, 4] float32, gcnt [G], cnt [G, 4])."""
    N, K = W.shape
    G = (N + 3) // 4
    Wd = (K + ELL_PAD - 1) // ELL_PAD * ELL_PAD
    ek = np.zeros((G, Wd, 4), dtype=np.int64)
    ew = np.zeros((G, Wd, 4), dtype=np.float32)
    cnt = np.zeros((G, 4), dtype=np.int64)
    for n in range(N):
        k = np.flatnonzero(W[n] != 0)
        g, u = divmod(n, 4)
        ek[g, :len(k), u] = k
        ew[g, :len(k), u] = W[n, k]
        cnt[g, u] = len(k)
    gcnt = (cnt.max(1) + ELL_PAD - 1) // ELL_PAD * ELL_PAD
    return ek, ew, gcnt, cnt


def ell_walk(x, ell, bias, groups=None):
    """sparse_mlp_kernel's sums for the listed groups (default: all): from the bias, entry by entry in k order, in
    float32; then ReLU.  x [B, K] float32 -> [B, 4 * len(groups)] float32 (neurons past N: the padded zero bias)."""
    ek, ew, gcnt, _ = ell
    groups = np.arange(len(gcnt)) if groups is None else np.asarray(groups)
    x = np.ascontiguousarray(x, dtype=np.float32)
    bp = np.zeros(4 * len(gcnt), dtype=np.float32)
    bp[:len(bias)] = bias
    acc = np.repeat(bp.reshape(-1, 4)[groups][None], x.shape[0], axis=0)  # [B, g, 4]
    for j in range(int(gcnt[groups].max(initial=0))):
        live = (gcnt[groups] > j)[None, :, None]
        term = (ew[groups, j][None] * x[:, ek[groups, j]]).astype(np.float32)
        acc = np.where(live, (acc + term).astype(np.float32), acc)
    return np.maximum(acc, np.float32(0)).reshape(x.shape[0], -1)


ROW_MUTATIONS = ["drop_first", "drop_last", "duplicate", "shift_k"]
SEAM_MUTATIONS = ["drop_before_seam", "drop_after_seam"]
GROUP_MUTATIONS = ["swap_neurons", "stop_short", "skip_bias"]


def mutate_group(ell, bias, K, g, mutation, u=None, cap=SP_CAP):
    """One group's (ek, ew, gcnt, bias4) after one mutation of the build or the walk; u: the row (row and seam
    mutations).  The result feeds walk_group."""
    ek, ew, gcnt, cnt = ell
    k, w, c = ek[g].copy(), ew[g].copy(), cnt[g].copy()
    b = np.zeros(4, dtype=np.float32)
    nb = bias[4 * g:4 * g + 4]
    b[:len(nb)] = nb
    n = int(gcnt[g])

    def drop(j):
        k[j:-1, u], w[j:-1, u] = k[j + 1:, u].copy(), w[j + 1:, u].copy()
        k[c[u] - 1, u], w[c[u] - 1, u] = 0, 0

    if mutation == "drop_first":
        drop(0)
    elif mutation == "drop_last":
        drop(c[u] - 1)
    elif mutation == "drop_before_seam":
        drop(cap - 1)
    elif mutation == "drop_after_seam":
        drop(cap)
    elif mutation == "duplicate":  # the middle entry twice (the group's count grows with it where it must)
        j = c[u] // 2
        if c[u] == k.shape[0]:
            k, w = np.concatenate([k, np.zeros((ELL_PAD, 4), k.dtype)]), np.concatenate([w, np.zeros((ELL_PAD, 4), w.dtype)])
        k[j + 1:c[u] + 1, u], w[j + 1:c[u] + 1, u] = k[j:c[u], u].copy(), w[j:c[u], u].copy()
        n = max(n, (c[u] + 1 + ELL_PAD - 1) // ELL_PAD * ELL_PAD)
    elif mutation == "shift_k":
        j = c[u] // 2
        k[j, u] += 1 if k[j, u] + 1 < K else -1
    elif mutation == "swap_neurons":  # rows u and u + 1 (mod 4) change places; the biases stay
        v = (u + 1) % 4
        k[:, [u, v]], w[:, [u, v]] = k[:, [v, u]], w[:, [v, u]]
    elif mutation == "stop_short":  # the walk ends one entry before the group's longest row does
        w[c.max() - 1] = 0
    elif mutation == "skip_bias":
        b[:] = 0
    else:
        raise KeyError(mutation)
    return k, w, n, b


def walk_group(x, mutated):
    k, w, n, b = mutated
    ell = (k[None], w[None], np.array([n]), None)
    return ell_walk(x, ell, b, [0])


def sparse_emul(cfg, params, xi, xv, mutation=None, parts=None):
    """Float32 logits with the deep tower computed by the ELL emulation: ((first + second) + deep) + bias as the
    kernel combines them.  mutation = (layer, group, name, u): that group of that layer is built or walked wrongly;
    the layers behind it are dense float64 products, which the exactness of the case makes the same numbers.
    parts: the oracle's parts of these inputs, where the caller has them."""
    if parts is None:
        _, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    B, H, N = len(xi), cfg["h_depth"], cfg["deep_nodes"]
    x = parts["E"].reshape(B, -1).astype(np.float32)
    cap = ecap(x.shape[1], N)
    for l in range(1, H + 1):
        W = params[f"net_1_linear_{l}.weight"]
        b = params[f"net_1_linear_{l}.bias"]
        if mutation is None:
            x = ell_walk(x, ell_build(W), b)[:, :N]
            continue
        h = np.maximum(x.astype(np.float64) @ W.T.astype(np.float64) + b.astype(np.float64), 0.0).astype(np.float32)
        if l == mutation[0]:
            _, g, name, u = mutation
            sub = W[4 * g:4 * g + 4]
            ell = ell_build(sub)
            got = walk_group(x, mutate_group(ell, b[4 * g:4 * g + 4], W.shape[1], 0, name, u, cap))
            h[:, 4 * g:4 * g + len(sub)] = got[:, :len(sub)]
        x = h
    deep = x.astype(np.float64) @ params["net_1_fc.weight"][0].astype(np.float64)
    total = ((parts["first"] + parts["second"]) + deep) + float(params["bias"][0])
    return total.astype(np.float32)


# ------------------------------------------------------------------------------------------------- pair list
PAIR_SHAPES = {
    "F39-D10": dict(F=39, num=13, D=10),
    "F39-D10-fwlw": dict(F=39, num=13, D=10, fwlw=1, lw=0),
    "F64-D16": dict(F=64, num=0, D=16),
    "F5-D4": dict(F=5, num=2, D=4),
    "F39-D32": dict(F=39, num=13, D=32),
    "F39-D10-qr": dict(F=39, num=13, D=10, qr=1),
}
PAIR_BATCHES = [1, 17, 33]
PAIR_ROWS = 33
# R[k,l], R[l,k] of a listed pair by its place in the list, and the weight (R[k,l] + R[l,k]) / 2 it must get
PAIR_KINDS = [(1.0, 0.0, 0.5), (1.5, -0.5, 0.5), (0.5, 0.5, 0.5), (0.0, -1.0, -0.5), (1.0, 1.0, 1.0)]


def pair_counts(shape):
    """Pairs after symmetrisation: around the 16 and 32 lanes a sample has on the two kernel forms.  Five fields have
    ten pairs: 0, 1 and all ten (the list at its capacity F (F - 1) / 2) there."""
    F = PAIR_SHAPES[shape]["F"]
    return [n for n in (0, 1, 15, 16, 17, 31, 32, 33) if n <= F * (F - 1) // 2 - 2] + ([10] if F == 5 else [])


def _pair_sizes(F, num):
    return [1] * num + [int(x) for x in 40 + (np.arange(F - num) * 53) % 700]


def pair_placements(shape):
    """{name: (k, l)}: the seams of the packed (R + R^T)/2 the builder decodes (16 rows, 4 columns), the corners, and
    the kinds of field.  Pairs that the shape does not have are left out."""
    c = PAIR_SHAPES[shape]
    F, num = c["F"], c["num"]
    out = {"first": (0, 1), "corner": (0, F - 1), "last": (F - 2, F - 1), "row_seam": (15, 16), "row15_col19": (15, 19),
           "row16": (16, 17), "col_seam": (3, 4)}
    if num >= 3:
        out["num_num"] = (1, 2)
    elif num == 2:
        out["num_num"] = (0, 1)
    if 0 < num < F:
        out["num_cat"] = (num - 1, num)
    if c.get("qr"):
        big = [num + j for j, s in enumerate(_pair_sizes(F, num)[num:]) if s > 200]
        out["qr_qr"] = (big[0], big[1])
    return {k: v for k, v in out.items() if v[1] < F}


def pair_plan(shape, n):
    """(listed, anti): the n pairs (k, l), k < l, that survive symmetrisation, in the order their kinds are dealt (the
    placements first, rotated by the shape so that a one-pair list is not always (0, 1)), and up to two antisymmetric
    pairs that must be dropped."""
    F = PAIR_SHAPES[shape]["F"]
    prio = list(dict.fromkeys(pair_placements(shape).values()))
    rot = list(PAIR_SHAPES).index(shape) % len(prio)
    prio = prio[rot:] + prio[:rot]
    rest = [(k, l) for k in range(F) for l in range(k + 1, F) if (k, l) not in prio]
    rs = np.random.RandomState(F + n)
    rest = [rest[i] for i in rs.permutation(len(rest))]
    order = prio + rest
    return order[:n], order[n:n + 2]


@functools.lru_cache(maxsize=None)
def pairs_case(shape, n):
    """(cfg, params, xi, xv) of an MLP-free FwFM model whose field_cov leaves exactly n pairs, PAIR_ROWS rows;
    computed once, shared, never modified.  Second-order tables and Xv are positive integers, so no pair's inner
    product is zero; field_cov also holds a nonzero diagonal and antisymmetric pairs, which the list must ignore."""
    from xsdeepfwfm_deprecated_amd import DeepFMs
    c = PAIR_SHAPES[shape]
    F, num, D, qr = c["F"], c["num"], c["D"], c.get("qr", 0)
    sizes = _pair_sizes(F, num)
    cfg = dict(field_size=F, feature_sizes=sizes, embedding_size=D, use_fwfm=1, use_fm=0, use_logit=0, use_deep=0,
               use_lw=c.get("lw", 1), use_fwlw=c.get("fwlw", 0), h_depth=3, deep_nodes=400, numerical=num,
               embedding_bag=int(qr), qr_flag=qr, qr_operation="mult", qr_collisions=4, qr_threshold=200)
    shapes = {k: tuple(v.shape) for k, v in DeepFMs(**model_kwargs(cfg)).state_dict().items()}
    rs = np.random.RandomState(list(PAIR_SHAPES).index(shape) * 100 + n)
    params = {}
    _exact_shallow(rs, shapes, params, positive_tables=True)
    R = np.zeros((F, F), dtype=np.float32)
    listed, anti = pair_plan(shape, n)
    for i, (k, l) in enumerate(listed):
        R[k, l], R[l, k], _ = PAIR_KINDS[i % len(PAIR_KINDS)]
    for k, l in anti:
        R[k, l], R[l, k] = 1.0, -1.0
    R[np.arange(F), np.arange(F)] = rs.choice([0.5, -1.0, 1.5], size=F)
    params["field_cov.weight"] = R
    assert set(params) == set(shapes), set(shapes) ^ set(params)
    xi, xv = _inputs(rs, sizes, num, PAIR_ROWS, 1)
    return cfg, params, xi, xv


def pair_list(R):
    """dfwfm_model_build_fwfm_pairs: the nonzero strictly-upper entries of (R + R^T) / 2 in float32, k-major:
    [(k, l, w)]."""
    R = np.asarray(R, dtype=np.float32)
    S = ((R + R.T) * np.float32(0.5)).astype(np.float32)
    F = R.shape[0]
    return [(k, l, S[k, l]) for k in range(F) for l in range(k + 1, F) if S[k, l] != 0]


PAIR_MUTATIONS = ["drop_first", "drop_last", "halve_twice", "keep_antisymmetric", "read_diagonal"]


def pairs_emul(cfg, params, xi, xv, mutation=None, parts=None):
    """Float32 logits with the second order summed over the emulated pair list (w * <E_k, E_l> pair by pair, in list
    order, float32), one mutation of the builder at a time.  None when the case has no place for the mutation."""
    if parts is None:
        _, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    R = params["field_cov.weight"]
    lst = pair_list(R)
    F = R.shape[0]
    if mutation == "drop_first" or mutation == "drop_last":
        if not lst:
            return None
        lst = lst[1:] if mutation == "drop_first" else lst[:-1]
    elif mutation == "halve_twice":  # a one-sided R[k,l] halved again
        one = [i for i, (k, l, w) in enumerate(lst) if (R[k, l] == 0) != (R[l, k] == 0)]
        if not one:
            return None
        k, l, w = lst[one[0]]
        lst[one[0]] = (k, l, np.float32(0.5) * w)
    elif mutation == "keep_antisymmetric":  # R[k,l] listed where R[k,l] + R[l,k] = 0
        anti = [(k, l) for k in range(F) for l in range(k + 1, F) if R[k, l] != 0 and R[k, l] + R[l, k] == 0]
        if not anti:
            return None
        lst = sorted(lst + [(anti[0][0], anti[0][1], R[anti[0]])])
    elif mutation == "read_diagonal":
        lst = sorted(lst + [(0, 0, R[0, 0])])
    elif mutation is not None:
        raise KeyError(mutation)
    E = parts["E"].astype(np.float32)
    second = np.zeros(len(xi), dtype=np.float32)
    for k, l, w in lst:
        dot = np.zeros(len(xi), dtype=np.float32)
        for d in range(E.shape[2]):
            dot = (E[:, k, d] * E[:, l, d] + dot).astype(np.float32)
        second = (np.float32(w) * dot + second).astype(np.float32)
    bias = float(params["bias"][0])
    return ((parts["first"] + second.astype(np.float64)) + bias).astype(np.float32)


# ---------------------------------------------------------------------------------------------- shared oracle
@functools.lru_cache(maxsize=None)
def sparse_ref(D, N, H, F=39, variant="A"):
    """The float64 oracle's logits of sparse_case cast to float32; computed once, shared, never modified."""
    return dfwfm_oracle.forward(*sparse_case(D, N, H, F, variant)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pairs_ref(shape, n):
    return dfwfm_oracle.forward(*pairs_case(shape, n)).astype(np.float32)
