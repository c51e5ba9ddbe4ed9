"""Helper (no tests): the numeric contract of the bf16 deep tower (include/dfwfm_bf16.h) in numpy, the shapes the
bf16 tests share, and a Criteo-39-shaped case on which every rounding of the contract is a no-op."""
import functools

import numpy as np

from conftest import load_golden, model_kwargs
from oracle import dfwfm_oracle

DEEP_GOLDENS = ["deepfwfm_lw", "deepfwfm_fwlw_lw", "deepfwfm_fwlw_nolw", "deepfwfm_embbag", "deepfwfm_qr_mult",
                "deepfwfm_qr_add_fwlw", "deepfwfm_pruned", "deepfwfm_small_mlp", "fm_deep", "tiny_deepfwfm_lw"]
# (F, num, D, N, H, fwlw, seed): the serve sweep's shapes and seeds plus N = 100 (7 tiles, 4 padded neurons, H = 4),
# then the limits of the layout (64 fields, no numerical field, only numerical fields, five hidden layers)
SWEEP = [(39, 13, D, N, H, fwlw, D * 1000 + N + H)
         for D, N, H, fwlw in [(10, 400, 3, 0), (10, 144, 2, 1), (4, 256, 1, 0), (16, 512, 2, 0), (8, 96, 3, 1),
                               (32, 400, 1, 0), (10, 340, 2, 0), (10, 100, 4, 0)]]
SWEEP += [(F, num, D, N, H, 0, F + num + D + N + H)
          for F, num, D, N, H in [(64, 16, 10, 256, 5), (20, 0, 8, 128, 2), (39, 39, 4, 64, 1)]]
SWEEP_ROWS = 96


def bf16_rne(x):
    """float32 array -> the float32 array of its bf16 roundings (round to nearest, ties to even; NaN stays NaN)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), np.float32(np.nan), r).astype(np.float32)


def forward(cfg, params, xi, xv, acc=np.float64, k_order=None):
    """Logits (float64 array) of the contract: E and the shallow terms from the float64 oracle, the tower with the
    contract's rounding points.  acc: the accumulator of the layers' sums and of deep.  k_order = (seed, chunk) with
    acc = float32 models another kernel's summation order: K is shuffled, cut into chunks, each chunk's partial
    product is formed in float32 and the partials are added in float32 in turn."""
    _, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    B = np.asarray(xi).shape[0]
    shallow = parts["first"] + parts["second"]
    x = bf16_rne(parts["E"].astype(np.float32).reshape(B, -1))
    H = cfg["h_depth"]
    h = None
    for l in range(1, H + 1):
        wb = bf16_rne(np.asarray(params[f"net_1_linear_{l}.weight"], dtype=np.float32))
        bias = np.asarray(params[f"net_1_linear_{l}.bias"], dtype=np.float32).astype(acc)
        K = wb.shape[1]
        if k_order is None:
            z = x.astype(acc) @ wb.T.astype(acc)
        else:
            seed, chunk = k_order
            perm = np.random.RandomState(seed + l).permutation(K)
            z = np.zeros((B, wb.shape[0]), dtype=acc)
            for c in range(0, K, chunk):
                idx = perm[c:c + chunk]
                z = (z + x[:, idx].astype(acc) @ wb[:, idx].T.astype(acc)).astype(acc)
        h = np.maximum(z + bias, acc(0))  # np.maximum keeps NaN, as relu_keep_nan
        if l < H:
            x = bf16_rne(h.astype(np.float32))
    fc = np.asarray(params["net_1_fc.weight"], dtype=np.float32)[0].astype(acc)
    deep = (h @ fc).astype(np.float64)
    bias = float(np.asarray(params["bias"], dtype=np.float64)[0]) if "bias" in params else 0.0
    return (shallow + deep) + bias


def sweep_case(F, num, D, N, H, fwlw, seed, rows=SWEEP_ROWS):
    """A synthetic DeepFwFM config (small tables) with its params and inputs: the recipe of the serve tests' sweep."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = [1] * num + [int(x) for x in 50 + (np.arange(F - num) * 37) % 400]
    cfg = dict(field_size=F, feature_sizes=sizes, embedding_size=D, use_fwfm=1, use_fm=0, use_logit=0,
               use_deep=1, use_lw=1, use_fwlw=int(fwlw), h_depth=H, deep_nodes=N, numerical=num,
               embedding_bag=0, qr_flag=0, qr_operation="mult", qr_collisions=4, qr_threshold=200)
    m = DeepFMs(**model_kwargs(cfg))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    params = synth.synth_state(shapes, F, D, N, True, True, seed=seed)
    xi, xv = synth.synth_inputs(sizes, num, rows, seed=seed)
    return cfg, params, xi, xv


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """(cfg, params, xi, xv, y, ref64, emul64) of a deep golden's first 256 rows (tiny_deepfwfm_lw: all 2000);
    computed once, shared, never modified."""
    cfg, params, xi, xv, y, l32, l64, auc = load_golden(name)
    n = xi.shape[0] if name == "tiny_deepfwfm_lw" else 256
    xi, xv, y, l64 = xi[:n], xv[:n], y[:n], l64[:n]
    return cfg, params, xi, xv, y, np.asarray(l64, dtype=np.float64), forward(cfg, params, xi, xv)


@functools.lru_cache(maxsize=None)
def sweep_ref(i):
    """(cfg, params, xi, xv, ref64, emul64) of SWEEP[i]; computed once, shared, never modified."""
    cfg, params, xi, xv = sweep_case(*SWEEP[i])
    return cfg, params, xi, xv, dfwfm_oracle.forward(cfg, params, xi, xv), forward(cfg, params, xi, xv)


def conditions(g, e, r):
    """The three figures the GPU tests bound, errors scaled by max(1, |r|): the share of rows with |g - e| <= 1e-5,
    the worst |g - e| over max(1e-5, fmt), the worst |g - r| over fmt -- fmt = max |e - r| is the format's own error,
    from the references alone."""
    g, e, r = (np.asarray(a, dtype=np.float64) for a in (g, e, r))
    s = np.maximum(1.0, np.abs(r))
    fmt = float((np.abs(e - r) / s).max())
    d = np.abs(g - e) / s
    return dict(fmt=fmt, close=float((d <= 1e-5).mean()), worst_ge=float(d.max()),
                worst_gr=float((np.abs(g - r) / s).max()))


def assert_conditions(g, e, r, what):
    c = conditions(g, e, r)
    print(what, c)
    assert np.isfinite(np.asarray(g)).all(), what
    assert c["close"] >= 0.90, (what, c)
    assert c["worst_ge"] <= max(1e-5, c["fmt"]), (what, c)
    assert c["worst_gr"] <= 2 * c["fmt"], (what, c)
    return c


@functools.lru_cache(maxsize=None)
def exact_case(rows=96, seed=5):
    """(cfg, params, xi, xv): Criteo-39 shaped (F = 39, 13 numerical, D = 10, N = 400, H = 3, lw) with small-integer
    tables and Xv, field_cov in multiples of 0.5, a handful of nonzeros from {+-1, +-0.5} per hidden row (layer 3:
    +-1 only) placed to cover the first and last K index and every 32-wide K chunk, small-integer biases and fc in
    {0, +-0.5, +-1}: every rounded activation is exactly representable in bf16 and every partial sum in float32, so
    the float64 oracle, the contract and any kernel honouring it give the same float32 logits bit for bit."""
    from xsdeepfwfm_deprecated_amd import DeepFMs
    F, num, D, N, H = 39, 13, 10, 400, 3
    sizes = [1] * num + [int(x) for x in 50 + (np.arange(F - num) * 37) % 400]
    cfg = dict(field_size=F, feature_sizes=sizes, embedding_size=D, use_fwfm=1, use_fm=0, use_logit=0,
               use_deep=1, use_lw=1, use_fwlw=0, h_depth=H, deep_nodes=N, numerical=num,
               embedding_bag=0, qr_flag=0, qr_operation="mult", qr_collisions=4, qr_threshold=200)
    shapes = {k: tuple(v.shape) for k, v in DeepFMs(**model_kwargs(cfg)).state_dict().items()}
    rs = np.random.RandomState(seed)
    params = {}
    for k, shp in shapes.items():
        if k.startswith("fm_2nd_embeddings") or k.startswith("fm_1st_embeddings"):
            v = rs.randint(-1, 2, size=shp)
            if shp[0] == 1:  # a numerical field's single row: never all zero
                v[v == 0] = 1
            params[k] = v.astype(np.float32)
        elif k == "field_cov.weight":
            r = rs.choice([0.0, 0.0, 0.0, 0.5, -0.5, 1.0, -1.0], size=shp)
            params[k] = (np.triu(r, 1) + np.triu(r, 1).T).astype(np.float32)  # symmetric: (R + R^T) / 2 exact
        elif k == "fm_1st.weight":
            params[k] = rs.choice([0.5, -0.5, 1.0, -1.0], size=shp).astype(np.float32)
        elif k == "bias":
            params[k] = np.full(shp, 2.0, dtype=np.float32)
        elif k == "net_1_fc.weight":
            params[k] = rs.choice([0.0, 0.5, -0.5, 1.0, -1.0], size=shp).astype(np.float32)
        elif k.startswith("net_1_linear_") and k.endswith(".bias"):
            params[k] = rs.randint(-1, 3, size=shp).astype(np.float32)
        elif k.startswith("net_1_linear_") and k.endswith(".weight"):
            n, K = shp
            vals = [1.0, -1.0] if k == "net_1_linear_3.weight" else [1.0, -1.0, 0.5, -0.5]
            nch = -(-K // 32)
            w = np.zeros(shp, dtype=np.float32)
            for i in range(n):
                c = i % nch  # one nonzero in K chunk i mod nch: every 32-wide chunk is covered many times
                pos = [rs.randint(32 * c, min(K, 32 * c + 32))] + list(rs.randint(0, K, size=3))
                if i % 7 == 0:
                    pos.append(0)
                if i % 7 == 1:
                    pos.append(K - 1)
                for p in set(int(q) for q in pos):
                    w[i, p] = rs.choice(vals)
            params[k] = w
        else:
            raise KeyError(k)
    xi = np.stack([rs.randint(0, s, size=rows) for s in sizes[num:]], axis=1).astype(np.int64)
    xv = rs.randint(0, 3, size=(rows, num)).astype(np.float32)
    # the construction's promise, checked on these very inputs: no rounding point of the contract changes a value
    _, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    h = parts["E"].reshape(rows, -1)
    assert np.array_equal(bf16_rne(h.astype(np.float32)).astype(np.float64), h)
    for l in range(1, H + 1):
        W = params[f"net_1_linear_{l}.weight"]
        assert np.array_equal(bf16_rne(W), W)
        h = np.maximum(h @ W.T.astype(np.float64) + params[f"net_1_linear_{l}.bias"].astype(np.float64), 0.0)
        # multiples of 2^-3 below 2^10: any partial sum of such terms is exact in float32's 24 bits
        assert np.array_equal(h * 8, np.round(h * 8)) and np.abs(h).max() < 1024
        if l < H:
            assert np.array_equal(bf16_rne(h.astype(np.float32)).astype(np.float64), h), f"layer {l} not bf16-exact"
    return cfg, params, xi, xv
