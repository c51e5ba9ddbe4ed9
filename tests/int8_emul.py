"""Helper (no tests): the numeric contract of the int8 deep tower (include/dfwfm_int8.h) in numpy, the cases the int8
tests share, and a Criteo-39-shaped case on which every quantization of the contract is exact."""
import functools

import numpy as np

import bf16_emul
from bf16_emul import DEEP_GOLDENS, SWEEP, SWEEP_ROWS, conditions, sweep_case  # noqa: F401 (shared with the tests)
from conftest import model_kwargs
from oracle import dfwfm_oracle

f32 = np.float32
# the sweep shapes the int8 forward runs (embedding_size 10, field_size <= 48) and those it refuses
SWEEP_SUPPORTED = [i for i, s in enumerate(SWEEP) if s[2] == 10 and s[0] <= 48]
SWEEP_UNSUPPORTED = [i for i in range(len(SWEEP)) if i not in SWEEP_SUPPORTED]


def quantize_weights(W):
    """(qW float64 array of integers in [-127, 127], sw float32 [N]) of a layer's f32 weights [N, K]: per neuron
    aw = max |W| (NaN kept), sw = aw / 127 (1 for a zero row), qW = clamp(rint(W / sw)) -- f32 division, ties to even
    --, 0 where W / sw is NaN.  A row that holds a NaN has sw = NaN, one that holds an infinity sw = inf; both have
    qW = 0."""
    W = np.asarray(W, dtype=f32)
    with np.errstate(all="ignore"):
        aw = np.abs(W).max(axis=1).astype(f32)  # np.max propagates NaN
        sw = np.where(aw == 0, f32(1), aw / f32(127)).astype(f32)
        q = np.rint((W / sw[:, None]).astype(f32))
        q = np.where(np.isnan(q), f32(0), q)
    return np.clip(q, -127, 127).astype(np.float64), sw


def quantize_rows(x):
    """(q float64 array of integers, sx float32 [B], inv float32 [B]) of f32 rows [B, K]: a = max |x| (NaN kept),
    inv = 127 / a and sx = a / 127 (both 0 for a zero row), q = clamp(rint(x inv)), 0 where x inv is NaN."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(all="ignore"):
        a = np.abs(x).max(axis=1).astype(f32)  # np.max propagates NaN
        zero = a == 0
        safe = np.where(zero, f32(1), a)
        inv = np.where(zero, f32(0), f32(127) / safe).astype(f32)
        sx = np.where(zero, f32(0), safe / f32(127)).astype(f32)
        r = np.rint((x * inv[:, None]).astype(f32))
        r = np.where(np.isnan(r), f32(0), r)
    return np.clip(r, -127, 127).astype(np.float64), sx, inv


def tower(cfg, params, x, fma=True, return_hidden=False):
    """h_H (float32 [B, N]) of the contract from the f32 tower input x [B, K]; rows and weights may hold NaN or inf.
    fma: the epilogue as one fused multiply-add (a float64 product -- exact for a 24-bit by 24-bit value -- plus add,
    rounded once to f32); False: a f32 multiply, then a f32 add (the other rounding a kernel might use)."""
    H = cfg["h_depth"]
    hidden = []
    h = None
    for l in range(1, H + 1):
        qW, sw = quantize_weights(params[f"net_1_linear_{l}.weight"])
        b = np.asarray(params[f"net_1_linear_{l}.bias"], dtype=f32)
        q, sx, _ = quantize_rows(x)
        acc = q @ qW.T  # integers below 2^24: exact in float64 in any order
        # q and qW are finite whatever x and W hold (a NaN quotient is 0): what is not finite enters through sx, sw, b
        assert np.abs(acc).max(initial=0) < 2 ** 24  # (false for a NaN too)
        with np.errstate(all="ignore"):
            t = (sx[:, None] * sw[None, :]).astype(f32)
            if fma:
                z = (acc * t.astype(np.float64) + b.astype(np.float64)).astype(f32)
            else:
                z = ((acc.astype(f32) * t).astype(f32) + b).astype(f32)
            h = np.maximum(z, f32(0))  # np.maximum keeps NaN, as relu_keep_nan
        hidden.append(h)
        x = h
    return (h, hidden) if return_hidden else h


def forward(cfg, params, xi, xv, fma=True):
    """Logits (float64 array) of the contract: E and the shallow terms from the float64 oracle, the tower with the
    contract's f32 steps, deep in float64."""
    _, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    B = np.asarray(xi).shape[0]
    shallow = parts["first"] + parts["second"]
    with np.errstate(all="ignore"):
        x = parts["E"].astype(f32).reshape(B, -1)
        h = tower(cfg, params, x, fma=fma)
        fc = np.asarray(params["net_1_fc.weight"], dtype=f32)[0].astype(np.float64)
        deep = h.astype(np.float64) @ fc
    bias = float(np.asarray(params["bias"], dtype=np.float64)[0]) if "bias" in params else 0.0
    return (shallow + deep) + bias


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """(cfg, params, xi, xv, y, ref64, emul64) of a deep golden's first 256 rows (tiny_deepfwfm_lw: all 2000), the
    int8 emulation in place of the bf16 one; computed once, shared, never modified."""
    cfg, params, xi, xv, y, r, _ = bf16_emul.golden_case(name)
    return cfg, params, xi, xv, y, r, forward(cfg, params, xi, xv)


@functools.lru_cache(maxsize=None)
def sweep_ref(i):
    """(cfg, params, xi, xv, ref64, emul64) of SWEEP[i]; computed once, shared, never modified."""
    cfg, params, xi, xv, r, _ = bf16_emul.sweep_ref(i)
    return cfg, params, xi, xv, r, forward(cfg, params, xi, xv)


def assert_conditions(g, e, r, what):
    """The acceptance conditions of kernel g against emulation e and float64 reference r (errors over max(1, |r|),
    fmt = max |e - r| the format's own error): at least 0.99 of the rows within 1e-5 of e -- the kernel's only freedom
    against e is f32 rounding in the epilogue and the order of deep's sum --, the worst |g - e| <= max(1e-5, fmt), the
    worst |g - r| <= 2 fmt."""
    c = conditions(g, e, r)
    print(what, c)
    assert np.isfinite(np.asarray(g)).all(), what
    assert c["close"] >= 0.99, (what, c)
    assert c["worst_ge"] <= max(1e-5, c["fmt"]), (what, c)
    assert c["worst_gr"] <= 2 * c["fmt"], (what, c)
    return c


@functools.lru_cache(maxsize=None)
def exact_case(rows=96, seed=11):
    """(cfg, params, xi, xv): Criteo-39 shaped (F = 39, 13 numerical, D = 10, N = 400, H = 2, lw) on which every
    quantization of the contract is exact, so the float64 oracle, the contract and any kernel honouring it give the
    same float32 logits bit for bit.

    Numerical field 0 is a pilot: its table row is [127, 0, ...] and its Xv is 1, so every E row's max is exactly 127
    (inv = sx = 1) and E column 1 is always 0.  The other tables and Xv hold small integers.  Hidden weights are
    multiples of 1/4 up to 3/4, plus one entry of +-127/128 per neuron on the layer's always-zero input column 1, so
    sw = 2^-7 exactly and qW = 128 W.  Neuron 0 of layer 1 is a pilot (no useful weight, bias 31.75): every hidden
    row's max is 127/4, inv = 4, sx = 1/4; neuron 1 is dead (bias 0), layer 2's always-zero column.  The pilot column 0
    carries weight -1/4 for every seventh neuron (the first real k), column K - 1 for the next; every 64-wide K step
    is covered many times."""
    from xsdeepfwfm_deprecated_amd import DeepFMs
    F, num, D, N, H = 39, 13, 10, 400, 2
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
            params[k] = v.astype(f32)
        elif k == "field_cov.weight":
            r = rs.choice([0.0, 0.0, 0.0, 0.5, -0.5, 1.0, -1.0], size=shp)
            params[k] = (np.triu(r, 1) + np.triu(r, 1).T).astype(f32)  # symmetric: (R + R^T) / 2 exact
        elif k == "fm_1st.weight":
            params[k] = rs.choice([0.5, -0.5, 1.0, -1.0], size=shp).astype(f32)
        elif k == "bias":
            params[k] = np.full(shp, 2.0, dtype=f32)
        elif k == "net_1_fc.weight":
            params[k] = rs.choice([0.0, 0.5, -0.5, 1.0, -1.0], size=shp).astype(f32)
        elif k.startswith("net_1_linear_") and k.endswith(".bias"):
            params[k] = (rs.randint(-4, 9, size=shp) / 4.0).astype(f32)
        elif k.startswith("net_1_linear_") and k.endswith(".weight"):
            n, K = shp
            nch = -(-K // 64)
            w = np.zeros(shp, dtype=f32)
            for i in range(n):
                w[i, 1] = rs.choice([127.0 / 128.0, -127.0 / 128.0])  # on the always-zero column: sw = 2^-7
                if i < 2:  # the pilot and the dead neuron
                    continue
                c = i % nch  # one nonzero in K step i mod nch: every 64-wide step is covered many times
                pos = [rs.randint(max(2, 64 * c), min(K, 64 * c + 64))] + list(rs.randint(2, K, size=3))
                if i % 7 == 1:
                    pos.append(K - 1)
                for p in set(int(q) for q in pos):
                    w[i, p] = rs.choice([0.25, -0.25, 0.5, -0.5, 0.75, -0.75])
                if i % 7 == 0:
                    w[i, 0] = -0.25  # the pilot column, the first real k
            params[k] = w
        else:
            raise KeyError(k)
    params["fm_2nd_embeddings.0.weight"] = np.array([[127.0] + [0.0] * (D - 1)], dtype=f32)
    for l in (1, 2):  # the neurons reading the pilot column get its product back in their bias, and stay visible
        b = params[f"net_1_linear_{l}.bias"]
        W = params[f"net_1_linear_{l}.weight"]
        b[W[:, 0] != 0] = 33.75 if l == 1 else 8.0
    params["net_1_linear_1.bias"][0] = 31.75
    params["net_1_linear_1.bias"][1] = 0.0
    xi = np.stack([rs.randint(0, s, size=rows) for s in sizes[num:]], axis=1).astype(np.int64)
    xv = rs.randint(0, 3, size=(rows, num)).astype(f32)
    xv[:, 0] = 1.0
    # the construction's promise, checked on these very inputs
    _, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    E = parts["E"].reshape(rows, -1)
    assert np.array_equal(E, np.round(E)) and (np.abs(E).max(axis=1) == 127).all() and (E[:, 1] == 0).all()
    for l in (1, 2):
        qW, sw = quantize_weights(params[f"net_1_linear_{l}.weight"])
        assert (sw == f32(2.0 ** -7)).all()
        assert np.array_equal(qW, params[f"net_1_linear_{l}.weight"].astype(np.float64) * 128)
    h1 = np.maximum(E @ params["net_1_linear_1.weight"].T.astype(np.float64)
                    + params["net_1_linear_1.bias"].astype(np.float64), 0.0)
    assert h1.max() <= 31.75 and (h1[:, 0] == 31.75).all() and (h1[:, 1] == 0).all()
    assert np.array_equal(h1 * 4, np.round(h1 * 4))
    assert (h1[:, params["net_1_linear_1.weight"][:, 0] != 0] > 0).any()  # the first real k shows in a live neuron
    q, sx, inv = quantize_rows(h1.astype(f32))
    assert (inv == 4).all() and (sx == 0.25).all() and np.array_equal(q, h1 * 4)
    return cfg, params, xi, xv
