"""Helper (no tests): the numeric contract of the folded layer 1 of the one-launch bf16 forward
(include/dfwfm_bf16_fold.h) in numpy, on bf16_emul and the oracle's parts["E"]; the folded references of the goldens,
computed once and shared; and the exact case, checked here on its own inputs."""
import functools

import numpy as np

import bf16_emul
from bf16_emul import bf16_rne
from oracle import dfwfm_oracle


def folded_p(cfg, params):
    """bf16(P) [N, num] as float32: P[f][n] = sum_d W1[n, f D + d] v_f[0][d] from the f32 parameters, accumulated in
    float64 over d ascending, rounded to float32, then to bf16."""
    num, D = cfg["numerical"], cfg["embedding_size"]
    W1 = np.asarray(params["net_1_linear_1.weight"], dtype=np.float32)
    P = np.zeros((W1.shape[0], num), dtype=np.float64)
    for f in range(num):
        v = np.asarray(params[f"fm_2nd_embeddings.{f}.weight"], dtype=np.float32)[0]
        for d in range(D):  # the contract's order
            P[:, f] = P[:, f] + W1[:, f * D + d].astype(np.float64) * np.float64(v[d])
    return bf16_rne(P.astype(np.float32))


def forward(cfg, params, xi, xv, acc=np.float64):
    """Logits (float64 array) of the folded contract: bf16_emul.forward with layer 1 over the K rows (categorical
    columns of E and bf16(W1) | Xv and bf16(P)).  A model without a numerical field never folds: the unfolded
    contract."""
    F, num, D = cfg["field_size"], cfg["numerical"], cfg["embedding_size"]
    if num == 0:
        return bf16_emul.forward(cfg, params, xi, xv, acc=acc)
    _, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    B = np.asarray(xi).shape[0]
    shallow = parts["first"] + parts["second"]
    W1 = np.asarray(params["net_1_linear_1.weight"], dtype=np.float32)
    xk = np.concatenate([bf16_rne(parts["E"][:, num:, :].astype(np.float32).reshape(B, (F - num) * D)),
                         bf16_rne(np.asarray(xv, dtype=np.float32)[:, :num])], axis=1)
    wk = np.concatenate([bf16_rne(W1[:, num * D:]), folded_p(cfg, params)], axis=1)
    H = cfg["h_depth"]
    h = None
    for l in range(1, H + 1):
        if l == 1:
            x, wb = xk, wk
        else:
            wb = bf16_rne(np.asarray(params[f"net_1_linear_{l}.weight"], dtype=np.float32))
        bias = np.asarray(params[f"net_1_linear_{l}.bias"], dtype=np.float32).astype(acc)
        h = np.maximum(x.astype(acc) @ wb.T.astype(acc) + bias, acc(0))  # np.maximum keeps NaN, as relu_keep_nan
        if l < H:
            x = bf16_rne(h.astype(np.float32))
    fc = np.asarray(params["net_1_fc.weight"], dtype=np.float32)[0].astype(acc)
    deep = (h @ fc).astype(np.float64)
    bias = float(np.asarray(params["bias"], dtype=np.float64)[0]) if "bias" in params else 0.0
    return (shallow + deep) + bias


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """(cfg, params, xi, xv, y, ref64, folded emul64) of bf16_emul.golden_case(name); shared, never modified."""
    cfg, params, xi, xv, y, r, _ = bf16_emul.golden_case(name)
    return cfg, params, xi, xv, y, r, forward(cfg, params, xi, xv)


@functools.lru_cache(maxsize=None)
def exact_case():
    """bf16_emul.exact_case() with its float32 oracle logits.  The promise the GPU test rests on, checked on these
    very inputs: P is exact in bf16 (a few terms from {+-1, +-0.5} times small integers), so the folded contract
    equals the float64 oracle bit for bit, as the unfolded one does."""
    cfg, params, xi, xv = bf16_emul.exact_case()
    ref = dfwfm_oracle.forward(cfg, params, xi, xv)
    num, D = cfg["numerical"], cfg["embedding_size"]
    W1 = params["net_1_linear_1.weight"].astype(np.float64)
    v0 = np.stack([params[f"fm_2nd_embeddings.{f}.weight"][0] for f in range(num)]).astype(np.float64)
    P = np.einsum("nfd,fd->nf", W1[:, :num * D].reshape(-1, num, D), v0)
    assert np.array_equal(folded_p(cfg, params).astype(np.float64), P) and np.abs(P).max() > 0
    assert np.array_equal(forward(cfg, params, xi, xv), ref)
    assert np.array_equal(bf16_emul.forward(cfg, params, xi, xv), ref)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    return cfg, params, xi, xv, ref.astype(np.float32)
