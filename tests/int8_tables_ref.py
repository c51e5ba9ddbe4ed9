"""The yardstick of the int8 serving copy (include/dfwfm_int8_tables.h, DeepFMs.table_dtype = "int8"): a model whose
categorical second-order tables went through the header's row-wise quantizer once -- written out here in numpy float32,
step by step as the header states it -- and nothing else.  The int8 forward of the original model must give that
model's f32-copy logits bit for bit.  A helper: no tests here."""
import copy

import numpy as np

TWO_M126 = np.float32(2.0 ** -126)  # the smallest normal f32


def categorical_second_order_keys(cfg, params):
    """The state-dict names of the tables the copy quantizes: second order, fields numerical .. field_size - 1."""
    keys = []
    for f in range(cfg["numerical"], cfg["field_size"]):
        keys += [k for k in params if k.startswith(f"fm_2nd_embeddings.{f}.")]
    return keys


def quantize_rows(w):
    """(q int8 [n, D], s float32 [n]) of the rows of w [n, D], all in IEEE float32:
    amax = max |w|, t = amax / 127, s = t rounded up to bf16 (0 when t < 2^-126), q = clamp(rint(w / s), -127, 127)
    with rint to nearest even and q = 0 when s = 0."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    assert w.ndim == 2
    with np.errstate(all="ignore"):
        amax = np.max(np.abs(w), axis=1).astype(np.float32)
        t = (amax / np.float32(127.0)).astype(np.float32)
        bits = t.view(np.uint32).astype(np.uint64)
        s = (((bits + 0xFFFF) & 0xFFFF0000) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
        s = np.where(t < TWO_M126, np.float32(0.0), s).astype(np.float32)
        safe = np.where(s == 0, np.float32(1.0), s)[:, None]
        r = np.rint((w / safe).astype(np.float32))  # numpy's rint: to nearest, ties to even
        r = np.where(s[:, None] == 0, np.float32(0.0), r)
        q = np.clip(np.nan_to_num(r, nan=0.0), -127.0, 127.0).astype(np.int8)
    return q, s


def dequantized(w):
    """The values the copy serves for the rows of w: float(q) * s, a product that is exact in float32."""
    q, s = quantize_rows(w)
    with np.errstate(all="ignore"):
        return (q.astype(np.float32) * s[:, None]).astype(np.float32)


def quantized_params(cfg, params):
    """A copy of `params` with only the categorical second-order tables replaced by their dequantized values."""
    out = {k: np.array(v, copy=True) for k, v in params.items()}
    for k in categorical_second_order_keys(cfg, params):
        v = np.asarray(params[k], dtype=np.float32)
        out[k] = dequantized(v.reshape(-1, v.shape[-1])).reshape(v.shape)
    return out


def quantized_model(m):
    """A copy of the module (same device and mode, its own engine) with the same tables dequantized, reading the f32
    copy: the quantizer is not idempotent (a second pass would round the scale up again)."""
    import torch
    held = {k: m.__dict__.pop(k) for k in ("_engine", "_dev_metrics") if k in m.__dict__}
    try:
        m.__dict__["_engine"] = None
        r = copy.deepcopy(m)
    finally:
        m.__dict__.update(held)
    r.table_dtype = "f32"
    with torch.no_grad():
        for f in range(m.num, m.field_size):
            for p in r.fm_2nd_embeddings[f].parameters():
                v = p.detach().cpu().numpy()
                p.copy_(torch.from_numpy(dequantized(v.reshape(-1, v.shape[-1])).reshape(v.shape)).to(p.device))
    return r
