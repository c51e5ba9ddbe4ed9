"""The yardstick of the fp16 serving copy (include/dfwfm_half_tables.h, DeepFMs.table_dtype = "fp16"): a model whose
categorical second-order tables went through IEEE fp16 once -- round to nearest even, subnormals kept, which is what
numpy's float16 cast and torch's .half() do -- and nothing else.  The fp16 forward of the original model must give that
model's f32-copy logits bit for bit.  A helper: no tests here."""
import copy

import numpy as np


def categorical_second_order_keys(cfg, params):
    """The state-dict names of the tables the copy rounds: second order, fields numerical .. field_size - 1."""
    keys = []
    for f in range(cfg["numerical"], cfg["field_size"]):
        keys += [k for k in params if k.startswith(f"fm_2nd_embeddings.{f}.")]
    return keys


def rounded_params(cfg, params):
    """A copy of `params` with only the categorical second-order tables passed through np.float16 and back."""
    out = {k: np.array(v, copy=True) for k, v in params.items()}
    with np.errstate(over="ignore"):
        for k in categorical_second_order_keys(cfg, params):
            out[k] = np.asarray(params[k], dtype=np.float32).astype(np.float16).astype(np.float32)
    return out


def rounded_model(m):
    """A copy of the module (same device and mode, its own engine) with the same tables rounded: w.half().float()."""
    import torch
    held = {k: m.__dict__.pop(k) for k in ("_engine", "_dev_metrics") if k in m.__dict__}
    try:
        m.__dict__["_engine"] = None
        r = copy.deepcopy(m)
    finally:
        m.__dict__.update(held)
    with torch.no_grad():
        for f in range(m.num, m.field_size):
            for p in r.fm_2nd_embeddings[f].parameters():
                p.copy_(p.half().float())
    return r
