"""A CPU reference of the row-lazy Adam step (include/dfwfm_lazy_adam.h): the touched rows of a table are gathered
into compact tensors, torch.optim.Adam(foreach=False) -- the reference's optimizer -- runs on them with its state's
`step` preset to the GLOBAL step, and the rows are scattered back.  The key mapping and the clamp are written out in
numpy, independently of the kernel."""
import numpy as np
import torch

PLAIN, QUOTIENT, REMAINDER = 0, 1, 2


def touched_rows(keys, key_range, kind=PLAIN, c=1):
    """Sorted distinct rows the keys map to: a key outside [0, key_range) counts as key 0; the row is the key (plain),
    key // c (QR quotient table) or key % c (QR remainder table)."""
    k = np.asarray(keys, dtype=np.int64).copy()
    k[(k < 0) | (k >= key_range)] = 0
    if kind == QUOTIENT:
        k = k // c
    elif kind == REMAINDER:
        k = k % c
    elif kind != PLAIN:
        raise ValueError(kind)
    return np.unique(k)


def lazy_adam_ref(p, g, m, v, keys, key_range, step, kind=PLAIN, c=1, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                  weight_decay=0.0):
    """(param, grad, exp_avg, exp_avg_sq) [rows, width] float32 numpy after the lazy step number `step` (>= 1) for
    `keys`; the inputs are not written.  Untouched rows are copies; touched rows' gradients are zero."""
    p, g, m, v = (np.array(a, dtype=np.float32, copy=True) for a in (p, g, m, v))
    rows = touched_rows(keys, key_range, kind, c)
    assert rows.size == 0 or rows.max() < p.shape[0]
    if rows.size == 0:
        return p, g, m, v
    q = torch.from_numpy(p[rows].copy()).requires_grad_(True)
    q.grad = torch.from_numpy(g[rows].copy())
    opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m[rows].copy()),
                    "exp_avg_sq": torch.from_numpy(v[rows].copy())}
    opt.step()
    st = opt.state[q]
    assert float(st["step"]) == float(step)
    p[rows] = q.detach().numpy()
    m[rows] = st["exp_avg"].numpy()
    v[rows] = st["exp_avg_sq"].numpy()
    g[rows] = 0.0
    return p, g, m, v
