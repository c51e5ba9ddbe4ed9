"""A CPU reference of the row-lazy SGD / Adagrad / RMSprop step (include/dfwfm_lazy_optim.h): the touched rows of a
table (lazy_adam_ref.touched_rows: the key mapping and the clamp, written out in numpy) are gathered into compact
arrays, the dense step's per-element arithmetic at the GLOBAL step -- optim_ref.np_step, the numpy restatement of
include/dfwfm_optim.h, or optim_ref.lib_step, the library's host function dfwfm_optim_elem_ref -- runs on them, and the
rows are scattered back with their gradient zeroed.  Independent of the kernel."""
import numpy as np

import optim_ref
from lazy_adam_ref import PLAIN, QUOTIENT, REMAINDER, touched_rows  # noqa: F401  (re-exported)


def lazy_optim_ref(opt, p, g, s, keys, key_range, step, kind=PLAIN, c=1, lr=1e-3, weight_decay=0.0, momentum=0.0,
                   alpha=optim_ref.DEFAULT_ALPHA, eps=None, elem="np"):
    """(param, grad, state) [rows, width] float32 numpy after the lazy step number `step` (>= 1, the global step) of
    optimizer `opt` ('sgd' / 'adag' / 'rmsp') for `keys`; the inputs are not written.  `s` None (and returned None)
    for plain SGD.  Untouched rows are copies; touched rows' gradients are zero.  elem: 'np' (optim_ref.np_step) or
    'lib' (dfwfm_optim_elem_ref, one call per element)."""
    p, g = (np.array(a, dtype=np.float32, copy=True) for a in (p, g))
    has = optim_ref.has_state(opt, momentum)
    s = np.array(s, dtype=np.float32, copy=True) if has else None
    rows = touched_rows(keys, key_range, kind, c)
    assert rows.size == 0 or rows.max() < p.shape[0]
    if rows.size == 0:
        return p, g, s
    sc = s[rows] if has else None
    if elem == "lib":
        h = optim_ref.hyper(opt, lr, weight_decay, momentum, alpha, eps)
        pc, sc = optim_ref.lib_step(h, step, p[rows], g[rows], sc)
    else:
        pc, sc = optim_ref.np_step(opt, step, p[rows], g[rows], sc, lr=lr, wd=weight_decay, momentum=momentum,
                                   alpha=alpha, eps=eps)
    p[rows] = pc
    if has:
        s[rows] = sc
    g[rows] = 0.0
    return p, g, s
