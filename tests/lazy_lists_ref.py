"""A CPU reference of the list-driven row-lazy steps (include/dfwfm_lazy_lists.h): the union of the lists' destinations
is mapped to rows per span -- written out in numpy, independently of the kernel -- and the key-driven references
(lazy_adam_ref.lazy_adam_ref, lazy_optim_ref.lazy_optim_ref) run on those rows of each span's slice of the flat
buffers.  A span is (offset, rows, width); a list is (dest int64 array, count, cap, width)."""
import numpy as np

import lazy_adam_ref
import lazy_optim_ref


def union_rows(spans, lists):
    """Per span the sorted distinct rows the lists name: the first min(max(count, 0), cap) destinations of every list
    of the span's width that are a row's first element inside the span; every other destination is skipped."""
    out = []
    for off, rows, width in spans:
        hit = []
        for dest, count, cap, w in lists:
            if w != width:
                continue
            d = np.asarray(dest, np.int64)[:min(max(int(count), 0), int(cap))]
            d = d[(d >= off) & (d < off + rows * width)]
            d = d[(d - off) % width == 0]
            hit.append((d - off) // width)
        out.append(np.unique(np.concatenate(hit)) if hit else np.zeros(0, np.int64))
    return out


def _slice(flat, off, rows, width):
    return None if flat is None else flat[off:off + rows * width].reshape(rows, width)


def lazy_adam_lists_ref(params, grad, exp_avg, exp_avg_sq, spans, lists, step, **kw):
    """(params, grad, exp_avg, exp_avg_sq) after the lists step number `step` (>= 1, the global step): params a list of
    [rows, width] arrays, one per span, the others flat float32 arrays.  The inputs are not written."""
    params = [np.array(p, np.float32, copy=True) for p in params]
    grad, m, v = (np.array(a, np.float32, copy=True) for a in (grad, exp_avg, exp_avg_sq))
    for i, ((off, rows, width), touched) in enumerate(zip(spans, union_rows(spans, lists))):
        p, g, mm, vv = lazy_adam_ref.lazy_adam_ref(params[i], _slice(grad, off, rows, width),
                                                   _slice(m, off, rows, width), _slice(v, off, rows, width), touched,
                                                   rows, step, **kw)
        params[i] = p
        for flat, new in ((grad, g), (m, mm), (v, vv)):
            flat[off:off + rows * width] = new.reshape(-1)
    return params, grad, m, v


def lazy_optim_lists_ref(opt, params, grad, state, spans, lists, step, **kw):
    """(params, grad, state) after the lists step number `step` of optimizer `opt` ('sgd' / 'adag' / 'rmsp'); `state`
    None (and returned None) for plain SGD."""
    params = [np.array(p, np.float32, copy=True) for p in params]
    grad = np.array(grad, np.float32, copy=True)
    state = None if state is None else np.array(state, np.float32, copy=True)
    for i, ((off, rows, width), touched) in enumerate(zip(spans, union_rows(spans, lists))):
        p, g, s = lazy_optim_ref.lazy_optim_ref(opt, params[i], _slice(grad, off, rows, width),
                                                _slice(state, off, rows, width), touched, rows, step, **kw)
        params[i] = p
        grad[off:off + rows * width] = g.reshape(-1)
        if s is not None:
            state[off:off + rows * width] = s.reshape(-1)
    return params, grad, state
