"""A CPU reference of the list-driven row-wise Adagrad step (include_dp/dfwfm_rowwise_lists.h), shared by
tests/test_rowwise_lists_boundary.py (CPU), tests/test_gpu_rowwise_lists.py and tests/test_gpu_rowwise_exchange.py.

The step is two things joined, and so is this reference: the union of the lists' destinations mapped to rows per span
(lazy_lists_ref.union_rows, written out in numpy independently of the kernel), and the row's arithmetic on those rows
(rowwise_adagrad_ref.lib_rows: dfwfm_rowwise_adagrad_row_ref, THE contract; or np_rows: the header's five lines in
numpy).  A span is (offset, rows, width) -- the offset indexes the flat gradient only; parameters and accumulators are
one array per span --, a list is (dest int64 array, count, cap, width)."""
import numpy as np

import lazy_lists_ref
import rowwise_adagrad_ref as rw

f32 = np.float32
union_rows = lazy_lists_ref.union_rows


def layout(shapes):
    """Spans (offset, rows, width) at 4-float-padded offsets, and the flat gradient's length."""
    spans, off = [], 0
    for rows, width in shapes:
        spans.append((off, rows, width))
        off += (rows * width + 3) & ~3
    return spans, off


def grad_rows(grad, span):
    """The span's [rows, width] view of the flat gradient."""
    off, rows, width = span
    return grad[off:off + rows * width].reshape(rows, width)


def rowwise_lists_ref(params, grad, accs, spans, lists, *, lr, weight_decay=0.0, eps=1e-10, elem="np",
                      ss_of=rw.chain_ss):
    """(params, grad, accs, union) after one list-driven row-wise step: params a list of [rows, width] arrays and accs a
    list of [rows] arrays, one per span, grad the flat float32 array, union the touched rows per span.  The inputs are
    not written.  Untouched rows, untouched accumulators and everything of grad outside the touched rows are copies;
    touched gradient rows are zero.  elem: 'np' (np_rows, with `ss_of` the chain or, to witness the order, a tree) or
    'lib' (dfwfm_rowwise_adagrad_row_ref, one call per row)."""
    params = [np.array(p, f32, copy=True) for p in params]
    accs = [np.array(a, f32, copy=True) for a in accs]
    grad = np.array(grad, f32, copy=True)
    union = union_rows(spans, lists)
    for i, (span, rows) in enumerate(zip(spans, union)):
        assert params[i].shape == (span[1], span[2]) and accs[i].shape == (span[1],)
        if not len(rows):
            continue
        g = grad_rows(grad, span)
        if elem == "lib":
            pc, ac = rw.lib_rows(rw.hyper(lr, weight_decay, eps), params[i][rows], g[rows], accs[i][rows])
        else:
            pc, ac = rw.np_rows(params[i][rows], g[rows], accs[i][rows], lr=lr, wd=weight_decay, eps=eps, ss_of=ss_of)
        params[i][rows], accs[i][rows] = pc, ac
        g[rows] = 0.0
    return params, grad, accs, union


def keys_for(union):
    """Keys [batch, n] (int64) for the n spans whose union is not empty, and those spans' indices: column j's keys
    touch exactly union[index[j]] on a plain table (short unions are padded by repeating their first row)."""
    index = [i for i, u in enumerate(union) if len(u)]
    batch = max((len(union[i]) for i in index), default=0)
    keys = np.zeros((batch, max(len(index), 1)), np.int64)
    for j, i in enumerate(index):
        keys[:, j] = union[i][0]
        keys[:len(union[i]), j] = union[i]
    return keys, index
