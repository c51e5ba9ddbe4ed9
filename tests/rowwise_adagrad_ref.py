"""A CPU reference of the row-wise Adagrad step (include/dfwfm_rowwise_adagrad.h), shared by
tests/test_rowwise_adagrad_boundary.py (CPU) and tests/test_gpu_rowwise_adagrad.py (GPU).

Two statements of the same arithmetic:
  * np_rows: the header's five lines in numpy float32, written here independently of the C function.  The chain
    ss = fmaf(g'_e, g'_e, ss) runs element by element through optim_ref.fma32 (one rounding of the exact product plus
    sum), vectorised over rows; numpy's float32 division and square root are the correctly rounded ones.
  * lib_rows: ctypes access to dfwfm_rowwise_adagrad_row_ref, the library's host function -- THE contract the GPU
    tests check the kernel against, one row per call.
rowwise_ref applies either to the touched rows of a table (lazy_optim_ref.touched_rows: the key mapping and the clamp)
and zeroes their gradient rows.  tree_ss is the sum of squares by a pairwise tree: what the contract's chain is NOT.
"""
import ctypes

import numpy as np

import optim_ref
from lazy_optim_ref import PLAIN, QUOTIENT, REMAINDER, touched_rows  # noqa: F401  (re-exported)

f32 = np.float32


def hyper(lr, wd=0.0, eps=1e-10, kind="adag"):
    return optim_ref.hyper(kind, lr, wd, eps=eps)


def chain_ss(gp):
    """ss [n] of g' [n, width]: the sequential chain in element order."""
    gp = np.asarray(gp, f32)
    ss = np.zeros(gp.shape[0], f32)
    for e in range(gp.shape[1]):
        ss = optim_ref.fma32(gp[:, e], gp[:, e], ss)
    return ss


def tree_ss(gp):
    """The same sum by a pairwise tree of rounded squares and rounded sums (adjacent pairs, an odd one carried up)."""
    gp = np.asarray(gp, f32)
    level = [(gp[:, e] * gp[:, e]).astype(f32) for e in range(gp.shape[1])]
    while len(level) > 1:
        nxt = [(level[i] + level[i + 1]).astype(f32) for i in range(0, len(level) - 1, 2)]
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    return level[0]


def np_rows(p, g, acc, *, lr, wd=0.0, eps=1e-10, ss_of=chain_ss):
    """(p', acc') of rows p, g [n, width] with accumulators acc [n], as new float32 arrays."""
    p, g, acc = np.asarray(p, f32), np.asarray(g, f32), np.asarray(acc, f32)
    neg_lr, wdf, ep = f32(-lr), f32(wd), f32(eps)
    with np.errstate(all="ignore"):
        gp = optim_ref.fma32(wdf, p, g) if wdf != 0 else g
        mean = (ss_of(gp) / f32(p.shape[1])).astype(f32)
        acc = (acc + mean).astype(f32)
        std = (np.sqrt(acc).astype(f32) + ep).astype(f32)
        q = ((neg_lr * gp).astype(f32) / std[:, None]).astype(f32)
        return (p + q).astype(f32), acc


def lib_rows(h, p, g, acc):
    """dfwfm_rowwise_adagrad_row_ref over rows, one call per row; (p', acc') as new float32 arrays (the function works
    in place on their memory)."""
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.lib()
    fn = ctypes.CDLL(_lib.LOAD_PATH).dfwfm_rowwise_adagrad_row_ref
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    p = np.array(p, f32, ndmin=2)
    g = np.ascontiguousarray(np.array(g, f32, ndmin=2))
    acc = np.array(acc, f32).reshape(-1)
    n, width = p.shape
    assert g.shape == p.shape and acc.shape == (n,)
    hp, pa, ga, aa = ctypes.addressof(h), p.ctypes.data, g.ctypes.data, acc.ctypes.data
    for r in range(n):
        rc = fn(hp, width, pa + 4 * width * r, ga + 4 * width * r, aa + 4 * r)
        if rc != 0:
            _lib.check(rc, "dfwfm_rowwise_adagrad_row_ref")
    return p, acc


def rowwise_ref(p, g, acc, keys, key_range, kind=PLAIN, c=1, lr=1e-3, weight_decay=0.0, eps=1e-10, elem="np"):
    """(param [rows, width], grad [rows, width], acc [rows]) float32 numpy after one row-wise step for `keys`; the
    inputs are not written.  Untouched rows are copies; touched rows' gradients are zero.  elem: 'np' (np_rows) or
    'lib' (dfwfm_rowwise_adagrad_row_ref, one call per row)."""
    p, g, acc = (np.array(a, dtype=f32, copy=True) for a in (p, g, acc))
    rows = touched_rows(keys, key_range, kind, c)
    assert acc.shape == (p.shape[0],) and (rows.size == 0 or rows.max() < p.shape[0])
    if rows.size == 0:
        return p, g, acc
    if elem == "lib":
        pc, ac = lib_rows(hyper(lr, weight_decay, eps), p[rows], g[rows], acc[rows])
    else:
        pc, ac = np_rows(p[rows], g[rows], acc[rows], lr=lr, wd=weight_decay, eps=eps)
    p[rows], acc[rows] = pc, ac
    g[rows] = 0.0
    return p, g, acc
