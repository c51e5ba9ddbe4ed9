"""References of the SGD / Adagrad / RMSprop steps (include/dfwfm_optim.h), shared by tests/test_optim_boundary.py
(CPU) and tests/test_gpu_optim.py (GPU).

Two of them, of the same arithmetic:
  * elem_ref / lib_step: ctypes access to dfwfm_optim_elem_ref, the library's host function -- THE contract the GPU
    tests check the kernels against, one element per call;
  * np_step: a numpy float32 restatement of the header's forms, vectorised, for arrays too long to walk through ctypes
    (the 2049-block grid walk) and as an independent statement of the header.  Its fused multiply-add goes through
    float64: the product of two float32 is exact there, the sum rounds once to float64 and once more to float32.  That
    double rounding can differ from a true fmaf only when the float64 sum lies exactly on a float32 tie while the
    exact sum does not; fma32 detects those elements (the float64 sum's low 29 bits are the half pattern and the
    addition's exact residual, by TwoSum, is not zero) and rounds them by the residual's sign.  The CPU leg verifies
    np_step against the library function bit for bit over every case it runs, and the GPU leg does on a sample of
    whatever long array it uses np_step for; the library function stays the reference wherever both fit.
"""
import ctypes

import numpy as np

f32 = np.float32

KINDS = {"sgd": 0, "adag": 1, "rmsp": 2}  # dfwfm_optim_kind
# the reference's constructions (model/DeepFMs.py:553-560): torch's defaults but for lr, momentum, weight_decay
DEFAULT_EPS = {"sgd": 0.0, "adag": 1e-10, "rmsp": 1e-8}
DEFAULT_ALPHA = 0.99


def hyper(kind, lr, wd=0.0, momentum=0.0, alpha=DEFAULT_ALPHA, eps=None):
    """A dfwfm_optim_hyper of `kind` ('sgd' / 'adag' / 'rmsp' or a raw integer)."""
    from xsdeepfwfm_deprecated_amd import _lib
    k = KINDS[kind] if isinstance(kind, str) else int(kind)
    if eps is None:
        eps = DEFAULT_EPS.get(kind, 0.0)
    return _lib.dfwfm_optim_hyper(k, 0, float(lr), float(wd), float(momentum), float(alpha), float(eps))


def has_state(kind, momentum):
    return kind != "sgd" or momentum != 0.0


def elem_ref(h, step, p, g, s=None):
    """dfwfm_optim_elem_ref on one element: (p', s') as float32 (s' None without a state)."""
    from xsdeepfwfm_deprecated_amd import _lib
    cp = ctypes.c_float(float(p))
    cs = ctypes.c_float(float(s)) if s is not None else None
    _lib.check(_lib.lib().dfwfm_optim_elem_ref(ctypes.byref(h), int(step), ctypes.byref(cp), ctypes.c_float(float(g)),
                                               ctypes.byref(cs) if cs is not None else None), "dfwfm_optim_elem_ref")
    return f32(cp.value), (f32(cs.value) if cs is not None else None)


def lib_step(h, step, p, g, s=None):
    """dfwfm_optim_elem_ref over arrays, one call per element (about a microsecond each: keep them to a few hundred
    thousand elements).  Returns (p', s') as new float32 arrays; the function works in place on their memory, so every
    bit it returns, a NaN's included, is the function's own."""
    from xsdeepfwfm_deprecated_amd import _lib
    _lib.lib()
    # the same symbol of the same loaded library, bound with plain addresses so that element i is base + 4 i
    fn = ctypes.CDLL(_lib.LOAD_PATH).dfwfm_optim_elem_ref
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
    shape = np.shape(p)
    p = np.array(p, f32).reshape(-1)
    g = np.ascontiguousarray(np.asarray(g, f32).reshape(-1))
    s = None if s is None else np.array(s, f32).reshape(-1)
    n = p.size
    if n == 0:
        return p.reshape(shape), s
    ga = g.tolist()  # (a float32 NaN gradient arrives as some NaN; nothing but its being one is part of the contract)
    hp, step = ctypes.addressof(h), int(step)
    pa, sa = p.ctypes.data, (s.ctypes.data if s is not None else None)
    for i in range(n):
        rc = fn(hp, step, pa + 4 * i, ga[i], sa + 4 * i if sa is not None else None)
        if rc != 0:
            _lib.check(rc, "dfwfm_optim_elem_ref")
    return p.reshape(shape), (None if s is None else s.reshape(shape))


def fma32(a, b, c):
    """fmaf(a, b, c) over float32 arrays: one rounding of the exact a * b + c (see the module docstring)."""
    a, b, c = np.broadcast_arrays(a, b, c)
    shape = a.shape
    a, b, c = (np.asarray(x, f32).astype(np.float64).reshape(-1) for x in (a, b, c))
    with np.errstate(all="ignore"):
        prod = a * b                      # exact: 24 + 24 significant bits
        s = prod + c                      # one rounding to float64
        r = s.astype(f32)                 # a second one to float32
        bb = s - prod                     # TwoSum: err is the exact residual (prod + c) - s
        err = (prod - (s - bb)) + (c - bb)
        tie = ((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (err != 0) & np.isfinite(s) & \
            np.isfinite(err)
        if tie.any():  # s is midway between two float32 values, the exact sum is not: the residual's sign decides
            rt = r[tie]
            up = np.nextafter(rt, f32(np.inf))
            dn = np.nextafter(rt, f32(-np.inf))
            below = rt.astype(np.float64) < s[tie]                     # r is the lower neighbour of s
            lo, hi = np.where(below, rt, dn), np.where(below, up, rt)
            r[tie] = np.where(err[tie] > 0, hi, lo)
    return r.reshape(shape) if shape else r[0]


def np_step(kind, step, p, g, s=None, *, lr, wd=0.0, momentum=0.0, alpha=DEFAULT_ALPHA, eps=None):
    """The header's forms in numpy float32.  Returns (p', s') as new arrays (s' None for plain SGD)."""
    if eps is None:
        eps = DEFAULT_EPS[kind]
    p = np.asarray(p, f32)
    g = np.asarray(g, f32)
    neg_lr, wdf, mom, al, oma, ep = f32(-lr), f32(wd), f32(momentum), f32(alpha), f32(1.0 - alpha), f32(eps)
    with np.errstate(all="ignore"):
        if wdf != 0:
            g = fma32(wdf, p, g)
        if kind == "sgd":
            if momentum != 0.0:
                s = g.copy() if step == 1 else ((np.asarray(s, f32) * mom).astype(f32) + g).astype(f32)
                d = s
            else:
                s, d = None, g
            return fma32(d, neg_lr, p), s
        s = np.asarray(s, f32)
        if kind == "adag":
            s = fma32(g, g, s)
        else:
            s = fma32(g, (oma * g).astype(f32), (s * al).astype(f32))
        den = (np.sqrt(s).astype(f32) + ep).astype(f32)
        q = ((neg_lr * g).astype(f32) / den).astype(f32)
        return (p + q).astype(f32), s


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.int32)


def same_bits(a, b):
    """Bit equality, every NaN counting as equal to every NaN (a NaN's payload and sign are not part of the
    contract: x86 and gfx950 propagate them differently)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def torch_optimizer(kind, params, lr, wd, momentum):
    """torch.optim's optimizer as the reference constructs it (model/DeepFMs.py:553-560), single-tensor form."""
    import torch
    if kind == "sgd":
        return torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=wd, foreach=False)
    if kind == "adag":
        return torch.optim.Adagrad(params, lr=lr, weight_decay=wd, foreach=False)
    return torch.optim.RMSprop(params, lr=lr, weight_decay=wd, foreach=False)


TORCH_STATE = {"sgd": "momentum_buffer", "adag": "sum", "rmsp": "square_avg"}
