"""Pruning inputs on which the reference's bisection (training.binary_search_threshold) leaves its usual path, shared
by tests/test_prune_cases.py (the host bisection takes the path each case is meant to take) and
tests/test_gpu_prune_edges.py (the device replay, csrc/dfwfm_prune.hip, returns the same threshold and mask).

Continuous random tensors end the bisection by `|rate - target| < 1e-4` after 19 to 27 rounds: two or three of the
device's nine 12-round passes.  CASES reach what those never do: the 101-round cap (pass 9), the `not lo < hi` exit,
candidate lists whose 4095 mids collapse to one or two f32 keys, a hit in round 1 (every later pass returns early),
NaN / Inf / denormal entries, the sizes around the workgroup-count step at 8192 and a long list of unequal sources
above 256 workgroups' worth of elements.  The order alternates capped, one-round and ordinary cases for the test
that reuses one workspace across all of them."""
import functools

import torch

CAP, HIT, COLLAPSED = "cap", "hit", "collapsed"


def bisect_traced(param, target_percent, total_no):
    """training.binary_search_threshold, also returning the rounds it ran and how it ended: (thr, rounds, exit) with
    exit `hit` (|rate - target| < 1e-4), `collapsed` (not lo < hi) or `cap` (101 rounds)."""
    lo, hi = 0.0, 1e2
    mid = (lo + hi) / 2
    rounds = 0
    for _ in range(101):
        if not lo < hi:
            return mid, rounds, COLLAPSED
        mid = (lo + hi) / 2
        rounds += 1
        rate = (param.abs() < mid).sum().item() * 1.0 / total_no
        if abs(rate - target_percent) < 0.0001:
            return mid, rounds, HIT
        if rate > target_percent:
            hi = mid
        else:
            lo = mid
    return mid, rounds, CAP


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _normal(n, scale, seed):
    return torch.randn(n, generator=_gen(seed)) * scale


def _zero_mass():
    x = _normal(50000, 0.05, 101)
    x[::2] = 0.0  # what re-pruning an already pruned table sees
    return [x]


def _constant():
    sign = torch.randint(0, 2, (5000,), generator=_gen(102)).float() * 2 - 1
    return [sign * 0.25]


def _few_levels():
    return [torch.randint(0, 16, (40000,), generator=_gen(103)).float() / 64]


def _one_ulp():
    a = torch.tensor(0.1, dtype=torch.float32)
    b = torch.nextafter(a, torch.tensor(1.0, dtype=torch.float32))
    x = torch.cat([a.expand(20000), b.expand(20000)])
    return [x[torch.randperm(40000, generator=_gen(104))].contiguous()]


def _plain():
    return [_normal(50000, 0.05, 105)]


def _above_range():
    x = _normal(50000, 0.05, 106)
    x[torch.randperm(50000, generator=_gen(107))[:100]] = 250.0  # above the bisection's (0, 100)
    return [x]


def _nan_inf():
    x = _normal(50000, 0.05, 108)
    at = torch.randperm(50000, generator=_gen(109))[:60]
    x[at[:25]] = float("nan")
    x[at[25:50]] = -float("nan")  # sign bit set
    x[at[50:]] = float("inf")
    return [x]


def _sized(n):
    return lambda: [_normal(n, 0.02, 110 + n)]


LARGE_SIZES = ([10] * 13 +
               [40, 77, 301, 1023, 4097, 8191, 8193, 12345, 20001, 23457, 33333, 40961, 45679, 50007, 54321, 60001,
                65537, 70003, 77777, 80001, 88889, 90001, 99999, 100003, 110001, 117001, 119999] +
               [1500001])
LARGE_MIN_TOTAL = 2097152 + 262144  # 256 workgroups x 4 x 256 lanes x 2 trips, and a ragged rest


def _large_list():
    # unequal sources at unequal scales: every workgroup runs the unrolled loop at least twice on the long source and
    # ends inside a trip on all of them
    return [_normal(n, 0.02 * (1 + i % 5), 200 + i) for i, n in enumerate(LARGE_SIZES)]


# (name, builder of the list of sources, target, exit, (fewest, most) rounds, exact threshold or None)
CASES = [
    ("zero_mass_below", _zero_mass, 0.3, CAP, (101, 101), 100.0 / 2.0 ** 101),
    ("zero_mass_above", _zero_mass, 0.7, HIT, (13, 36), None),
    ("zero_mass_equal", _zero_mass, 0.5, HIT, (20, 101), None),
    ("constant", _constant, 0.5, CAP, (101, 101), None),
    ("few_levels_0.4", _few_levels, 0.4, CAP, (101, 101), None),
    ("few_levels_0.5", _few_levels, 0.5, CAP, (101, 101), None),
    ("one_ulp_0.5", _one_ulp, 0.5, HIT, (25, 101), None),
    ("one_ulp_0.25", _one_ulp, 0.25, CAP, (101, 101), None),
    ("target_one", _plain, 1.0, HIT, (1, 1), None),
    ("denormal", lambda: [_normal(30000, 1e-41, 111)], 0.5, CAP, (101, 101), None),
    ("target_one_again", _plain, 1.0, HIT, (1, 1), None),
    ("tiny", lambda: [_normal(30000, 1e-30, 112)], 0.5, CAP, (101, 101), None),
    ("target_zero", _plain, 0.0, HIT, (20, 101), None),
    ("above_range_1.0", _above_range, 1.0, COLLAPSED, (1, 100), 100.0),
    ("above_range_0.999", _above_range, 0.999, COLLAPSED, (1, 100), 100.0),
    ("nan_inf", _nan_inf, 0.9, HIT, (1, 101), None),
    ("size_8191", _sized(8191), 0.3996, HIT, (1, 101), None),
    ("size_8192", _sized(8192), 0.3996, HIT, (1, 101), None),
    ("size_8193", _sized(8193), 0.3996, HIT, (1, 101), None),
    ("large_list", _large_list, 0.3996, HIT, (1, 101), None),
]
NAMES = [c[0] for c in CASES]
_BY_NAME = {c[0]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def _built(builder):
    return tuple(builder())


def sources(name):
    """The case's source tensors (CPU, float32, contiguous).  Shared between the tests: never modify them."""
    return _built(_BY_NAME[name][1])


def target(name):
    return _BY_NAME[name][2]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(thr, rounds, exit) of the host bisection on the concatenated sources."""
    flat = torch.cat([s.reshape(-1) for s in sources(name)])
    return bisect_traced(flat, target(name), flat.numel())


def host_mask(x, thr):
    """The reference's in-place mask on a copy: x[|x| < thr] = 0."""
    out = x.clone()
    out[out.abs() < thr] = 0
    return out


# ---- the symmetric interaction matrix: threshold and mask from 0.5 * (W + W^T) of the unmodified W
SYM_F = (2, 39, 64)  # 64: the LDS buffer's limit


@functools.lru_cache(maxsize=None)
def sym_case(F):
    """(W, target, pairs): pairs lists (k, l, zeroed) where W[k, l] and W[l, k] lie on opposite sides of the
    threshold and their mean decides (zeroed: the mean is below it)."""
    if F == 2:
        # |sym| = {0.5, 0.35, 0.35, 0.7}: the bisection stops at 0.390625 with half the entries below
        W = torch.tensor([[0.5, 0.8], [-0.1, -0.7]])
        return W, 0.5, ((0, 1, True),)
    W = torch.randn(F, F, generator=_gen(300 + F)) * 0.2
    W[0, 1], W[1, 0] = 0.5, 0.0     # mean 0.25: kept, though W[1, 0] alone is below the threshold
    W[2, 3], W[3, 2] = 0.25, -0.05  # mean 0.10: zeroed, though W[2, 3] alone is above it
    return W, 0.7, ((0, 1, False), (2, 3, True))


@functools.lru_cache(maxsize=None)
def sym_reference(F):
    W, tgt, _ = sym_case(F)
    return bisect_traced(0.5 * (W + W.t()), tgt, W.numel())
