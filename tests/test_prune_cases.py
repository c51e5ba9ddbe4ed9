"""The fixtures of tests/prune_cases.py take the paths of the reference's bisection they are meant to take (no GPU):
the device test built on them (tests/test_gpu_prune_edges.py) checks the 101-round cap, the collapsed interval and
the one-round hit only as long as the inputs still end there."""
import pytest
import torch

import prune_cases as pc
from xsdeepfwfm_deprecated_amd.training import binary_search_threshold


@pytest.mark.parametrize("name,builder,target,exit_,rounds,exact", pc.CASES, ids=pc.NAMES)
def test_case_takes_its_path(name, builder, target, exit_, rounds, exact):
    flat = torch.cat([s.reshape(-1) for s in pc.sources(name)])
    thr, n_rounds, how = pc.reference(name)
    # the instrumented copy is the original
    assert thr == binary_search_threshold(flat, target, flat.numel())
    assert how == exit_, (how, n_rounds, thr)
    assert rounds[0] <= n_rounds <= rounds[1], n_rounds
    if exact is not None:
        assert thr == exact
    for s in pc.sources(name):
        assert s.dtype == torch.float32 and s.is_contiguous()


def test_case_inputs_are_what_they_claim():
    (x,) = pc.sources("zero_mass_below")
    assert x.numel() == 50000 and int((x == 0).sum()) == 25000
    (x,) = pc.sources("constant")
    assert x.numel() == 5000 and torch.equal(x.abs(), torch.full((5000,), 0.25)) and (x < 0).any() and (x > 0).any()
    (x,) = pc.sources("few_levels_0.4")
    assert x.numel() == 40000 and len(torch.unique(x)) == 16
    (x,) = pc.sources("one_ulp_0.25")
    u = torch.unique(x)
    assert len(u) == 2 and int(u.view(torch.int32)[1] - u.view(torch.int32)[0]) == 1
    assert int((x == u[0]).sum()) == 20000
    (x,) = pc.sources("above_range_1.0")
    assert int((x == 250.0).sum()) == 100
    (x,) = pc.sources("nan_inf")
    assert int(x.isnan().sum()) == 50 and int(x.isinf().sum()) == 10
    assert int((x.view(torch.int32)[x.isnan()] < 0).sum()) == 25  # NaNs of either sign
    (x,) = pc.sources("denormal")
    tiny = torch.finfo(torch.float32).tiny
    assert int(((x != 0) & (x.abs() < tiny)).sum()) > 29000  # stored denormal, not flushed
    (x,) = pc.sources("tiny")
    assert float(x.abs().max()) < 1e-28 and int((x.abs() < tiny).sum()) == 0
    for n in (8191, 8192, 8193):
        assert pc.sources(f"size_{n}")[0].numel() == n


def test_large_list_shape():
    src = pc.sources("large_list")
    sizes = [s.numel() for s in src]
    assert sizes == pc.LARGE_SIZES and len(sizes) == 41
    assert sizes[:13] == [10] * 13 and sizes[-1] == 1500001
    assert all(40 <= n <= 120000 and n % 256 for n in sizes[13:40]) and len(set(sizes[13:40])) == 27
    assert sum(sizes) > pc.LARGE_MIN_TOTAL


def test_order_alternates_capped_and_one_round_cases():
    """The reuse test walks CASES in order with one workspace: a 101-round case must be followed by a one-round case
    and a one-round case by a 101-round case."""
    ends = [(pc.reference(n)[2], pc.reference(n)[1]) for n in pc.NAMES]
    pairs = list(zip(ends, ends[1:]))
    assert any(a == (pc.CAP, 101) and b == (pc.HIT, 1) for a, b in pairs)
    assert any(a == (pc.HIT, 1) and b == (pc.CAP, 101) for a, b in pairs)
    assert any(a[0] == pc.HIT and a[1] > 12 and b[0] == pc.COLLAPSED for a, b in pairs)


@pytest.mark.parametrize("F", pc.SYM_F)
def test_sym_case_pairs_straddle_the_threshold(F):
    W, tgt, pairs = pc.sym_case(F)
    thr, _, _ = pc.sym_reference(F)  # F * F entries move the rate in steps above 1e-4: a hit or the cap, either will do
    assert W.shape == (F, F)
    sym = 0.5 * (W + W.t())
    assert thr == binary_search_threshold(sym, tgt, W.numel())
    for k, l, zeroed in pairs:
        a, b = abs(float(W[k, l])), abs(float(W[l, k]))
        assert min(a, b) < thr <= max(a, b)  # alone, one would go and one would stay
        assert (abs(float(sym[k, l])) < thr) == zeroed
