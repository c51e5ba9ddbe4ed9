"""The device bisection replay (csrc/dfwfm_prune.hip) on the inputs of tests/prune_cases.py: the threshold equals the
host bisection's bit for bit, as the kernel's header claims, on the paths continuous random tensors never reach (the
101-round cap in pass 9, the collapsed interval, candidate lists of one or two distinct f32 keys, a hit in round 1,
NaN / Inf / denormal entries, the workgroup-count step at 8192 elements, the unrolled loop running twice over a long
list of unequal sources), and the applied mask equals the host's."""
import pytest
import torch

import prune_cases as pc

pytestmark = pytest.mark.gpu


def _pruner(gpu):
    from xsdeepfwfm_deprecated_amd.training import DevicePruner
    return DevicePruner(gpu)


def _same_bits(got, ref):
    """torch.equal, with NaNs compared where they stand (they stay NaN, payload and sign included) and a written
    zero required to be +0 as the host's."""
    return torch.equal(got.view(torch.int32), ref.view(torch.int32))


@pytest.mark.parametrize("name", pc.NAMES)
def test_threshold_and_mask_equal_host_bisection(gpu, name):
    thr_ref, rounds, how = pc.reference(name)
    pr = _pruner(gpu)
    dev = [s.to(gpu) for s in pc.sources(name)]
    thr = pr.threshold([(d, 0) for d in dev], pc.target(name))
    got = thr.item()
    print(f"{name}: device {got!r} host {thr_ref!r} ({how}, {rounds} rounds)")
    assert got == thr_ref, (name, got, thr_ref, how, rounds)
    for d in dev:
        pr.apply(d, thr)
    torch.cuda.synchronize()
    for d, s in zip(dev, pc.sources(name)):
        ref = pc.host_mask(s, thr_ref)
        out = d.cpu()
        assert torch.equal(out.isnan(), s.isnan())
        assert torch.equal(out.nan_to_num(nan=7.0), ref.nan_to_num(nan=7.0))
        assert _same_bits(out, ref)


@pytest.mark.parametrize("F", pc.SYM_F)
def test_symmetric_mask_follows_the_mean(gpu, F):
    W, tgt, pairs = pc.sym_case(F)
    thr_ref, _, _ = pc.sym_reference(F)
    pr = _pruner(gpu)
    d = W.to(gpu)
    thr = pr.threshold([(d, F)], tgt)
    assert thr.item() == thr_ref, (F, thr.item(), thr_ref)
    pr.apply(d, thr, F)
    torch.cuda.synchronize()
    sym = 0.5 * (W + W.t())  # of the unmodified W
    ref = W.clone()
    ref[sym.abs() < thr_ref] = 0
    out = d.cpu()
    assert _same_bits(out, ref)
    for k, l, zeroed in pairs:
        if zeroed:
            assert out[k, l] == 0 and out[l, k] == 0
        else:
            assert out[k, l] == W[k, l] and out[l, k] == W[l, k]


def test_one_workspace_across_all_cases(gpu):
    """One DevicePruner (workspace: state, ticket, candidate list, histograms) through CASES in order -- capped,
    one-round, capped, collapsed ... -- and the first case again: nothing of a bisection outlives it."""
    pr = _pruner(gpu)
    for name in pc.NAMES + [pc.NAMES[0]]:
        dev = [s.to(gpu) for s in pc.sources(name)]
        got = pr.threshold([(d, 0) for d in dev], pc.target(name)).item()
        assert got == pc.reference(name)[0], (name, got, pc.reference(name))


def test_source_limit(gpu):
    from xsdeepfwfm_deprecated_amd._lib import DfwfmError
    from xsdeepfwfm_deprecated_amd.training import binary_search_threshold
    g = torch.Generator().manual_seed(96)
    src = [torch.randn(16, generator=g) * 0.1 for _ in range(97)]
    flat = torch.cat(src[:96])
    ref = binary_search_threshold(flat, 0.4, flat.numel())
    pr = _pruner(gpu)
    dev = [s.to(gpu) for s in src]
    thr = pr.threshold([(d, 0) for d in dev[:96]], 0.4)
    assert thr.item() == ref
    for d, s in zip(dev[:96], src):
        pr.apply(d, thr)
        assert torch.equal(d.cpu(), pc.host_mask(s, ref))
    with pytest.raises(DfwfmError, match="more than 96 pruning sources"):
        pr.threshold([(d, 0) for d in dev], 0.4)
