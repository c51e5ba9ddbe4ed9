"""The device evaluation metrics (csrc/dfwfm_metrics.hip: radix ranking, three-level scans, tie groups) at the sizes
and values where they can go wrong and continuous random logits at a few odd sizes do not: whole 4096-item tiles, the
digit-count scan's step from one scan tile to two (n = 65536 / 65537), more than 1024 tiles (the top scan's threads take
more than one tile sum each; a Criteo validation split is that large), saturated predictions (the log-loss clamp), one
class only, a NaN logit, a workspace reused after a larger evaluation, and (found here) more than 32 tiles, where the
tile sums of the scan over the ranked items outgrew a buffer sized for the shorter digit-count scan.

The reference is sklearn on torch.sigmoid(z).double(), as in test_gpu_parity (taken per element, see sigmoid32).
Every fixture draws its finite logits from a grid coarse enough that neighbouring distinct f32 predictions are at least
16 ulps apart
(test_fixture_predictions_are_separated, no GPU): a 1-ulp difference between the device's expf and torch's cannot
merge, split or reorder predictions, so tie groups and ranks are the reference's exactly and the AUCs agree to rounding.
No logit lies in (-104, -87), where the prediction is denormal or flushed depending on the implementation."""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

AUC_TOL = 1e-12  # test_gpu_parity.test_device_metrics_exact_on_separated_logits, the same construction
EPS = float(np.finfo(np.float64).eps)


def _grid(levels, lim):
    return np.linspace(-lim, lim, levels).astype(np.float32)


def _labels(rng, z):
    with np.errstate(over="ignore"):
        return (rng.random(len(z)) < 1 / (1 + np.exp(-z.astype(np.float64)))).astype(np.float32)


def _drawn(n, levels, lim, seed):
    rng = np.random.default_rng(seed)
    z = _grid(levels, lim)[rng.integers(0, levels, size=n)]
    return z, _labels(rng, z)


def _distinct_4096():
    rng = np.random.default_rng(4096)
    z = rng.permutation(np.linspace(-4, 4, 4096).astype(np.float32))  # every prediction its own group: G == n
    return z, _labels(rng, z)


def _boundary_8192():
    """401 levels; the 200 highest hold exactly 4096 samples: in ranked order a tie group ends at index 4096, where the
    second tile starts, and the last group ends at index n, where it ends."""
    rng = np.random.default_rng(8192)
    lv = _grid(401, 4)
    cnt = np.full(401, 20)
    cnt[:76] += 1     # the 201 lowest levels: 4020 + 76
    cnt[201:297] += 1  # the 200 highest: 4000 + 96
    z = rng.permutation(np.repeat(lv, cnt))
    return z, _labels(rng, z)


SAT = (30.0, -30.0, 60.0, -60.0, 120.0, -120.0, np.inf, -np.inf)


def _saturated():
    rng = np.random.default_rng(30)
    body = np.round(np.clip(rng.normal(size=4600), -4, 4) * 50) / 50  # N(0, 1) on the 401-level grid of [-4, 4]
    z = np.concatenate([body, np.repeat(SAT, 50)]).astype(np.float32)
    y = np.concatenate([_labels(rng, body.astype(np.float32)), np.tile([1.0, 0.0], 200)]).astype(np.float32)
    p = rng.permutation(len(z))
    return z[p], y[p]


def _with_nan():
    z, y = _drawn(5000, 401, 4, 13)
    z = z.copy()
    z[1234] = np.nan
    return z, y


BIG_N = 4096 * 1024 + 4097  # 1026 tiles: two tile sums per thread of the top scan, and a ragged last tile

BUILDERS = {
    "distinct_4096": _distinct_4096,
    "boundary_8192": _boundary_8192,
    "levels_65536": lambda: _drawn(65536, 401, 4, 65536),
    "levels_65537": lambda: _drawn(65537, 401, 4, 65537),
    "levels_262145": lambda: _drawn(262145, 401, 4, 262145),
    "big": lambda: _drawn(BIG_N, 2001, 6, 1026),
    "saturated": _saturated,
    "no_positives": lambda: (_drawn(5000, 401, 4, 11)[0], np.zeros(5000, np.float32)),
    "no_negatives": lambda: (_drawn(5000, 401, 4, 12)[0], np.ones(5000, np.float32)),
    "one_nan": _with_nan,
    "small_1000": lambda: _drawn(1000, 401, 4, 1000),
}


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(z, y, pred): float32 logits and labels, and the reference's float64 predictions.  Shared: never modify."""
    z, y = BUILDERS[name]()
    pred = sigmoid32(z).astype("float64")
    for a in (z, y, pred):
        a.setflags(write=False)
    return z, y, pred


def sigmoid32(z):
    """torch.sigmoid in float32, one element at a time: the vectorised CPU kernel rounds its SIMD body and its scalar
    tail differently in the last bit, so over a whole array equal logits can get unequal predictions (2002 distinct
    values from 2001 levels at an odd n) and the reference itself would split a tie group."""
    u, inv = np.unique(z, return_inverse=True)
    pu = np.array([torch.sigmoid(torch.tensor(float(v), dtype=torch.float32)).item() for v in u], dtype=np.float32)
    return pu[inv]


def row_log_loss(y, pred):
    """The per-row formula of the kernel's header (sklearn 1.7's log_loss without its label checks), float64."""
    a, b = 1.0 - pred, pred
    s = a + b
    a, b = np.clip(a / s, EPS, 1 - EPS), np.clip(b / s, EPS, 1 - EPS)
    return float(np.mean(np.where(y > 0.5, -np.log(b), -np.log(a))))


@functools.lru_cache(maxsize=None)
def sk(name):
    """sklearn's four metrics on a two-class fixture, computed once."""
    from sklearn.metrics import auc, log_loss, precision_recall_curve, roc_auc_score
    z, y, pred = fixture(name)
    prec, rec, _ = precision_recall_curve(y, pred)
    ll = log_loss(y, pred)
    c = float(np.mean(y == 1))
    return dict(auc=roc_auc_score(y, pred), prauc=auc(rec, prec), log_loss=ll,
                rce=(1.0 - ll / log_loss(y, np.full(len(y), c))) * 100.0)


def device(gpu, name, dm=None):
    from xsdeepfwfm_deprecated_amd.metrics import DeviceMetrics
    z, y, _ = fixture(name)
    return (dm or DeviceMetrics(gpu))(torch.tensor(z, device=gpu), torch.tensor(y, device=gpu))


def check_against_sklearn(m, name):
    z, y, pred = fixture(name)
    ref = sk(name)
    print(name, {k: (m[k], ref[k]) for k in ref}, m["distinct_predictions"])
    assert m["n"] == len(z) and m["positives"] == float((y == 1).sum())
    assert m["distinct_predictions"] == len(np.unique(pred))
    assert abs(m["auc"] - ref["auc"]) < AUC_TOL
    assert abs(m["prauc"] - ref["prauc"]) < AUC_TOL
    assert abs(m["log_loss"] - ref["log_loss"]) < 1e-7 * max(1.0, ref["log_loss"])
    assert abs(m["rce"] - ref["rce"]) < 1e-5  # test_gpu_parity.test_device_metrics_match_sklearn's bar
    assert m["ctr"] == float((y == 1).sum()) / len(y)


# ------------------------------------------------------------------------------------------- the fixtures (no GPU)
@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_fixture_predictions_are_separated(name):
    z, y, pred = fixture(name)
    assert z.dtype == np.float32 and y.dtype == np.float32 and set(np.unique(y)) <= {0.0, 1.0}
    p32 = sigmoid32(z)
    whole = torch.sigmoid(torch.tensor(z)).numpy()
    # within the spread of torch's own SIMD body and scalar tail (a NaN has the same bits in both)
    assert np.abs(p32.view(np.int32).astype(np.int64) - whole.view(np.int32)).max() <= 2
    u = np.unique(p32[~np.isnan(p32)])  # ascending; non-negative floats order like their bit patterns
    gaps = np.diff(u.view(np.int32).astype(np.int64))
    assert gaps.min() >= 16, gaps.min()
    finite = z[np.isfinite(z)]
    assert not ((finite > -104) & (finite < -87)).any()
    assert (u[u > 0] >= np.finfo(np.float32).tiny).all()  # no denormal prediction


def test_fixtures_sit_on_the_edges_they_name():
    z, y, pred = fixture("distinct_4096")
    assert len(z) == 4096 and len(np.unique(pred)) == 4096
    z, y, pred = fixture("boundary_8192")
    r = np.sort(pred)[::-1]
    assert len(r) == 8192 and r[4095] != r[4096] and len(np.unique(pred)) == 401
    assert len(fixture("levels_65536")[0]) == 65536 and len(fixture("levels_65537")[0]) == 65537
    assert len(fixture("big")[0]) == BIG_N > 1024 * 4096 and len(np.unique(fixture("big")[2])) == 2001
    for name in ("distinct_4096", "boundary_8192", "levels_65536", "levels_65537", "levels_262145", "big", "saturated",
                 "small_1000"):
        y = fixture(name)[1]
        assert 0 < y.sum() < len(y)
    # saturation: exactly 1 from z = 30 up, exactly 0 from z = -120 down, both labels at each saturated logit
    z, y, pred = fixture("saturated")
    for v in SAT:
        at = z == np.float32(v)
        assert at.sum() == 50 and y[at].sum() == 25
        if v >= 30:
            assert (pred[at] == 1.0).all()
        if v <= -120:
            assert (pred[at] == 0.0).all()
    assert (pred == 1.0).sum() == 200 and (pred == 0.0).sum() == 100
    assert 0 < pred[z == -60].max() < pred[z == -30].min() < pred[np.abs(z) <= 4].min()
    assert fixture("no_positives")[1].sum() == 0 and fixture("no_negatives")[1].min() == 1
    z = fixture("one_nan")[0]
    assert np.isnan(z).sum() == 1 and len(z) == 5000


def test_reference_conventions():
    """What the device is held to where sklearn's metric functions refuse or warn: the clamp at the float64 eps, PR-AUC
    0.5 without positives (recall 1 at every threshold, then the point (0, 1)) and 1.0 without negatives, and a
    ValueError on a NaN prediction."""
    from sklearn.metrics import auc, log_loss, precision_recall_curve, roc_auc_score
    z, y, pred = fixture("saturated")
    assert abs(log_loss(y, pred) - row_log_loss(y, pred)) < 1e-12
    assert row_log_loss(np.array([0.0, 1.0]), np.array([1.0, 0.0])) == -np.log(EPS)
    assert row_log_loss(np.array([1.0, 0.0]), np.array([1.0, 0.0])) == -np.log(1 - EPS)
    for name, want in (("no_positives", 0.5), ("no_negatives", 1.0)):
        z, y, pred = fixture(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            prec, rec, _ = precision_recall_curve(y, pred)
        assert abs(auc(rec, prec) - want) < 1e-15
    z, y, pred = fixture("one_nan")
    with pytest.raises(ValueError):
        roc_auc_score(y, pred)
    with pytest.raises(ValueError):
        log_loss(y, pred)


# ------------------------------------------------------------------------------------------------------ the device
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["distinct_4096", "boundary_8192", "levels_65536", "levels_65537"])
def test_whole_tiles(gpu, name):
    m = device(gpu, name)
    check_against_sklearn(m, name)
    if name == "distinct_4096":
        assert m["distinct_predictions"] == m["n"] == 4096


@pytest.mark.gpu
def test_more_tile_sums_than_digit_scan_tiles(gpu):
    """The scan over the n ranked items has 16 times the tile sums of the scan over the 256 x tiles digit counts.  Sized
    for the latter, the tile sums of 65 tiles ran over the positives' and groups' totals and the first tiles' log-loss
    sums, all inside the workspace; up to 32 tiles (every size tested before) the 256-byte rounding hid it."""
    check_against_sklearn(device(gpu, "levels_262145"), "levels_262145")


@pytest.mark.gpu
def test_more_than_1024_tiles(gpu):
    check_against_sklearn(device(gpu, "big"), "big")


@pytest.mark.gpu
def test_saturated_predictions(gpu):
    m = device(gpu, "saturated")
    check_against_sklearn(m, "saturated")
    z, y, pred = fixture("saturated")
    ll = row_log_loss(y, pred)
    assert abs(m["log_loss"] - ll) < 1e-7 * max(1.0, ll)
    # the clamp alone: certain and wrong costs -log(eps), certain and right -log(1 - eps), in float64
    zs = torch.tensor([np.inf, 120.0, 30.0, -np.inf, -120.0, 60.0], device=gpu)
    from xsdeepfwfm_deprecated_amd.metrics import DeviceMetrics
    wrong = DeviceMetrics(gpu)(zs, torch.tensor([0.0, 0, 0, 1, 1, 0], device=gpu))
    right = DeviceMetrics(gpu)(zs, torch.tensor([1.0, 1, 1, 0, 0, 1], device=gpu))
    assert abs(wrong["log_loss"] + np.log(EPS)) < 1e-12 and abs(right["log_loss"] + np.log(1 - EPS)) < 1e-18
    assert wrong["distinct_predictions"] == 2 and right["distinct_predictions"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("name,prauc", [("no_positives", 0.5), ("no_negatives", 1.0)])
def test_one_class(gpu, name, prauc):
    """sklearn's one-class conventions (test_reference_conventions).  Without the P == 0 case in
    metrics_groups_kernel, no_positives gave prauc 0.0."""
    m = device(gpu, name)  # rce: no assertion beyond its not raising
    z, y, pred = fixture(name)
    print(name, m)
    assert np.isnan(m["auc"])
    assert abs(m["prauc"] - prauc) < AUC_TOL
    ll = row_log_loss(y, pred)
    assert abs(m["log_loss"] - ll) < 1e-7 * max(1.0, ll)
    assert m["n"] == 5000 and m["positives"] == y.sum() and m["distinct_predictions"] == len(np.unique(pred))


@pytest.mark.gpu
def test_nan_logit_poisons_the_metrics(gpu):
    """sklearn raises ValueError on a NaN prediction; the kernel cannot raise and answers NaN.  Without the NaN case in
    clipped_ll and metrics_final_kernel, all four came out finite and plausible."""
    m = device(gpu, "one_nan")
    z, y, _ = fixture("one_nan")
    print(m)
    for k in ("auc", "prauc", "log_loss", "rce"):
        assert np.isnan(m[k]), (k, m[k])
    assert m["n"] == 5000 and m["positives"] == float(y.sum()) and m["ctr"] == float(y.sum()) / 5000


@pytest.mark.gpu
def test_workspace_reuse_after_a_larger_evaluation(gpu):
    from xsdeepfwfm_deprecated_amd.metrics import DeviceMetrics
    dm = DeviceMetrics(gpu)
    check_against_sklearn(device(gpu, "levels_65537", dm), "levels_65537")
    kept = dm.ws.data_ptr()
    again = device(gpu, "small_1000", dm)
    assert dm.ws.data_ptr() == kept  # the larger workspace, carved anew for n = 1000
    fresh = device(gpu, "small_1000")
    assert again == fresh
    check_against_sklearn(again, "small_1000")


@pytest.mark.gpu
def test_caller_workspace_smallest_unaligned_and_dirty(gpu):
    """dfwfm_eval_metrics on a caller-made workspace: the smallest size dfwfm_metrics_workspace_bytes allows, every
    byte 0xFF, at a base that is not 256-aligned -- nothing is read before it is written, nothing assumes zeros."""
    from xsdeepfwfm_deprecated_amd import _lib
    L = _lib.lib()
    fresh = device(gpu, "small_1000")
    z, y, _ = fixture("small_1000")
    zt, yt = torch.tensor(z, device=gpu), torch.tensor(y, device=gpu)
    need = int(L.dfwfm_metrics_workspace_bytes(1000))
    buf = torch.full((need + 8,), 0xFF, dtype=torch.uint8, device=gpu)
    base = buf.data_ptr() + 8
    assert base % 256 != 0
    out = torch.full((8,), float("nan"), dtype=torch.float64, device=gpu)
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    _lib.check(L.dfwfm_eval_metrics(ctypes.c_void_p(zt.data_ptr()), ctypes.c_void_p(yt.data_ptr()), 1000,
                                    ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(base), need, st),
               "dfwfm_eval_metrics")
    from xsdeepfwfm_deprecated_amd.metrics import DeviceMetrics
    assert dict(zip(DeviceMetrics.NAMES, out.cpu().tolist())) == fresh
    assert bool((buf[:8] == 0xFF).all())  # nothing written below the base
    with pytest.raises(_lib.DfwfmError):
        _lib.check(L.dfwfm_eval_metrics(ctypes.c_void_p(zt.data_ptr()), ctypes.c_void_p(yt.data_ptr()), 1000,
                                        ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(base), need - 1, st),
                   "dfwfm_eval_metrics")
