"""GPU: the two list-walking inference paths -- the sparse deep tower (csrc/dfwfm_spmlp.hip) and the FwFM pair list
(dfwfm_model_build_fwfm_pairs, fwd_kernel PART 3) -- bit for bit against the float64 oracle on the structured cases of
tests/pruned_cases.py.

Every operation of those cases is exact in float32 (tests/test_pruned_cases.py proves it, and that one dropped,
duplicated or misplaced list entry changes a logit), so every assertion here is np.array_equal: a differing bit is a
wrong or missing term, never rounding.  The dense kernels run the same models and must give the same bits."""
import numpy as np
import pytest
import torch

import pruned_cases as pc
from conftest import model_kwargs

pytestmark = pytest.mark.gpu
_sid = lambda c: "-".join(str(x) for x in c)


def _model(cfg, params, dev, **attrs):
    from xsdeepfwfm_deprecated_amd import DeepFMs
    m = DeepFMs(**model_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev).eval()
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _run(m, xi, xv, dev):
    with torch.no_grad():
        out = m(torch.from_numpy(xi).to(dev), torch.from_numpy(xv).to(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _copy_in_place(m, params):
    with torch.no_grad():
        own = dict(m.named_parameters())
        for k, v in params.items():
            own[k].copy_(torch.from_numpy(v))  # the same tensors, new versions


# ---------------------------------------------------------------------------------------------- sparse tower
@pytest.mark.parametrize("B", pc.SPARSE_BATCHES)
@pytest.mark.parametrize("shape", pc.SPARSE_SHAPES, ids=_sid)
def test_sparse_tower_and_dense_forward_give_the_oracles_bits(gpu, shape, B):
    D, N, H, F = shape
    cfg, params, xi, xv = pc.sparse_case(D, N, H, F, "A")
    ref = pc.sparse_ref(D, N, H, F, "A")[:B]
    xi, xv = xi[:B], xv[:B]
    m = _model(cfg, params, gpu, sparse_mlp_max_density=1.0)
    got = _run(m, xi, xv, gpu)
    assert m._engine._sparse_on
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)
    for fold in (True, False):  # the dense f32 forward, its numerical fields folded into layer 1 or not
        d = _model(cfg, params, gpu, sparse_mlp_max_density=0.0, fold_numerical=fold)
        dense = _run(d, xi, xv, gpu)
        assert not d._engine._sparse_on
        assert np.array_equal(dense, ref), (fold, np.flatnonzero(dense != ref))


@pytest.mark.parametrize("shape", pc.SPARSE_SHAPES, ids=_sid)
def test_sparse_rows_alone_keep_their_bits(gpu, shape):
    """Rows 0, 63, 64 and B-1 as one-row batches: a row's logit does not depend on its lane, workgroup or batch."""
    D, N, H, F = shape
    cfg, params, xi, xv = pc.sparse_case(D, N, H, F, "A")
    ref = pc.sparse_ref(D, N, H, F, "A")
    for density in (1.0, 0.0):
        m = _model(cfg, params, gpu, sparse_mlp_max_density=density)
        full = _run(m, xi, xv, gpu)
        assert m._engine._sparse_on == (density > 0)
        assert np.array_equal(full, ref)
        for r in (0, 63, 64, len(xi) - 1):
            one = _run(m, xi[r:r + 1], xv[r:r + 1], gpu)
            assert one.shape == (1,) and one[0] == full[r], (density, r)


@pytest.mark.parametrize("shape", pc.SPARSE_SHAPES, ids=_sid)
def test_ell_rebuilt_when_row_lengths_change_under_it(gpu, shape):
    """Pattern A, then B copied into the same parameter tensors (A's lengths mirrored: full rows empty, empty rows
    full), then A again: every run gives a fresh model's bits and the oracle's."""
    D, N, H, F = shape
    a = pc.sparse_case(D, N, H, F, "A")
    b = pc.sparse_case(D, N, H, F, "B")
    refs = dict(A=pc.sparse_ref(D, N, H, F, "A"), B=pc.sparse_ref(D, N, H, F, "B"))
    xi, xv = a[2], a[3]
    assert np.array_equal(xi, b[2]) and np.array_equal(xv, b[3])
    m = _model(a[0], a[1], gpu, sparse_mlp_max_density=1.0)
    for which, case in (("A", a), ("B", b), ("A", a)):
        _copy_in_place(m, case[1])
        got = _run(m, xi, xv, gpu)
        assert m._engine._sparse_on
        assert np.array_equal(got, refs[which]), which
        fresh = _run(_model(case[0], case[1], gpu, sparse_mlp_max_density=1.0), xi, xv, gpu)
        assert np.array_equal(got, fresh), which


def test_density_switch_at_equality(gpu):
    """Every row of layer 1 holds 78 of 312 nonzeros and every row of layer 2 holds 24 of 96: the density is 0.25
    exactly, and `density <= max_density` takes the tower at 0.25 and leaves it one ulp below."""
    cfg, params, xi, xv = pc.sparse_case(8, 96, 2, 39, "density")
    ref = pc.sparse_ref(8, 96, 2, 39, "density")
    m = _model(cfg, params, gpu)
    for density, on in ((0.25, True), (float(np.nextafter(0.25, 0)), False), (0.25, True)):
        m.sparse_mlp_max_density = density
        got = _run(m, xi, xv, gpu)
        assert m._engine._sparse_on == on, density
        assert np.array_equal(got, ref), density


# ------------------------------------------------------------------------------------------------- pair list
PAIRS = [(s, n) for s in pc.PAIR_SHAPES for n in pc.pair_counts(s)]


# (a model with a QR field always takes the eight-wave kernel: no four-wave run of it)
FORMS = [(c, f) for c in PAIRS for f in ("default", "p3ng=4") if not (f == "p3ng=4" and pc.PAIR_SHAPES[c[0]].get("qr"))]


@pytest.mark.parametrize("case,form", FORMS, ids=lambda v: v if isinstance(v, str) else _sid(v))
def test_pair_list_and_gram_give_the_oracles_bits(gpu, monkeypatch, case, form):
    """n pairs with fwfm_pair_max = n (the list is on at equality) and n - 1 (off: the Gram path), on the eight-wave
    kernel (32 lanes per sample) and the four-wave one (16).  fwfm_pair_max = 0 is the switch's off position, so the
    empty list runs with fwfm_pair_max = 1 and the Gram path with 0."""
    shape, n = case
    cfg, params, xi, xv = pc.pairs_case(shape, n)
    ref = pc.pairs_ref(shape, n)
    if form != "default":
        monkeypatch.setenv("DFWFM_DIAG", form)  # read at every launch: set for the whole test
    m = _model(cfg, params, gpu)
    for pair_max, on in ((max(n, 1), True), (n - 1 if n else 0, False)):
        m.fwfm_pair_max = pair_max
        for B in pc.PAIR_BATCHES:
            got = _run(m, xi[:B], xv[:B], gpu)
            assert m._engine._pairs_on == on, (pair_max, B)
            assert np.array_equal(got, ref[:B]), (pair_max, B, np.flatnonzero(got != ref[:B]))
        for r in (0, 16, len(xi) - 1):  # a row alone keeps its bits
            one = _run(m, xi[r:r + 1], xv[r:r + 1], gpu)
            assert one[0] == ref[r], (pair_max, r)


@pytest.mark.parametrize("shape", ["F39-D10", "F64-D16", "F39-D10-qr"])
def test_pair_list_rebuilt_when_its_length_changes_under_it(gpu, shape):
    """33 pairs, then 1, then 0, then 33, copied into the same parameter tensors: every run gives a fresh model's bits
    and the oracle's, and the list stays on."""
    cfg, params, xi, xv = pc.pairs_case(shape, 33)
    m = _model(cfg, params, gpu, fwfm_pair_max=33)
    for n in (33, 1, 0, 33):
        case = pc.pairs_case(shape, n)
        _copy_in_place(m, case[1])
        got = _run(m, case[2], case[3], gpu)
        assert m._engine._pairs_on
        assert np.array_equal(got, pc.pairs_ref(shape, n)), n
        fresh = _run(_model(case[0], case[1], gpu, fwfm_pair_max=33), case[2], case[3], gpu)
        assert np.array_equal(got, fresh), n


# ------------------------------------------------------------------------------------- module-level batch calls
def _tiled(case, ref, n):
    cfg, params, xi, xv = case
    reps = -(-n // len(xi))
    return np.tile(xi, (reps, 1))[:n], np.tile(xv, (reps, 1))[:n], np.tile(ref, reps)[:n]


@pytest.mark.parametrize("path", ["sparse", "pairs"])
def test_predict_and_eval_by_batch_run_the_pruned_paths_per_batch(gpu, path):
    """Three batches of eval_by_batch's 8192 with a ragged last one: with the tower or the list on, eval_batch_sets
    keeps one forward per batch, so predict / predict_proba / eval_by_batch give what one forward per batch gives."""
    from xsdeepfwfm_deprecated_amd import synth
    if path == "sparse":
        case, ref = pc.sparse_case(10, 20, 2, 39, "A"), pc.sparse_ref(10, 20, 2, 39, "A")
        m = _model(case[0], case[1], gpu, sparse_mlp_max_density=1.0)
    else:
        case, ref = pc.pairs_case("F39-D10", 17), pc.pairs_ref("F39-D10", 17)
        m = _model(case[0], case[1], gpu, fwfm_pair_max=17)
    bs, n = 8192, 2 * 8192 + 37
    xi, xv, want = _tiled(case, ref, n)
    y = synth.synth_labels(n, seed=5)
    per_batch = np.concatenate([_run(m, xi[o:o + bs], xv[o:o + bs], gpu) for o in range(0, n, bs)])
    on = m._engine._sparse_on if path == "sparse" else m._engine._pairs_on
    assert on
    assert np.array_equal(per_batch, want)  # the oracle's bits, row by row
    proba = m.predict_proba(xi.reshape(n, -1, 1), xv)
    assert np.array_equal(proba, torch.sigmoid(torch.from_numpy(per_batch).to(gpu)).cpu().numpy())
    assert np.array_equal(m.predict(xi.reshape(n, -1, 1), xv), proba > 0.5)
    res = {}
    for sets in (True, False):
        m.eval_batch_sets = sets
        res[sets] = m.eval_by_batch(xi.reshape(n, -1, 1), xv, y, n)
    assert res[True][:2] == res[False][:2]  # loss and AUC exactly
    on = m._engine._sparse_on if path == "sparse" else m._engine._pairs_on
    assert on
