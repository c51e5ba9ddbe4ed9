"""CPU: the non-finite cases themselves (tests/nonfinite_cases.py) -- every reference's mask for every site, the
placement of the poisons on the skip-list models -- and the host library (libdfwfm_cpu.so, DeepFMs on the CPU) over
every site.  No device needed."""
import numpy as np
import pytest
import torch

import nonfinite_cases as nf
from conftest import model_kwargs

DEEP = ["criteo", "generic", "criteo_qr", "criteo_pruned_mlp", "criteo_qr_pruned_mlp"]
SHALLOW = ["criteo_shallow", "generic_shallow", "criteo_qr_shallow", "criteo_pruned_pairs", "criteo_qr_pruned_pairs"]


@pytest.mark.parametrize("name", DEEP + SHALLOW)
def test_reference_masks_are_the_sites_rows(name):
    """Under the float64 oracle a NaN reaches exactly the rows of its site's scope -- the one row of Xv, the rows
    whose index reads the table row, or every row -- and +Inf leaves exactly those rows not finite."""
    cfg, params, xi, xv = nf.CASES[name]()
    assert xi.shape[0] == nf.ROWS == 40
    f = nf.CAT
    assert sorted(np.flatnonzero(xi[:, f] == nf.CAT_ROW)) == list(nf.READERS)
    assert sorted(np.flatnonzero(xi[:, nf.QR_CAT] // 4 == nf.QR_Q)) == list(nf.READERS)
    assert len(set(xi[list(nf.READERS), nf.QR_CAT] % 4)) == 3  # three remainders: three different rows of weight_r
    masks = nf.expected_masks(name, "f32")
    names = [s.name for s in nf.sites(cfg)]
    assert len(masks) > len(names) and ("table2_qr" in names) == bool(cfg["qr_flag"])
    for s in nf.sites(cfg):
        for v in nf.site_values(s):
            assert np.array_equal(masks[s.name, "nan" if np.isnan(v) else "inf"], nf.site_rows(s)), (s, v)


def test_the_sites_cover_the_edges_of_every_layer():
    cfg = nf.case("criteo")[0]
    names = {s.name for s in nf.sites(cfg)}
    for l, K in ((1, 390), (2, 400), (3, 400)):  # first, middle and last layer: k = 0, K - 1; n = 0 and the tail tile
        assert {f"W{l}[0,0]", f"W{l}[0,{K - 1}]", f"W{l}[399,0]", f"W{l}[399,{K - 1}]", f"b{l}"} <= names
    assert {"Xv", "table2", "table1", "v_num", "field_cov", "lw", "fc", "bias"} <= names
    g = {s.name for s in nf.sites(nf.case("generic")[0])}
    assert "Xv" not in g and "v_num" not in g and {"W1[127,159]", "W2[127,127]"} <= g


@pytest.mark.parametrize("name,refs", [("criteo", ["bf16", "bf16_fold", "int8"]), ("criteo_qr", ["bf16", "int8"]),
                                       ("generic", ["bf16", "bf16_fold"])])
def test_reduced_precision_references_agree_with_the_oracle(name, refs):
    """The bf16 contract, its fold and the int8 contract give the oracle's mask at every site, +Inf included: the
    folded and the unfolded reference agree wherever +Inf is used, and on int8 an infinity is a NaN."""
    want = nf.expected_masks(name, "f32")
    for r in refs:
        got = nf.expected_masks(name, r)
        assert got.keys() == want.keys()
        for k in want:
            assert np.array_equal(got[k], want[k]), (r, k)
    if "int8" in refs:  # the int8 contract on an infinite tower input: not merely not finite
        cfg, params, xi, xv = nf.CASES[name]()
        for s in nf.sites(cfg):
            if s.inf and s.key.startswith(("Xv", "fm_2nd")):
                p2, xv2 = nf.poison(params, xv, s, np.float32(np.inf))
                with np.errstate(all="ignore"):
                    out = nf.reference("int8")(cfg, p2, xi, xv2)
                assert np.isnan(out[nf.site_rows(s)]).all(), s


@pytest.mark.parametrize("name", ["criteo_pruned_mlp", "criteo_pruned_pairs", "criteo_qr_pruned_mlp",
                                  "criteo_qr_pruned_pairs"])
def test_skip_list_models_read_every_poison_through_a_nonzero_entry(name):
    """The sparse MLP's lists and the pruned FwFM pair list read a value only through a nonzero entry (a NaN is one):
    followed along nonzero entries alone, every poison still reaches every row of its scope -- so the oracle's mask
    is what these paths owe."""
    cfg, params, xi, xv = nf.CASES[name]()
    if name.endswith("pruned_mlp"):
        dens = [float((params[f"net_1_linear_{l}.weight"] != 0).mean()) for l in (1, 2, 3)]
        assert max(dens) < 0.25 and all((params[f"net_1_linear_{l}.weight"] != 0).sum(1).min() == 0 for l in (1, 2, 3))
    else:
        R = params["field_cov.weight"]
        kept = int((np.triu(0.5 * (R + R.T), 1) != 0).sum())
        assert 0 < kept <= 192 and R[nf.NUM_F, cfg["numerical"] + nf.CAT] != 0
    for s in nf.sites(cfg):
        for v in nf.site_values(s):
            assert np.array_equal(nf.reaches_logit(cfg, params, xi, xv, s, v), nf.site_rows(s)), (s, v)


# -- the host library ----------------------------------------------------------------------------------------------
def cpu_forward(m):
    def forward(xi, xv):
        with torch.no_grad():
            return m(torch.from_numpy(np.array(xi)), torch.from_numpy(np.array(xv))).numpy()
    return forward


@pytest.mark.parametrize("name", ["criteo", "generic", "criteo_qr", "criteo_shallow", "criteo_qr_shallow",
                                  "criteo_pruned_mlp"])
def test_host_library_propagates_every_site(name):
    """DeepFMs on the CPU: a NaN hidden weight or bias used to end in finite logits (a ReLU written y > 0 ? y : 0)."""
    from xsdeepfwfm_deprecated_amd import DeepFMs
    cfg, params, xi, xv = nf.CASES[name]()
    m = DeepFMs(**model_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    m.eval()
    cells = nf.check_path(cpu_forward(m), m, name, "f32", f"host library, {name}")
    assert cells >= 12
