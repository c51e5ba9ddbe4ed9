"""CPU: the rounding witnesses themselves (tests/rounding_witness.py).  These are conditions on the references alone,
not measurements of a kernel: every rounding site of the bf16 and int8 contracts meets at least 32 exact ties over the
96 rows, at least 8 that ties-to-even rounds down and 8 that it rounds up; everything else is exact in float32 in any
order; and a wrong rule (half away from zero, truncation) at any one site moves the float32 logits of at least a
quarter of the rows -- without that the device test would prove nothing."""
import numpy as np
import pytest

import bf16_emul
import bf16_fold_emul
import int8_emul
import rounding_witness as rw
from oracle import dfwfm_oracle

f32 = np.float32
QUARTER = rw.ROWS // 4


def moved(a, b):
    return int((np.asarray(a, dtype=np.float64).astype(f32) != np.asarray(b, dtype=np.float64).astype(f32)).sum())


def enough(counts, what):
    ties, down, up = counts
    print(what, dict(ties=ties, down=down, up=up))
    assert ties >= 32 and down >= 8 and up >= 8, (what, counts)


# -- bf16 ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bf16():
    case = rw.bf16_case()
    pre, pref = {}, {}
    return case, rw.bf16_logits(case, pre=pre), pre, rw.bf16_logits(case, fold=True, pre=pref), pref


def test_bf16_witness_default_rules_are_the_contracts(bf16):
    (cfg, params, xi, xv), e, _, ef, _ = bf16
    assert xi.shape[0] == 96 and (cfg["field_size"], cfg["numerical"], cfg["h_depth"]) == (39, 13, 3)
    assert np.array_equal(e, bf16_emul.forward(cfg, params, xi, xv))
    assert np.array_equal(ef, bf16_fold_emul.forward(cfg, params, xi, xv))
    assert np.array_equal(rw.folded_p32(cfg, params), rw.folded_p32(cfg, params).astype(np.float64).astype(f32))
    assert np.array_equal(rw.bf16_rne(rw.folded_p32(cfg, params)), bf16_fold_emul.folded_p(cfg, params))
    rw.as_f32(e), rw.as_f32(ef)  # nothing left to round in the logits
    # the rounding is live: neither is the float64 oracle's float32 answer
    o = dfwfm_oracle.forward(cfg, params, xi, xv)
    assert moved(e, o) >= QUARTER and moved(ef, o) >= QUARTER


def test_bf16_witness_ties_at_every_site(bf16):
    _, _, pre, _, pref = bf16
    enough(rw.bf16_ties(pre["x0"]), "x0 = bf16(E)")
    for l, h in enumerate(pre["xl"], 1):
        enough(rw.bf16_ties(h), f"x{l} = bf16(h_{l})")
    assert len(pre["w"]) == 3
    for l, w in enumerate(pre["w"], 1):
        enough(rw.bf16_ties(w), f"bf16(W{l})")
    enough(rw.bf16_ties(pref["xv"]), "fold: bf16(Xv)")
    enough(rw.bf16_ties(pref["p"]), "fold: bf16(P)")
    for l, h in enumerate(pref["xl"], 1):
        enough(rw.bf16_ties(h), f"fold: x{l}")


def test_bf16_witness_sums_are_exact_in_any_order(bf16):
    """Every layer's terms are multiples of one power of two whose magnitudes sum below 2^24 of it, the output sum
    too; and bf16_emul's float32 accumulation gives the float64 bits under several shuffles of K."""
    (cfg, params, xi, xv), e, pre, ef, pref = bf16
    for p in (pre, pref):
        for x, w, b in p["layers"]:
            assert rw.exact_in_f32(x, w, b)
        h, fc = p["last"]
        assert rw.exact_in_f32(h, fc[None, :])
    for seed, chunk in ((1, 32), (2, 7), (3, 64), (4, 1)):
        assert np.array_equal(bf16_emul.forward(cfg, params, xi, xv, acc=np.float32, k_order=(seed, chunk)), e)
    assert np.array_equal(bf16_emul.forward(cfg, params, xi, xv, acc=np.float32), e)
    assert np.array_equal(bf16_fold_emul.forward(cfg, params, xi, xv, acc=np.float32), ef)
    R = params["field_cov.weight"]
    for f in rw.TIE_XV:  # the fields that carry ties stay out of the f32 second order
        assert not R[f].any() and not R[:, f].any()


@pytest.mark.parametrize("rule", ["away", "trunc"])
@pytest.mark.parametrize("site", rw.BF16_SITES + ("xl1", "xl2", "w1", "w2", "w3") + tuple("fold:" + s for s in
                                                                                   rw.BF16_SITES + rw.FOLD_SITES))
def test_bf16_witness_sees_a_wrong_rule_at_one_site(bf16, site, rule):
    case, e, _, ef, _ = bf16
    fold = site.startswith("fold:")
    got = rw.bf16_logits(case, rules={site.split(":")[-1]: rule}, fold=fold)
    n = moved(got, ef if fold else e)
    print(site, rule, "rows moved:", n)
    assert n >= QUARTER


# -- int8 ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def int8():
    case = rw.int8_case()
    pre = {}
    return case, rw.int8_logits(case, pre=pre), pre


def test_int8_witness_default_rules_are_the_contract(int8):
    (cfg, params, xi, xv), e, pre = int8
    assert xi.shape[0] == 96 and (cfg["field_size"], cfg["numerical"], cfg["h_depth"]) == (39, 13, 2)
    assert np.array_equal(e, int8_emul.forward(cfg, params, xi, xv))
    assert np.array_equal(e, int8_emul.forward(cfg, params, xi, xv, fma=False))  # the epilogue has nothing to round
    rw.as_f32(e)
    assert moved(e, dfwfm_oracle.forward(cfg, params, xi, xv)) >= QUARTER


def test_int8_witness_ties_and_exactness(int8):
    (cfg, params, xi, xv), e, pre = int8
    for l in (0, 1):
        enough(rw.int_ties(pre["q"][l]), f"q, layer {l + 1}")
        enough(rw.int_ties(pre["qW"][l]), f"qW, layer {l + 1}")
        inv = pre["inv"][l]
        assert set(np.unique(inv)) <= {0.0, 1.0, 4.0}  # a power of two (0: the zero row)
        assert np.array_equal(pre["q"][l] * 2, np.round(pre["q"][l] * 2))  # quotients are (half-)integers: exact
        assert np.array_equal(pre["qW"][l] * 2, np.round(pre["qW"][l] * 2))
    z = rw.ZERO_ROW
    assert pre["inv"][0][z] == 0 and (pre["inv"][0][np.arange(96) != z] == 1).all() and (pre["inv"][1] == 4).all()
    h1, h2 = pre["h"]
    assert h1.max() == 31.75 and (h1[:, 0] == 31.75).all() and (h1[:, 1] == 0).all()
    # the all-zero input row and the all-zero weight rows: relu(b) exactly
    b1, b2 = params["net_1_linear_1.bias"], params["net_1_linear_2.bias"]
    assert np.array_equal(h1[z], np.maximum(b1, 0)) and (h1[z] > 0).sum() > 100
    n = rw.ZERO_NEURON
    assert not params["net_1_linear_1.weight"][n].any() and not params["net_1_linear_2.weight"][n].any()
    assert (h1[:, n] == b1[n]).all() and (h2[:, n] == b2[n]).all() and b1[n] > 0 and b2[n] > 0
    assert params["net_1_fc.weight"][0, n] != 0
    # the output sum and the logit: multiples of 2^-5 far below 2^24 of it, in any order
    h, fc = pre["last"]
    assert rw.exact_in_f32(h, fc[None, :]) and rw.lsb(h) <= 4 and rw.lsb(e) <= 5 and np.abs(e).max() < 2 ** 18
    _, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    assert rw.lsb(parts["first"]) <= 3 and rw.lsb(parts["second"]) <= 3 and rw.lsb(parts["E"]) == 1


@pytest.mark.parametrize("rule", ["away", "trunc"])
@pytest.mark.parametrize("site", rw.INT8_SITES + ("q1", "q2", "qW1", "qW2"))
def test_int8_witness_sees_a_wrong_rule_at_one_site(int8, site, rule):
    case, e, _ = int8
    n = moved(rw.int8_logits(case, rules={site: rule}), e)
    print(site, rule, "rows moved:", n)
    assert n >= QUARTER
