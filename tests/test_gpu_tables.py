"""GPU: every HIP forward on the table zoo (tests/table_cases.py) -- tables of 1 .. 1031 rows around the row counts where
kernels change path, QR collision counts c from 1 (one remainder row) to 5000 (> n: one quotient row), "mult" and "add",
with the three forced rows at the ends of every table's index range.  Each forward turns an index into table rows with
its own copy of the arithmetic (plain row; QR: i // c and i % c); the suite ran them at c = 4 only.

Reference: the float64 oracle at 1e-5 * max(1, |ref|) for the f32 routes; the bf16 / folded bf16 / int8 contracts in
numpy with their own conditions for those towers.  A route that could refuse a shape asserts that it ran:

    route                      how the test knows it ran
    gather                     ForwardEngine.forward_gather called directly
    f32 r32 = 0 / 1            DFWFM_DIAG; the library has no query, so the test asserts the shape fwd32_supported takes
                               (F D in 385 .. 400, N = 400: the 39-field zoo) -- the same rule as csrc/dfwfm_fwd32.hip
    batch set                  ForwardEngine.forward_batches called directly
    small batch                a spy on ForwardEngine.forward_small counts one call per module forward
    bf16 per layer             engine.bf16 and not engine.bf16_fused
    bf16 fused / its set       bf16_fused_supported() and engine.bf16_fused, fold off / forward_bf16_batches directly
    bf16 fused + folded        engine.bf16_fused and engine._bf16_fold_on is True
    int8 / its set             int8_supported() and engine.int8 / forward_int8_batches directly
    sparse tower               engine._sparse_on
    MLP-free part3 / part3=0   use_deep = 0 (the model has no other forward); DFWFM_DIAG part3=0 for the generic kernel
    serving copy on / off      engine._packed_on is the switch's value
"""
import numpy as np
import pytest
import torch

import bf16_emul
import bf16_fold_emul
import int8_emul
import table_cases as zc
from conftest import logit_close
from oracle import dfwfm_oracle
from test_gpu_parity import make_model, run

pytestmark = pytest.mark.gpu

CASES_ALL = [(c, op) for c in zc.C_ALL for op in zc.OPS]
CASES_FEW = [(c, op) for c in zc.C_FEW for op in zc.OPS]


def dev(gpu, *arrs):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrs)


def np32_embeddings(cfg, params, xi, xv):
    """deep_emb [B, F D] as numpy float32 computes it: every entry one IEEE product (v_f[0] Xv; Wq Wr), one sum
    (Wq + Wr) or a copy -- one rounding, so the kernel's value must be these bits."""
    num, c = cfg["numerical"], cfg["qr_collisions"]
    cols = []
    for f in range(cfg["field_size"]):
        k = f"fm_2nd_embeddings.{f}"
        if f < num:
            cols.append(xv[:, f:f + 1].astype(np.float32) * params[k + ".weight"][0][None, :])
        elif k + ".weight" in params:
            cols.append(params[k + ".weight"][xi[:, f - num]])
        else:
            q, r = params[k + ".weight_q"][xi[:, f - num] // c], params[k + ".weight_r"][xi[:, f - num] % c]
            cols.append(q * r if cfg["qr_operation"] == "mult" else q + r)
    out = np.concatenate(cols, axis=1)
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("c,op", CASES_ALL)
def test_forward_gather_rows_are_bit_exact(gpu, c, op):
    cfg, params, xi, xv = zc.zoo(1, op, c)
    m = make_model(cfg, params, gpu)
    with torch.no_grad():
        E, fs = m._sync_engine(gpu).forward_gather(*dev(gpu, xi, xv))
    E, fs = E.cpu().numpy(), fs.cpu().numpy()
    FD = cfg["field_size"] * cfg["embedding_size"]
    assert np.array_equal(E[:, :FD], np32_embeddings(cfg, params, xi, xv))
    assert E.shape[1] == -(-FD // 16) * 16 and not E[:, FD:].any()
    _, parts = dfwfm_oracle.forward(cfg, params, xi, xv, return_parts=True)
    assert logit_close(fs, parts["first"] + parts["second"]) < 1e-5
    assert m._engine.read_error_flag() == 0  # forced row 2 (i >= n in a QR field) is valid


@pytest.mark.parametrize("c,op", CASES_ALL)
def test_lone_f32_forward_both_kernels(gpu, monkeypatch, c, op):
    """fwd_kernel (r32=0) and fwd32_kernel (r32=1) on the 39-field zoo: the oracle's logits, equal bits between the
    two, and every row run alone bit-identical to its value in the batch.  Also the 18-field zoo (the generic K loop)
    against the oracle."""
    cfg, params, xi, xv = zc.zoo(1, op, c, wide=True)
    F, D, N = cfg["field_size"], cfg["embedding_size"], cfg["deep_nodes"]
    assert D == 10 and F <= 48 and -(-F * D // 16) == 25 and N == 400 and cfg["h_depth"] >= 1  # fwd32_supported
    ref = dfwfm_oracle.forward(cfg, params, xi, xv)
    outs = {}
    for r32 in ("0", "1"):
        monkeypatch.setenv("DFWFM_DIAG", f"r32={r32}")
        m = make_model(cfg, params, gpu)
        outs[r32] = run(m, xi, xv, gpu)
        assert logit_close(outs[r32], ref) < 1e-5, r32
        alone = np.concatenate([run(m, xi[b:b + 1], xv[b:b + 1], gpu) for b in range(len(xi))])
        assert np.array_equal(alone, outs[r32]), r32
    assert np.array_equal(outs["0"], outs["1"])
    monkeypatch.delenv("DFWFM_DIAG")
    cfg, params, xi, xv = zc.zoo(1, op, c)
    got = run(make_model(cfg, params, gpu), xi, xv, gpu)
    assert logit_close(got, dfwfm_oracle.forward(cfg, params, xi, xv)) < 1e-5


# ------------------------------------------------------------------------------------------------------ the routes
def pruned(params, sparse=0.9):
    """The hidden layers magnitude-pruned to `sparse` (the reference's masks: |w| below the layer's quantile)."""
    p = dict(params)
    for k in params:
        if k.startswith("net_1_linear") and k.endswith("weight"):
            w = params[k].copy()
            w[np.abs(w) < np.quantile(np.abs(w), sparse)] = 0.0
            p[k] = w
    return p


def oracle_bar(got, cfg, params, xi, xv, what):
    assert logit_close(got, dfwfm_oracle.forward(cfg, params, xi, xv)) < 1e-5, what


def bf16_bar(got, cfg, params, xi, xv, what):
    bf16_emul.assert_conditions(got, bf16_emul.forward(cfg, params, xi, xv),
                                dfwfm_oracle.forward(cfg, params, xi, xv), what)


def bf16_fold_bar(got, cfg, params, xi, xv, what):
    bf16_emul.assert_conditions(got, bf16_fold_emul.forward(cfg, params, xi, xv),
                                dfwfm_oracle.forward(cfg, params, xi, xv), what)


def int8_bar(got, cfg, params, xi, xv, what):
    int8_emul.assert_conditions(got, int8_emul.forward(cfg, params, xi, xv),
                                dfwfm_oracle.forward(cfg, params, xi, xv), what)


def _set(method):
    """A batch set of three batches (the rows, the rows reversed, the rows rotated by 7) through the engine's
    `method`; returns the three outputs in the rows' own order, concatenated."""
    def go(m, xi, xv, gpu):
        B = len(xi)
        orders = [np.arange(B), np.arange(B)[::-1], np.roll(np.arange(B), 7)]
        with torch.no_grad():
            eng = m._sync_inference(gpu)
            outs = [torch.full((B,), float("nan"), device=gpu) for _ in orders]
            getattr(eng, method)([dev(gpu, xi[o], xv[o]) for o in orders], outs)
        torch.cuda.synchronize()
        back = []
        for o, t in zip(orders, outs):
            a = np.empty(B, np.float32)
            a[o] = t.cpu().numpy()
            back.append(a)
        assert np.array_equal(back[0], back[1]) and np.array_equal(back[0], back[2])  # a row's bits: any slot
        m.check_index_errors()
        return back[0]
    return go


def _module(m, xi, xv, gpu):
    return run(m, xi, xv, gpu)


def _small(m, xi, xv, gpu):
    eng = m._sync_inference(gpu)
    calls, orig = [], eng.forward_small
    eng.forward_small = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        out = run(m, xi, xv, gpu)
    finally:
        del eng.forward_small
    assert len(calls) == 1
    return out


def _taken(**want):
    def check(m):
        for k, v in want.items():
            assert getattr(m._engine, k) is v, (k, getattr(m._engine, k))
    return check


# name: (model variant, module switches, DFWFM_DIAG, forward, route-taken check, reference and bar)
ROUTES = {
    "batch_set": (dict(), dict(), None, _set("forward_batches"), None, oracle_bar),
    "small": (dict(), dict(small_batch_rows=zc.B_FWD), None, _small, None, oracle_bar),
    "bf16": (dict(), dict(mlp_dtype="bf16"), None, _module, _taken(bf16=True, bf16_fused=False), bf16_bar),
    "bf16_fused": (dict(), dict(mlp_dtype="bf16", bf16_fused=True), None, _module,
                   _taken(bf16=True, bf16_fused=True, _bf16_fold_on=False), bf16_bar),
    "bf16_set": (dict(), dict(mlp_dtype="bf16", bf16_fused=True), None, _set("forward_bf16_batches"),
                 _taken(bf16=True, bf16_fused=True, _bf16_fold_on=False), bf16_bar),
    "bf16_fold": (dict(), dict(mlp_dtype="bf16", bf16_fused=True, bf16_fold=True), None, _module,
                  _taken(bf16=True, bf16_fused=True, _bf16_fold_on=True), bf16_fold_bar),
    "int8": (dict(), dict(mlp_dtype="int8"), None, _module, _taken(int8=True), int8_bar),
    "int8_set": (dict(), dict(mlp_dtype="int8"), None, _set("forward_int8_batches"), _taken(int8=True), int8_bar),
    "sparse": (dict(prune=True), dict(sparse_mlp_max_density=0.25), None, _module, _taken(_sparse_on=True), oracle_bar),
    "shallow_part3": (dict(deep=0), dict(), None, _module, None, oracle_bar),
    "shallow_generic": (dict(deep=0), dict(), "part3=0", _module, None, oracle_bar),
    "shallow_set": (dict(deep=0), dict(), None, _set("forward_batches"), None, oracle_bar),
}


def route_model(route, gpu, monkeypatch, c, op, qr=1):
    variant, switches, diag, fwd, taken, bar = ROUTES[route]
    cfg, params, xi, xv = zc.zoo(qr, op, c, deep=variant.get("deep", 1))
    if variant.get("prune"):
        params = pruned(params)
    if diag:
        monkeypatch.setenv("DFWFM_DIAG", diag)
    m = make_model(cfg, params, gpu)
    for k, v in switches.items():
        setattr(m, k, v)
    if cfg["use_deep"]:
        with torch.no_grad():
            eng = m._sync_inference(gpu)
            assert eng.bf16_fused_supported() and eng.int8_supported()  # the zoo's shape: no route drops out
    return m, cfg, params, xi, xv


@pytest.mark.parametrize("c,op", CASES_FEW)
@pytest.mark.parametrize("route", list(ROUTES))
def test_route_on_the_zoo(gpu, monkeypatch, route, c, op):
    """Each forward route on the zoo against its own reference and bar; the route's own switch is checked after."""
    _, _, _, fwd, taken, bar = ROUTES[route]
    m, cfg, params, xi, xv = route_model(route, gpu, monkeypatch, c, op)
    got = fwd(m, xi, xv, gpu)
    if taken:
        taken(m)
    bar(got, cfg, params, xi, xv, (route, c, op))


@pytest.mark.parametrize("deep", [1, 0])
def test_plain_zoo_serving_copy_on_and_off(gpu, deep):
    """qr_flag = 0: every table of the zoo a plain bag (1 .. 1031 rows) read through the serving copy (second-order row
    and first-order weight in one 64-byte row) or from the tables: equal bits, lone batch and batch set, and the
    oracle's logits."""
    cfg, params, xi, xv = zc.zoo(0, "mult", 7, deep=deep)
    m = make_model(cfg, params, gpu)
    outs = {}
    for packed in (True, False):
        m.pack_tables = packed
        lone = run(m, xi, xv, gpu)
        assert m._engine._packed_on is packed
        outs[packed] = (lone, _set("forward_batches")(m, xi, xv, gpu))
        assert m._engine._packed_on is packed
    assert np.array_equal(outs[True][0], outs[False][0]) and np.array_equal(outs[True][1], outs[False][1])
    oracle_bar(outs[True][0], cfg, params, xi, xv, "lone")
    oracle_bar(outs[True][1], cfg, params, xi, xv, "set")


@pytest.mark.parametrize("route", ["gather", "f32", "r32_0", "r32_1", "plain_packed", "plain_unpacked"] + list(ROUTES))
def test_index_range_on_every_route(gpu, monkeypatch, route):
    """c = 7 divides none of the QR fields' sizes.  The first invalid index of the 1-row table, of a plain field and of
    a QR field (ceil(n / c) c, not n), then -1 and 2^32 + 3 (valid low 32 bits): each raises IndexError; the flag is
    cleared by the read, and the clean batch -- whose row 2 holds the last valid index of every field, >= n for the QR
    fields -- passes at the route's bar."""
    c, op = 7, "mult"
    if route in ("gather", "f32", "r32_0", "r32_1", "plain_packed", "plain_unpacked"):
        cfg, params, xi, xv = zc.zoo(0 if route.startswith("plain") else 1, op, c, wide=route.startswith("r32"))
        if route.startswith("r32"):  # the 39-field zoo: fwd_kernel's static K loop and fwd32_kernel
            monkeypatch.setenv("DFWFM_DIAG", f"r32={route[-1]}")
        m = make_model(cfg, params, gpu)
        m.pack_tables = route != "plain_unpacked"
        bar = oracle_bar
        if route == "gather":
            def fwd(m, xi, xv, gpu):
                with torch.no_grad():
                    m._sync_engine(gpu).forward_gather(*dev(gpu, xi, xv))
                m.check_index_errors()
                return None
        else:
            fwd = _module
    else:
        _, _, _, fwd, _, bar = ROUTES[route]
        m, cfg, params, xi, xv = route_model(route, gpu, monkeypatch, c, op)
    if cfg["qr_flag"]:  # row 2: i >= n and still valid, in every QR field whose n is no multiple of c
        n = np.asarray(cfg["feature_sizes"][cfg["numerical"]:])
        past = (n > cfg["qr_threshold"]) & (n % c != 0)
        assert past.sum() >= 7 and (xi[2] >= n)[past].all()
    for what, bad in zc.bad_inputs(cfg, xi):
        with pytest.raises(IndexError):
            fwd(m, bad, xv, gpu)
    got = fwd(m, xi, xv, gpu)
    if got is not None:
        bar(got, cfg, params, xi, xv, route)
