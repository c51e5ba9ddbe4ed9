"""GPU: the row-lazy Adam step (include/dfwfm_lazy_adam.h).

The call alone: bit for bit the dense kernel (dfwfm_adam_step at the explicit step number) run on the touched rows
gathered into compact tensors, over the WHOLE table (untouched rows keep their bits), for every table shape, batch and
key pattern; the clamp; the QR kinds; the global step over consecutive calls (and torch.optim.Adam on the compacted
rows, tests/lazy_adam_ref.py, at the project's Adam bar); graph capture; run-to-run identity.

The step: FusedTrainStep(lazy_table_adam=True) on train_cases.FUSED at B = 37 against the dense step where the two
semantics coincide (fresh moments, no weight decay), against the dense kernel on the touched rows of a twin's
gradients over three steps, and the invariants around it (zero table gradients, step_many, the atomic scatter, the
serving copy, fit(), data parallelism refused)."""
import ctypes

import numpy as np
import pytest
import torch

import lazy_adam_ref as ref
import train_cases as tc
from test_gpu_train import _sparse_step, build

pytestmark = pytest.mark.gpu

LR, WD, BETAS, EPS = 1e-3, 3e-7, (0.9, 0.999), 1e-8
SHAPES = [(1, 10), (7, 10), (7, 1), (5000, 10), (5000, 1)]


# ------------------------------------------------------------------------------------------------ the call alone
def _rand_table(rows, width, seed, gpu, key_range=None, kind=ref.PLAIN, c=0, column=0):
    """Random p, g (magnitudes 1e-8 .. 1), m, v >= 0 on the device, zero stamps."""
    r = np.random.default_rng(seed)
    p = r.standard_normal((rows, width)).astype(np.float32)
    g = (r.standard_normal((rows, width)) * 10.0 ** r.uniform(-8, 0, (rows, width))).astype(np.float32)
    m = (0.1 * r.standard_normal((rows, width))).astype(np.float32)
    v = (0.01 * r.random((rows, width))).astype(np.float32)
    t = {k: torch.from_numpy(a).to(gpu) for k, a in (("p", p), ("g", g), ("m", m), ("v", v))}
    t.update(stamp=torch.zeros(rows, dtype=torch.int32, device=gpu), rows=rows, width=width,
             key_range=rows if key_range is None else key_range, kind=kind, c=c, column=column)
    return t


def _clone(t):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in t.items()}


def _new_state(gpu):
    from xsdeepfwfm_deprecated_amd import _lib
    return torch.zeros(_lib.ADAM_STATE_BYTES // 8, dtype=torch.int64, device=gpu)


def _lazy_call(tabs, xi, batch, state, gpu, wd=WD):
    from xsdeepfwfm_deprecated_amd import _lib
    arr = (_lib.dfwfm_lazy_adam_table * max(len(tabs), 1))()
    for i, t in enumerate(tabs):
        arr[i] = _lib.dfwfm_lazy_adam_table(t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(),
                                            t["stamp"].data_ptr(), t["rows"], t["key_range"], t["c"], t["width"],
                                            t["column"], t["kind"], 0)
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    _lib.check(_lib.lib().dfwfm_lazy_adam_step_dev(arr, len(tabs), ctypes.c_void_p(xi.data_ptr()), xi.stride(0), batch,
                                                   LR, BETAS[0], BETAS[1], EPS, wd,
                                                   ctypes.c_void_p(state.data_ptr()), st), "dfwfm_lazy_adam_step_dev")


def _dense_on_rows(t, keys, step, gpu, wd=WD):
    """Expected table after the lazy step `step` for `keys` (a numpy column): the touched rows gathered into compact
    tensors, the existing dense kernel (dfwfm_adam_step, explicit step number) run on them, scattered back.  t is
    updated in place (its grad zeroed on the touched rows); returns the touched rows."""
    from xsdeepfwfm_deprecated_amd import engine
    rows = ref.touched_rows(keys, t["key_range"], t["kind"], max(t["c"], 1))
    idx = torch.from_numpy(rows).to(gpu)
    pc, gc, mc, vc = (t[k][idx].contiguous() for k in "pgmv")
    engine.adam_step([(pc, gc, mc, vc)], LR, BETAS[0], BETAS[1], EPS, wd, step, gpu)
    t["p"][idx], t["m"][idx], t["v"][idx] = pc, mc, vc
    t["g"][idx] = 0.0
    return rows


def _same(got, want, what=""):
    for k in "pgmv":
        assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), (what, k)


def _keys(pattern, rows, batch, seed):
    if pattern == "equal":
        return np.full(batch, min(3, rows - 1), np.int64)
    if pattern == "distinct":  # all distinct where the table has the rows for it
        return (np.arange(batch, dtype=np.int64) * 7 + 2) % rows if rows % 7 else np.arange(batch, dtype=np.int64) % rows
    return np.random.default_rng(seed).integers(0, rows, batch)


@pytest.mark.parametrize("pattern", ["equal", "distinct", "random"])
@pytest.mark.parametrize("batch", [1, 37, 4133])
def test_lazy_call_equals_dense_kernel_on_touched_rows(gpu, batch, pattern):
    """The five table shapes as one call's table list, one xi column each.  param / exp_avg / exp_avg_sq array_equal
    over the whole table, grad zero on the touched rows and unchanged elsewhere, the counter advanced once."""
    tabs = [_rand_table(r, w, 10 + i, gpu, column=i) for i, (r, w) in enumerate(SHAPES)]
    xi = np.stack([_keys(pattern, r, batch, 50 + i) for i, (r, w) in enumerate(SHAPES)], axis=1)
    want = [_clone(t) for t in tabs]
    state = _new_state(gpu)
    _lazy_call(tabs, torch.from_numpy(xi).to(gpu), batch, state, gpu)
    torch.cuda.synchronize()
    assert int(state[0].item()) == 1
    for i, (t, w) in enumerate(zip(tabs, want)):
        before = w["g"].clone()
        rows = _dense_on_rows(w, xi[:, i], 1, gpu)
        _same(t, w, SHAPES[i])
        if pattern == "distinct":
            assert len(rows) == min(batch, t["rows"])
        if pattern == "equal":
            assert len(rows) == 1
        rest = np.setdiff1d(np.arange(t["rows"]), rows)
        assert np.array_equal(t["g"].cpu().numpy()[rest], before.cpu().numpy()[rest])
        assert not t["g"].cpu().numpy()[rows].any()
        assert np.array_equal(np.flatnonzero(t["stamp"].cpu().numpy()), rows)  # claimed exactly the touched rows


def test_lazy_call_over_more_tables_than_one_launch_takes(gpu):
    """60 tables (a launch takes 54): two launches, one counter advance, every table updated."""
    tabs = [_rand_table(5 + i % 3, 1 + 9 * (i % 2), 100 + i, gpu, column=i % 4) for i in range(60)]
    xi = np.random.default_rng(9).integers(0, 5, (6, 4))
    want = [_clone(t) for t in tabs]
    state = _new_state(gpu)
    _lazy_call(tabs, torch.from_numpy(xi).to(gpu), 6, state, gpu)
    torch.cuda.synchronize()
    assert int(state[0].item()) == 1
    for t, w in zip(tabs, want):
        _dense_on_rows(w, xi[:, t["column"]], 1, gpu)
        _same(t, w)


def test_lazy_call_empty_batch_or_list_advances_the_counter_only(gpu):
    t = _rand_table(7, 10, 1, gpu)
    want = _clone(t)
    xi = torch.zeros(4, 1, dtype=torch.int64, device=gpu)
    state = _new_state(gpu)
    _lazy_call([t], xi, 0, state, gpu)
    _lazy_call([], xi, 4, state, gpu)
    torch.cuda.synchronize()
    assert int(state[0].item()) == 2
    _same(t, want)


def test_out_of_range_keys_hit_row_zero_only(gpu):
    for rows, width in ((7, 10), (7, 1)):
        t = _rand_table(rows, width, 3, gpu)
        want = _clone(t)
        keys = np.array([-1, rows, -(2 ** 40), 2 ** 40], np.int64)
        _lazy_call([t], torch.from_numpy(keys[:, None].copy()).to(gpu), 4, _new_state(gpu), gpu)
        assert _dense_on_rows(want, keys, 1, gpu).tolist() == [0]
        _same(t, want)
        assert not np.array_equal(t["p"][0].cpu().numpy(), _rand_table(rows, width, 3, gpu)["p"][0].cpu().numpy())


def test_qr_quotient_and_remainder_rows(gpu):
    """c = 4 on a 23-key range: quotient rows key / 4 (6 rows), remainder rows key % 4 (4 rows); key 23 clamps to 0."""
    keys = np.array([22, 5, 23, 9, 5], np.int64)
    q = _rand_table(6, 10, 5, gpu, key_range=23, kind=ref.QUOTIENT, c=4)
    r = _rand_table(4, 10, 6, gpu, key_range=23, kind=ref.REMAINDER, c=4)
    q1 = _rand_table(6, 1, 7, gpu, key_range=23, kind=ref.QUOTIENT, c=4)
    r1 = _rand_table(4, 1, 8, gpu, key_range=23, kind=ref.REMAINDER, c=4)
    tabs = [q, r, q1, r1]
    want = [_clone(t) for t in tabs]
    _lazy_call(tabs, torch.from_numpy(keys[:, None].copy()).to(gpu), 5, _new_state(gpu), gpu)
    touched = [_dense_on_rows(w, keys, 1, gpu).tolist() for w in want]
    assert touched == [[0, 1, 2, 5], [0, 1, 2], [0, 1, 2, 5], [0, 1, 2]]
    for t, w in zip(tabs, want):
        _same(t, w)


def test_three_calls_use_the_global_step(gpu):
    """Keys differ per call; row 3 is touched in calls 1 and 3 only: it equals the compact dense kernel run at steps 1
    and 3 (and nothing at step 2), and torch.optim.Adam on the compacted rows at the project's Adam bar."""
    t = _rand_table(50, 10, 21, gpu)
    t["m"].zero_()
    t["v"].zero_()
    want = _clone(t)
    host = {k: t[k].cpu().numpy() for k in "pgmv"}
    p0 = host["p"].copy()
    calls = [np.array([3, 7, 7, 9], np.int64), np.array([1, 2], np.int64), np.array([3, 4, 60], np.int64)]
    grads = [_rand_table(50, 10, 30 + s, gpu)["g"] for s in range(3)]
    state = _new_state(gpu)
    row3 = []
    for s, (keys, g) in enumerate(zip(calls, grads), 1):
        for x in (t, want):
            x["g"].copy_(g)
        _lazy_call([t], torch.from_numpy(keys[:, None].copy()).to(gpu), len(keys), state, gpu)
        _dense_on_rows(want, keys, s, gpu)
        _same(t, want, s)
        hp, hg, hm, hv = ref.lazy_adam_ref(host["p"], g.cpu().numpy(), host["m"], host["v"], keys, 50, s, lr=LR,
                                           betas=BETAS, eps=EPS, weight_decay=WD)
        host.update(p=hp, m=hm, v=hv)
        row3.append(t["p"][3].cpu().numpy().copy())
    torch.cuda.synchronize()
    assert int(state[0].item()) == 3
    assert np.array_equal(row3[0], row3[1]) and not np.array_equal(row3[1], row3[2])
    # row 3 alone through the dense kernel at steps 1 and 3
    from xsdeepfwfm_deprecated_amd import engine
    pc = torch.from_numpy(p0[[3]]).to(gpu)
    mc, vc = torch.zeros_like(pc), torch.zeros_like(pc)
    for s in (1, 3):
        engine.adam_step([(pc, grads[s - 1][[3]].contiguous(), mc, vc)], LR, BETAS[0], BETAS[1], EPS, WD, s, gpu)
    assert np.array_equal(t["p"][[3]].cpu().numpy(), pc.cpu().numpy())
    assert np.array_equal(t["m"][[3]].cpu().numpy(), mc.cpu().numpy())
    # torch.optim.Adam on the compacted rows: test_gpu_train.test_adam_matches_torch_over_steps' bar
    np.testing.assert_allclose(t["p"].cpu().numpy(), host["p"], rtol=2.4e-7, atol=2e-9)
    untouched = np.setdiff1d(np.arange(50), [0, 1, 2, 3, 4, 7, 9])
    assert np.array_equal(t["p"].cpu().numpy()[untouched], p0[untouched])


def _three_calls(gpu, graph):
    tabs = [_rand_table(200, 10, 41, gpu, column=0), _rand_table(200, 1, 42, gpu, column=1)]
    rng = np.random.default_rng(43)
    keys = [torch.from_numpy(rng.integers(0, 200, (37, 2))).to(gpu) for _ in range(4)]
    grads = [[_rand_table(200, w, 60 + 2 * s + i, gpu)["g"] for i, w in enumerate((10, 1))] for s in range(4)]
    xi = keys[0].clone()
    state = _new_state(gpu)
    _lazy_call(tabs, xi, 37, state, gpu)  # one eager call first
    g = None
    if graph:
        s = torch.cuda.Stream(gpu)
        s.wait_stream(torch.cuda.current_stream(gpu))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                _lazy_call(tabs, xi, 37, state, gpu)
        torch.cuda.current_stream(gpu).wait_stream(s)
    for k in range(1, 4):
        xi.copy_(keys[k])
        for t, gg in zip(tabs, grads[k]):
            t["g"].copy_(gg)
        if graph:
            g.replay()
        else:
            _lazy_call(tabs, xi, 37, state, gpu)
    torch.cuda.synchronize()
    return tabs, int(state[0].item())


def test_captured_call_replays_equal_eager_calls(gpu):
    """A capture records and does not run: three replays with the key buffer (and the gradients) rewritten between them
    equal three eager calls, counter included."""
    eager, n0 = _three_calls(gpu, False)
    replay, n1 = _three_calls(gpu, True)
    assert n0 == n1 == 4
    for a, b in zip(eager, replay):
        _same(b, a)
        assert np.array_equal(a["stamp"].cpu().numpy(), b["stamp"].cpu().numpy())


def test_two_runs_from_the_same_start_are_identical(gpu):
    res = []
    for _ in range(2):
        t = _rand_table(300, 10, 77, gpu)
        xi = torch.from_numpy(np.random.default_rng(5).integers(0, 300, (4133, 1))).to(gpu)
        _lazy_call([t], xi, 4133, _new_state(gpu), gpu)
        res.append(t)
    _same(res[0], res[1])


# ---------------------------------------------------------------------------------------------------- the step
def _trainer(name, gpu, lazy, B=37, wd=0.0, det=True, **kw):
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, *_ = tc.case(name)  # (the weights do not depend on the case's batch)
    m = build(cfg, params, gpu, is_deep_dropout=False)
    t = FusedTrainStep(m, B, lr=LR, weight_decay=wd, deterministic=det, lazy_table_adam=lazy, **kw)
    t.seed = 12345
    return m, t


def _dev(gpu, *arrs):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrs)


def _snapshot(m, t):
    d = {k: p.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    d["/exp_avg"] = t.exp_avg.cpu().numpy().copy()
    d["/exp_avg_sq"] = t.exp_avg_sq.cpu().numpy().copy()
    return d


@pytest.mark.parametrize("name,B", [(n, 37) for n in tc.FUSED] + [("fm_deep", 4133)])
def test_one_lazy_step_equals_dense_step_from_fresh_moments(gpu, name, B):
    """weight_decay = 0 and zero moments: the dense Adam leaves an untouched row's bits alone (m = v = 0 -> the
    update is -lr * 0 / eps), so the two semantics coincide and every tensor and moment is array_equal.  Pins the
    gradient path (the table region without its fill) and the table offsets.  B = 4133: two scatter passes."""
    cfg, params, xi, xv, y = tc.case(name, B)
    snaps = []
    for lazy in (False, True):
        m, t = _trainer(name, gpu, lazy, B=B)
        assert t.lazy is (lazy and name != "allnum")  # no categorical table: the switch is a no-op
        t.step(*_dev(gpu, xi, xv, y))
        torch.cuda.synchronize()
        if t.n_tables:
            assert bool(t.grad[:t.n_tables].any()) is (not t.lazy)  # the lazy step leaves the tables' gradients zero
        snaps.append(_snapshot(m, t))
        t.close()
    assert any(not np.array_equal(params[k], snaps[1][k]) for k in params)
    for k in snaps[0]:
        assert np.array_equal(snaps[0][k], snaps[1][k]), k


def _table_info(m, t):
    """[(name, parameter, (column, key_range, kind, c))] of the categorical tables in the trainer's order."""
    names = {id(p): k for k, p in m.named_parameters()}
    return [(names[id(p)], p, (int(d.column), int(d.key_range), int(d.kind), int(d.c)))
            for p, d in zip(t.params[:t.n_cat], t.lazy_tables)]


@pytest.mark.parametrize("name", [n for n in tc.FUSED if n != "allnum"])
def test_three_lazy_steps_equal_dense_kernel_on_touched_rows(gpu, name):
    """Three steps on three batches, weight_decay 3e-7.  Before each step a twin gets the lazy model's parameters and
    runs dfwfm_train_forward + dfwfm_backward (deterministic) for the step's dense table gradients; the expected tables
    and moments are dfwfm_adam_step at that step number on the compacted touched rows.  A dense trainer holding the
    same parameters, moments and counters runs the same batch: every non-table tensor equals its result.  After every
    lazy step the tables' region of the gradient buffer is all zero."""
    from xsdeepfwfm_deprecated_amd import engine
    B, K = 37, 3
    cfg, params, xi, xv, y = tc.case(name, B * K)
    bats = [(xi[k * B:(k + 1) * B], xv[k * B:(k + 1) * B], y[k * B:(k + 1) * B]) for k in range(K)]
    m, t = _trainer(name, gpu, True, wd=WD)
    md, td = _trainer(name, gpu, False, wd=WD)
    twin = build(cfg, params, gpu, is_deep_dropout=False)
    info = _table_info(m, t)
    table_names = {n for n, _, _ in info}
    exp_m = {n: torch.zeros_like(p) for n, p, _ in info}
    exp_v = {n: torch.zeros_like(p) for n, p, _ in info}
    for s, (xb, vb, yb) in enumerate(bats, 1):
        with torch.no_grad():
            for other in (twin, md):
                for (_, a), (_, b) in zip(m.named_parameters(), other.named_parameters()):
                    b.copy_(a)
            td.exp_avg.copy_(t.exp_avg)
            td.exp_avg_sq.copy_(t.exp_avg_sq)
        twin._sync_engine(gpu).set_deterministic(True)
        grads, _, _ = _sparse_step(twin, gpu, xb, vb, yb, sparse=False)
        exp_p = {n: p.detach().clone() for n, p, _ in info}
        t.step(*_dev(gpu, xb, vb, yb))
        td.step(*_dev(gpu, xb, vb, yb))
        torch.cuda.synchronize()
        assert t.graphs is not None or s == 1  # steps 2 and 3 are graph replays
        assert not bool(t.grad[:t.n_tables].any()), s
        assert int(t.state_t[0].item()) == int(t.state[0].item()) == s
        for n, p, (col, key_range, kind, c) in info:
            rows = torch.from_numpy(ref.touched_rows(xb[:, col], key_range, kind, max(c, 1))).to(gpu)
            g = torch.from_numpy(grads[n]).to(gpu)
            assert not grads[n][np.setdiff1d(np.arange(p.shape[0]), rows.cpu().numpy())].any(), n
            pc, gc, mc, vc = (a[rows].contiguous() for a in (exp_p[n], g, exp_m[n], exp_v[n]))
            engine.adam_step([(pc, gc, mc, vc)], LR, BETAS[0], BETAS[1], EPS, WD, s, gpu)
            exp_p[n][rows], exp_m[n][rows], exp_v[n][rows] = pc, mc, vc
            off = (p.grad.data_ptr() - t.grad.data_ptr()) // 4
            assert np.array_equal(p.detach().cpu().numpy(), exp_p[n].cpu().numpy()), (n, s)
            assert np.array_equal(t.exp_avg[off:off + p.numel()].cpu().numpy(), exp_m[n].reshape(-1).cpu().numpy()), (n, s)
            assert np.array_equal(t.exp_avg_sq[off:off + p.numel()].cpu().numpy(),
                                  exp_v[n].reshape(-1).cpu().numpy()), (n, s)
        for (k, a), (_, b) in zip(m.named_parameters(), md.named_parameters()):
            if k not in table_names:
                assert np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy()), (k, s)
        assert np.array_equal(t.exp_avg[t.n_tables:].cpu().numpy(), td.exp_avg[td.n_tables:].cpu().numpy()), s
    t.close()
    td.close()


def test_step_many_equals_single_steps_under_the_switch(gpu):
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    B, K = 37, 3
    cfg, params, xi, xv, y = tc.case("qr_add", B * (K + 1))
    bat = [_dev(gpu, xi[k * B:(k + 1) * B], xv[k * B:(k + 1) * B], y[k * B:(k + 1) * B]) for k in range(K + 1)]
    res = []
    for many in (False, True):
        m = build(cfg, params, gpu, is_deep_dropout=False)
        t = FusedTrainStep(m, B, lr=LR, weight_decay=WD, resident_inputs=True, deterministic=True,
                           lazy_table_adam=True)
        t.seed = 12345
        t.step(*bat[0])
        if many:
            t.step_many(bat[1:])
            assert any(k[0] == "many" for k in t._many_sets)
        else:
            for b in bat[1:]:
                t.step(*b)
        torch.cuda.synchronize()
        assert t.steps == K + 1 and not bool(t.grad[:t.n_tables].any())
        res.append(_snapshot(m, t))
        t.close()
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k


def test_atomic_scatter_lazy_step_moves_touched_rows_only(gpu):
    """deterministic=False (float-atomic scatter): untouched rows bit-unchanged; after step 1 every touched element
    moved by at most lr (1 + 1e-3) -- Adam's first update is bounded by lr, weight decay far below the margin."""
    cfg, params, xi, xv, y = tc.case("fm_deep")
    m, t = _trainer("fm_deep", gpu, True, wd=WD, det=False)
    info = _table_info(m, t)
    t.step(*_dev(gpu, xi, xv, y))
    torch.cuda.synchronize()
    moved = 0
    for n, p, (col, key_range, kind, c) in info:
        rows = ref.touched_rows(xi[:, col], key_range, kind, max(c, 1))
        rest = np.setdiff1d(np.arange(p.shape[0]), rows)
        new = p.detach().cpu().numpy()
        assert np.array_equal(new[rest], params[n][rest]), n
        d = np.abs(new[rows].astype(np.float64) - params[n][rows])
        assert d.max() <= LR * (1 + 1e-3), (n, d.max())
        moved += int((d > 0).sum())
    assert moved > 0 and not bool(t.grad[:t.n_tables].any())
    t.close()


def test_serving_copy_is_refreshed_after_lazy_steps(gpu):
    """As test_gpu_batches.test_packed_tables_after_fused_training_steps for the dense step: the eval forward over the
    serving copy (pack_tables, the default) equals the plain-table forward bit for bit after lazy steps."""
    cfg, params, xi, xv, y = tc.case("fm_deep")
    m, t = _trainer("fm_deep", gpu, True, wd=WD)
    dev = _dev(gpu, xi, xv, y)
    m.eval()
    with torch.no_grad():
        before = m(dev[0], dev[1]).cpu().numpy()  # packs
    m.train()
    for _ in range(2):
        t.step(*dev)
    t.close()
    m.eval()
    with torch.no_grad():
        assert m.pack_tables is True
        packed = m(dev[0], dev[1]).cpu().numpy()
        m.pack_tables = False
        plain = m(dev[0], dev[1]).cpu().numpy()
    assert not np.array_equal(packed, before)
    assert np.array_equal(packed, plain)


def test_fit_with_lazy_table_adam_learns(gpu, caplog):
    """fit() end to end under the switch on a small synthetic set: the last logged training loss is below the first."""
    import logging
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = [1] * 13 + [50, 300, 7, 1000, 20, 5, 64, 9, 100, 3, 11, 17, 250, 4, 6, 30, 8, 2, 40, 12, 90, 5, 15,
                        300, 7, 60]
    xi, xv = synth.synth_inputs(sizes, 13, 4096, seed=5)
    logit = ((xi[:, 0] % 7) - 3) * 0.6 + (xv[:, 0] > 30) * 1.0 - 0.5
    y = (np.random.default_rng(1).random(4096) < 1 / (1 + np.exp(-logit))).astype(np.float32)
    log = logging.getLogger("test_lazy_fit")
    log.setLevel(logging.INFO)
    m = DeepFMs(field_size=39, feature_sizes=sizes, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1, n_epochs=3,
                batch_size=256, learning_rate=1e-2, weight_decay=3e-7, h_depth=2, deep_nodes=64, logger=log).to(gpu)
    m.lazy_table_adam = True
    with caplog.at_level(logging.INFO, logger="test_lazy_fit"):
        m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    losses = [float(r.getMessage().split("loss:")[1].split()[0]) for r in caplog.records
              if r.getMessage().startswith("Training [")]
    assert len(losses) == 3 and losses[-1] < losses[0], losses


def test_data_parallel_with_the_switch_is_refused(gpu):
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, *_ = tc.case("fm_deep")
    m = build(cfg, params, gpu, is_deep_dropout=False)

    class FakeDist:  # refused before it is asked anything
        pass
    with pytest.raises(NotImplementedError, match="lazy_table_adam"):
        FusedTrainStep(m, 37, dist=FakeDist(), lazy_table_adam=True)
