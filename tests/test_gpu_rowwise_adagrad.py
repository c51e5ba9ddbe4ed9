"""GPU: the row-wise Adagrad step (include/dfwfm_rowwise_adagrad.h).  Every comparison is bit for bit.

The call alone: the kernel against the host function dfwfm_rowwise_adagrad_row_ref applied to the touched rows of a
host copy (tests/rowwise_adagrad_ref.py), over the WHOLE table -- untouched rows, their state and their gradients keep
their bits, touched gradient rows are zero --, for every table shape (widths 1, 4, 10, 16, 17 and 33: the owning lane
alone, one and two registers per lane, the re-read pass), batch, key pattern and weight decay; the clamp; the QR kinds;
two columns sharing a table; a list longer than a launch; the global step and the stamps over consecutive calls; the
empty call; the scheduled entry; graph capture; run-to-run identity; and the corner in which the element-wise lazy
Adagrad kernel (dfwfm_lazy_optim_step_dev) gives the same bits.

The step: FusedTrainStep(optimizer="adag", rowwise_tables=True) on train_cases.FUSED at B = 37.  The tables and
row_state against the host function on the touched rows of a twin's table gradients over three steps; every other
tensor and opt_state against a FusedTrainStep(optimizer="adag", lazy_tables=True) twin that is handed the same
parameters and state before each step (so the tables' different learning does not enter); and the invariants around
it (zero table gradients, step_many, lr_schedule, the atomic scatter, the serving copy, the state sizes, fit(), off
means off)."""
import ctypes

import numpy as np
import pytest
import torch

import optim_ref
import rowwise_adagrad_ref as ref
import train_cases as tc
from test_gpu_train import _sparse_step, build

pytestmark = pytest.mark.gpu

LR, WD, EPS = 1e-3, 3e-7, 1e-10
SHAPES = [(1, 10), (7, 10), (7, 1), (5000, 10), (5000, 1), (7, 4), (7, 16), (7, 17), (7, 33)]
K_LIST = 60  # tables per launch (csrc/dfwfm_lazy_optim.h: the launch arguments the row-wise kernel shares)


def _stream(gpu):
    return ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


# ------------------------------------------------------------------------------------------------ the call alone
def _rand_table(rows, width, seed, gpu, key_range=None, kind=ref.PLAIN, c=0, column=0):
    """Random p, g (magnitudes 1e-8 .. 1) and accumulators as after earlier steps (>= 0, every fourth row still zero)
    on the device, zero stamps."""
    r = np.random.default_rng(seed)
    p = r.standard_normal((rows, width)).astype(np.float32)
    g = (r.standard_normal((rows, width)) * 10.0 ** r.uniform(-8, 0, (rows, width))).astype(np.float32)
    s = np.abs(0.1 * r.standard_normal(rows)).astype(np.float32)
    s[::4] = 0
    t = {k: torch.from_numpy(v).to(gpu) for k, v in (("p", p), ("g", g), ("s", s))}
    t.update(stamp=torch.zeros(rows, dtype=torch.int32, device=gpu), rows=rows, width=width,
             key_range=rows if key_range is None else key_range, kind=kind, c=c, column=column)
    return t


def _clone(t):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in t.items()}


def _new_state(gpu, step_before=0):
    from xsdeepfwfm_deprecated_amd import _lib
    st = torch.zeros(_lib.ADAM_STATE_BYTES // 8, dtype=torch.int64, device=gpu)
    st[0] = step_before
    return st


def _call(tabs, xi, batch, state, gpu, wd=WD, lr=LR, eps=EPS, sched=None):
    from xsdeepfwfm_deprecated_amd import _lib
    arr = (_lib.dfwfm_rowwise_table * max(len(tabs), 1))()
    for i, t in enumerate(tabs):
        arr[i] = _lib.dfwfm_rowwise_table(t["p"].data_ptr(), t["g"].data_ptr(), t["s"].data_ptr(),
                                          t["stamp"].data_ptr(), t["rows"], t["key_range"], t["c"], t["width"],
                                          t["column"], t["kind"], 0)
    h = ref.hyper(lr, wd, eps)
    if sched is not None:
        _lib.check(_lib.lib().dfwfm_rowwise_adagrad_step_dev_sched(
            arr, len(tabs), ctypes.c_void_p(xi.data_ptr()), xi.stride(0), batch, ctypes.byref(h),
            ctypes.c_void_p(sched.data_ptr()), ctypes.c_void_p(state.data_ptr()), _stream(gpu)),
            "dfwfm_rowwise_adagrad_step_dev_sched")
        return
    _lib.check(_lib.lib().dfwfm_rowwise_adagrad_step_dev(
        arr, len(tabs), ctypes.c_void_p(xi.data_ptr()), xi.stride(0), batch, ctypes.byref(h),
        ctypes.c_void_p(state.data_ptr()), _stream(gpu)), "dfwfm_rowwise_adagrad_step_dev")


def _host(t):
    return {k: t[k].cpu().numpy() for k in "pgs"}


def _want(before, t, keys, wd=WD, lr=LR, eps=EPS):
    """The expected table by dfwfm_rowwise_adagrad_row_ref on the touched rows of the host copy `before`."""
    p, g, s = ref.rowwise_ref(before["p"], before["g"], before["s"], keys, t["key_range"], t["kind"], max(t["c"], 1),
                              lr=lr, weight_decay=wd, eps=eps, elem="lib")
    return {"p": p, "g": g, "s": s}


def _same(got, want, what=""):
    for k in "pgs":
        a = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        b = want[k].cpu().numpy() if torch.is_tensor(want[k]) else want[k]
        assert optim_ref.same_bits(a, b), (what, k)


def _touched(t, keys):
    return ref.touched_rows(keys, t["key_range"], t["kind"], max(t["c"], 1))


def _keys(pattern, rows, batch, seed):
    if pattern == "equal":
        return np.full(batch, min(3, rows - 1), np.int64)
    if pattern == "distinct":  # all distinct where the table has the rows for it
        i = np.arange(batch, dtype=np.int64)
        return (i * 7 + 2) % rows if rows % 7 else i % rows
    if pattern == "clamp":  # keys below 0 and at or past the key range (both count as key 0) among valid ones
        k = np.random.default_rng(seed).integers(-rows - 2, 2 * rows + 2, batch)
        k[:2] = (-1, rows)[:min(batch, 2)]
        return k
    return np.random.default_rng(seed).integers(0, rows, batch)


@pytest.mark.parametrize("pattern", ["equal", "distinct", "random", "clamp"])
@pytest.mark.parametrize("batch", [1, 37, 256, 257, 1000])
def test_call_equals_host_function_on_touched_rows(gpu, batch, pattern):
    """The nine table shapes as one call's table list, one xi column each, with weight_decay 0 and 3e-7, at step 2 (the
    counter preset to 1).  param / state / grad bit for bit over the whole table against dfwfm_rowwise_adagrad_row_ref
    on the touched rows, stamps non-zero exactly on the touched rows, the counter advanced once."""
    xi = np.stack([_keys(pattern, r, batch, 50 + i) for i, (r, w) in enumerate(SHAPES)], axis=1)
    changed = 0
    for wd in (0.0, WD):
        tabs = [_rand_table(r, w, 10 + i, gpu, column=i) for i, (r, w) in enumerate(SHAPES)]
        before = [_host(t) for t in tabs]
        state = _new_state(gpu, 1)
        _call(tabs, torch.from_numpy(xi).to(gpu), batch, state, gpu, wd=wd)
        torch.cuda.synchronize()
        assert int(state[0].item()) == 2 and int(state[4].item()) >> 32 == 0  # (the ticket is 0 again)
        for i, t in enumerate(tabs):
            rows = _touched(t, xi[:, i])
            _same(t, _want(before[i], t, xi[:, i], wd=wd), (SHAPES[i], wd))
            if pattern == "distinct":
                assert len(rows) == min(batch, t["rows"])
            if pattern == "equal":
                assert len(rows) == 1
            if pattern == "clamp":
                assert 0 in rows
            rest = np.setdiff1d(np.arange(t["rows"]), rows)
            got = _host(t)
            assert np.array_equal(got["g"][rest], before[i]["g"][rest]) and not got["g"][rows].any()
            assert np.array_equal(got["s"][rest], before[i]["s"][rest])
            assert np.all(got["s"][rows] >= before[i]["s"][rows])
            assert np.array_equal(np.flatnonzero(t["stamp"].cpu().numpy()), rows)  # claimed exactly the touched rows
            changed += int(not np.array_equal(got["p"][rows], before[i]["p"][rows]))
    assert changed >= 9


@pytest.mark.parametrize("c", [1, 7, 5000])
def test_qr_quotient_and_remainder_pair(gpu, c):
    """A QR field of 5000 keys with c collisions: quotient rows key / c, remainder rows key % c, in widths 10 and 1;
    keys outside [0, 5000) clamp to key 0."""
    n, batch = 5000, 257
    keys = np.random.default_rng(c).integers(0, n, batch)
    keys[:3] = (n, -7, n - 1)
    qrows, rrows = (n - 1) // c + 1, min(c, n)
    tabs = [_rand_table(qrows, 10, 5, gpu, key_range=n, kind=ref.QUOTIENT, c=c),
            _rand_table(rrows, 10, 6, gpu, key_range=n, kind=ref.REMAINDER, c=c),
            _rand_table(qrows, 1, 7, gpu, key_range=n, kind=ref.QUOTIENT, c=c),
            _rand_table(rrows, 1, 8, gpu, key_range=n, kind=ref.REMAINDER, c=c)]
    before = [_host(t) for t in tabs]
    _call(tabs, torch.from_numpy(keys[:, None].copy()).to(gpu), batch, _new_state(gpu, 4), gpu)
    torch.cuda.synchronize()
    for t, b in zip(tabs, before):
        rows = _touched(t, keys)
        assert 0 in rows and (len(rows) == 1) is (t["rows"] == 1)
        _same(t, _want(b, t, keys), (c, t["kind"], t["width"]))
        assert np.array_equal(np.flatnonzero(t["stamp"].cpu().numpy()), rows)


def test_two_columns_sharing_one_table_and_its_stamps(gpu):
    """A table listed twice (columns 0 and 1) with one stamp array: its rows are updated once for the union of the
    columns' keys."""
    for rows, width in ((300, 10), (300, 1)):
        t = _rand_table(rows, width, 3, gpu)
        before = _host(t)
        xi = np.random.default_rng(4).integers(0, rows, (257, 2))
        xi[:40, 1] = xi[:40, 0]  # rows both columns touch
        second = dict(t, column=1)
        _call([t, second], torch.from_numpy(xi).to(gpu), 257, _new_state(gpu), gpu)
        torch.cuda.synchronize()
        union = xi.reshape(-1)
        assert len(_touched(t, union)) > max(len(_touched(t, xi[:, 0])), len(_touched(t, xi[:, 1])))
        _same(t, _want(before, t, union), (rows, width))


def test_call_over_one_more_table_than_a_launch_takes(gpu):
    """61 tables of 3 rows (a launch takes 60): two launches, one counter advance, every table updated."""
    n = K_LIST + 1
    tabs = [_rand_table(3, (10, 1, 17)[i % 3], 100 + i, gpu, column=i % 4) for i in range(n)]
    xi = np.random.default_rng(9).integers(0, 3, (6, 4))
    before = [_host(t) for t in tabs]
    state = _new_state(gpu)
    _call(tabs, torch.from_numpy(xi).to(gpu), 6, state, gpu)
    torch.cuda.synchronize()
    assert int(state[0].item()) == 1
    for t, b in zip(tabs, before):
        _same(t, _want(b, t, xi[:, t["column"]]))
        assert t["stamp"].any()


def test_empty_batch_or_list_advances_the_counter_only(gpu):
    t = _rand_table(7, 10, 1, gpu)
    want = _clone(t)
    xi = torch.zeros(4, 1, dtype=torch.int64, device=gpu)
    state = _new_state(gpu)
    _call([t], xi, 0, state, gpu)
    _call([], xi, 4, state, gpu)
    torch.cuda.synchronize()
    assert int(state[0].item()) == 2
    _same(t, want)
    assert not t["stamp"].any()


@pytest.mark.parametrize("before", [0, 6], ids=["steps-1-2-3", "steps-7-8-9"])
@pytest.mark.parametrize("width", [10, 1, 33])
def test_three_calls_on_one_state_block(gpu, width, before):
    """Keys differ per call; row 3 is touched in calls 1 and 3 only, row 4 in call 3 only.  The stamps of a step do
    not hide a row from the next one, a call that does not touch row 3 leaves it (and its accumulator) alone, and the
    third call starts from what the first left."""
    t = _rand_table(50, width, 21, gpu)
    calls = [np.array([3, 7, 7, 9], np.int64), np.array([1, 2], np.int64), np.array([3, 4, 60], np.int64)]
    grads = [_rand_table(50, width, 30 + s, gpu)["g"] for s in range(3)]
    for g in grads:
        g[3] = 0.5  # (large enough to move row 3 and its accumulator at any width)
    state = _new_state(gpu, before)
    row3 = []
    for k, (keys, g) in enumerate(zip(calls, grads)):
        t["g"].copy_(g)
        host = _host(t)
        _call([t], torch.from_numpy(keys[:, None].copy()).to(gpu), len(keys), state, gpu)
        _same(t, _want(host, t, keys), before + k + 1)
        row3.append((t["p"][3].cpu().numpy().copy(), float(t["s"][3].item())))
    torch.cuda.synchronize()
    assert int(state[0].item()) == before + 3
    assert np.array_equal(row3[0][0], row3[1][0]) and not np.array_equal(row3[1][0], row3[2][0])
    assert row3[0][1] == row3[1][1] and row3[2][1] > row3[1][1]
    stamp = t["stamp"].cpu().numpy()
    assert stamp[3] == stamp[4] == stamp[0] == before + 3 and stamp[7] == before + 1 and stamp[1] == before + 2


KNOTS = [(1, 1e-4), (5, 1e-3), (9, 2e-4)]


@pytest.mark.parametrize("s", [5, 3, 7, 12], ids=["at-a-knot", "mid-ramp", "mid-descent", "past-the-last-knot"])
def test_scheduled_entry_equals_the_unscheduled_one_at_the_evaluated_rate(gpu, s):
    """The scheduled call at step s equals, bit for bit, the unscheduled one with lr = dfwfm_lr_schedule_eval(s), and
    the host function at that rate; hyper->lr is not read (a NaN there is accepted)."""
    from xsdeepfwfm_deprecated_amd import _lib
    block = torch.zeros(_lib.LR_SCHEDULE_BYTES // 8, dtype=torch.int64, device=gpu)
    arr, n = _lib.lr_knots(KNOTS)
    _lib.check(_lib.lib().dfwfm_lr_schedule_write(ctypes.c_void_p(block.data_ptr()), arr, n, _stream(gpu)),
               "dfwfm_lr_schedule_write")
    xi = torch.from_numpy(np.random.default_rng(3).integers(0, 300, (37, 3))).to(gpu)
    lr = _lib.lr_schedule_eval(KNOTS, s)
    assert (lr in (1e-4, 1e-3, 2e-4)) is (s in (5, 12))
    res = []
    for sched in (None, block):
        tabs = [_rand_table(300, w, 41 + i, gpu, column=i) for i, w in enumerate((10, 1, 33))]
        before = [_host(t) for t in tabs]
        state = _new_state(gpu, s - 1)
        _call(tabs, xi, 37, state, gpu, lr=lr if sched is None else float("nan"), sched=sched)
        torch.cuda.synchronize()
        assert int(state[0].item()) == s
        res.append(tabs)
    for i, (a, b) in enumerate(zip(*res)):
        _same(a, b, s)
        _same(b, _want(before[i], b, xi[:, i].cpu().numpy(), lr=lr), (s, "host function at the evaluated rate"))
        assert not np.isnan(b["p"].cpu().numpy()).any()


def _three_calls(gpu, graph):
    tabs = [_rand_table(200, w, 41 + i, gpu, column=i) for i, w in enumerate((10, 1, 17))]
    rng = np.random.default_rng(43)
    keys = [torch.from_numpy(rng.integers(0, 200, (37, 3))).to(gpu) for _ in range(3)]
    grads = [[_rand_table(200, w, 60 + 3 * s + i, gpu)["g"] for i, w in enumerate((10, 1, 17))] for s in range(3)]
    xi = keys[0].clone()
    state = _new_state(gpu)
    _call(tabs, xi, 37, state, gpu)  # one eager call first
    g = None
    if graph:
        s = torch.cuda.Stream(gpu)
        s.wait_stream(torch.cuda.current_stream(gpu))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                _call(tabs, xi, 37, state, gpu)
        torch.cuda.current_stream(gpu).wait_stream(s)
    for k in range(1, 3):
        xi.copy_(keys[k])
        for t, gg in zip(tabs, grads[k]):
            t["g"].copy_(gg)
        if graph:
            g.replay()
        else:
            _call(tabs, xi, 37, state, gpu)
    torch.cuda.synchronize()
    return tabs, int(state[0].item())


def test_captured_call_replays_equal_eager_calls(gpu):
    """A capture records and does not run: one eager call and two replays with the key buffer (and the gradients)
    rewritten between them equal three eager calls, counter and stamps included."""
    eager, n0 = _three_calls(gpu, False)
    replay, n1 = _three_calls(gpu, True)
    assert n0 == n1 == 3
    for a, b in zip(eager, replay):
        _same(b, a)
        assert np.array_equal(a["stamp"].cpu().numpy(), b["stamp"].cpu().numpy())


def test_two_runs_from_the_same_start_are_identical(gpu):
    res = []
    for _ in range(2):
        tabs = [_rand_table(300, w, 77 + i, gpu, column=i) for i, w in enumerate((10, 33))]
        xi = torch.from_numpy(np.random.default_rng(5).integers(0, 300, (1000, 2))).to(gpu)
        _call(tabs, xi, 1000, _new_state(gpu), gpu)
        res.append(tabs)
    for a, b in zip(*res):
        _same(a, b)


@pytest.mark.parametrize("width", [4, 8, 16])
def test_witness_corner_equals_the_elementwise_lazy_adagrad_kernel(gpu, width):
    """weight_decay 0, a power-of-two width, every gradient of a row +-2^k for the row's k: the kernel that already
    exists (dfwfm_lazy_optim_step_dev with kind Adagrad) on a twin table whose `sum` is the accumulator broadcast gives
    the same parameters, and a `sum` that is the new accumulator in every element."""
    from xsdeepfwfm_deprecated_amd import _lib
    rows, batch = 300, 257
    r = np.random.default_rng(width)
    t = _rand_table(rows, width, 9, gpu)
    k = r.integers(-12, 3, rows)
    g = (np.ldexp(1.0, k)[:, None] * r.choice([-1.0, 1.0], (rows, width))).astype(np.float32)
    t["g"].copy_(torch.from_numpy(g))
    twin = _clone(t)
    twin["s"] = t["s"][:, None].repeat(1, width).contiguous()
    xi = torch.from_numpy(r.integers(0, rows, (batch, 1))).to(gpu)
    _call([t], xi, batch, _new_state(gpu), gpu, wd=0.0)
    arr = (_lib.dfwfm_lazy_optim_table * 1)(_lib.dfwfm_lazy_optim_table(
        twin["p"].data_ptr(), twin["g"].data_ptr(), twin["s"].data_ptr(), twin["stamp"].data_ptr(), rows, rows, 0,
        width, 0, ref.PLAIN, 0))
    h = optim_ref.hyper("adag", LR, 0.0)
    _lib.check(_lib.lib().dfwfm_lazy_optim_step_dev(arr, 1, ctypes.c_void_p(xi.data_ptr()), 1, batch, ctypes.byref(h),
                                                    ctypes.c_void_p(_new_state(gpu).data_ptr()), _stream(gpu)),
               "dfwfm_lazy_optim_step_dev")
    torch.cuda.synchronize()
    assert torch.equal(t["p"], twin["p"]) and torch.equal(t["g"], twin["g"])
    assert torch.equal(t["s"][:, None].expand(rows, width), twin["s"])
    assert torch.equal(t["stamp"], twin["stamp"]) and int(t["stamp"].count_nonzero()) > 100


# ---------------------------------------------------------------------------------------------------- the step
def _trainer(name, gpu, B=37, wd=WD, det=True, **kw):
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, *_ = tc.case(name)  # (the weights do not depend on the case's batch)
    m = build(cfg, params, gpu, is_deep_dropout=False)
    t = FusedTrainStep(m, B, weight_decay=wd, deterministic=det, **{"optimizer": "adag", "lr": LR, **kw})
    t.seed = 12345
    return m, t


def _dev(gpu, *arrs):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrs)


def _snapshot(m, t):
    d = {k: p.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    for k in ("opt_state", "row_state", "exp_avg", "exp_avg_sq"):
        if getattr(t, k, None) is not None:
            d["/" + k] = getattr(t, k).cpu().numpy().copy()
    d["/counters"] = np.array([int(s[0].item()) for s in (t.state, t.state_t)])
    return d


def _batches(name, B, K):
    cfg, params, xi, xv, y = tc.case(name, B * K)
    return params, [(xi[k * B:(k + 1) * B], xv[k * B:(k + 1) * B], y[k * B:(k + 1) * B]) for k in range(K)]


def _table_info(m, t):
    """[(name, parameter, (column, key_range, kind, c), first row in row_state)] of the categorical tables in the
    trainer's order."""
    names = {id(p): k for k, p in m.named_parameters()}
    out, row0 = [], 0
    for p, d in zip(t.params[:t.n_cat], t.lazy_tables):
        out.append((names[id(p)], p, (int(d.column), int(d.key_range), int(d.kind), int(d.c)), row0))
        row0 += int(p.shape[0])
    return out


def _three_steps(gpu, name, det=True, own_grads=False, **kw):
    """Three steps on three batches, weight_decay 3e-7.  Before each step a twin model gets the row-wise model's
    parameters and runs dfwfm_train_forward + dfwfm_backward for the step's dense table gradients (own_grads: the
    trainer's own gradient buffer is read instead, right before its table update -- the atomic scatter's sums are not
    reproducible by a twin); the expected tables and row_state are dfwfm_rowwise_adagrad_row_ref on the touched rows,
    at the step's rate.  A FusedTrainStep(optimizer="adag", lazy_tables=True) twin holding the same parameters, state
    and counters runs the same batch: every non-table tensor and opt_state equal its result (not under own_grads).
    After every step the tables' region of the gradient buffer is all zero."""
    B, K = 37, 3
    cfg, params, *_ = tc.case(name)
    _, bats = _batches(name, B, K)
    m, t = _trainer(name, gpu, det=det, rowwise_tables=True, **kw)
    md, td = _trainer(name, gpu, det=det, lazy_tables=True, **kw)
    twin = build(cfg, params, gpu, is_deep_dropout=False)
    info = _table_info(m, t)
    table_names = {n for n, *_ in info}
    assert t.lazy and t.rowwise and t.row_state.dtype == torch.float32 and not bool(t.row_state.any())
    assert t.row_state.numel() == sum(int(p.shape[0]) for _, p, _, _ in info)
    assert t.opt_state.numel() == t.grad.numel() - t.n_tables and td.opt_state.numel() == td.grad.numel()
    seen = {}
    if own_grads:
        inner = t._adam_tables

        def spy(n):
            seen["g"] = t.grad[:t.n_tables].clone()
            inner(n)
        t._adam_tables = spy
    exp_s = {n: np.zeros(int(p.shape[0]), np.float32) for n, p, _, _ in info}
    for s, (xb, vb, yb) in enumerate(bats, 1):
        with torch.no_grad():
            for other in (twin, md):
                for (_, a), (_, b) in zip(m.named_parameters(), other.named_parameters()):
                    b.copy_(a)
            td.opt_state[td.n_tables:].copy_(t.opt_state)
        exp_p = {n: p.detach().cpu().numpy().copy() for n, p, _, _ in info}
        if not own_grads:
            twin._sync_engine(gpu).set_deterministic(True)
            grads, _, _ = _sparse_step(twin, gpu, xb, vb, yb, sparse=False)
        t.step(*_dev(gpu, xb, vb, yb))
        td.step(*_dev(gpu, xb, vb, yb))
        torch.cuda.synchronize()
        assert own_grads or t.graphs is not None or s == 1  # steps 2 and 3 are graph replays
        assert not bool(t.grad[:t.n_tables].any()), s
        assert int(t.state_t[0].item()) == int(t.state[0].item()) == s
        lr = t.lr_at(s)
        for n, p, (col, key_range, kind, c), row0 in info:
            if own_grads:
                off = (p.grad.data_ptr() - t.grad.data_ptr()) // 4
                g = seen["g"][off:off + p.numel()].view_as(p).cpu().numpy()
            else:
                g = grads[n]
            rows = ref.touched_rows(xb[:, col], key_range, kind, max(c, 1))
            assert not g[np.setdiff1d(np.arange(p.shape[0]), rows)].any(), n
            wp, _, ws = ref.rowwise_ref(exp_p[n], g, exp_s[n], xb[:, col], key_range, kind, max(c, 1), lr=lr,
                                        weight_decay=WD, eps=EPS, elem="lib")
            assert optim_ref.same_bits(p.detach().cpu().numpy(), wp), (n, s)
            assert optim_ref.same_bits(t.row_state[row0:row0 + p.shape[0]].cpu().numpy(), ws), (n, s)
            exp_s[n] = ws
        if own_grads:  # (arrival-order sums: the twin trainer's other gradients are not this trainer's)
            continue
        for (k, a), (_, b) in zip(m.named_parameters(), md.named_parameters()):
            if k not in table_names:
                assert np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy()), (k, s)
        assert np.array_equal(t.opt_state.cpu().numpy(), td.opt_state[td.n_tables:].cpu().numpy()), s
    assert bool(t.row_state.any()) and bool(t.opt_state.any())
    t.close()
    td.close()


@pytest.mark.parametrize("name", [n for n in tc.FUSED if n != "allnum"])
def test_three_rowwise_steps_equal_host_function_on_touched_rows(gpu, name):
    _three_steps(gpu, name)


def test_three_rowwise_steps_under_lr_schedule_with_a_knot_inside(gpu):
    """Knots at steps 1, 2 and 5: step 2 is at a knot, step 3 on the descent behind it; the scheduled row-wise entry
    runs on the tables and the scheduled dense one on the rest, at dfwfm_lr_schedule_eval(s)."""
    sched = [(1, 1e-4), (2, 1e-3), (5, 2e-4)]
    _three_steps(gpu, "qr_add", lr_schedule=sched)
    _, bats = _batches("fm_deep", 37, 1)
    res = []
    for kw in (dict(lr_schedule=sched), dict(lr_schedule=[(1, LR)]), dict()):
        m, t = _trainer("fm_deep", gpu, rowwise_tables=True, **kw)
        t.step(*_dev(gpu, *bats[0]))
        torch.cuda.synchronize()
        res.append(_snapshot(m, t))
        t.close()
    assert any(not np.array_equal(res[0][k], res[2][k]) for k in res[0])
    for k in res[1]:
        assert np.array_equal(res[1][k], res[2][k]), k  # the constant schedule IS the fixed rate


def test_set_lr_moves_the_tables_rate_without_a_recapture(gpu):
    """set_lr between graph replays: the next step's tables are the host function's at the new rate."""
    _, bats = _batches("fm_deep", 37, 3)
    m, t = _trainer("fm_deep", gpu, rowwise_tables=True, lr_schedule=[(1, LR)])
    for b in bats[:2]:
        t.step(*_dev(gpu, *b))
    graphs = t.graphs
    t.set_lr(5e-3)
    assert t.lr_at(3) == 5e-3
    before = _snapshot(m, t)
    twin_m, twin_t = _trainer("fm_deep", gpu, rowwise_tables=True, lr=5e-3)
    with torch.no_grad():
        for (_, a), (_, b) in zip(m.named_parameters(), twin_m.named_parameters()):
            b.copy_(a)
    twin_t.opt_state.copy_(t.opt_state)
    twin_t.row_state.copy_(t.row_state)
    for st in (twin_t.state, twin_t.state_t):
        st[0] = 2
    twin_t.step(*_dev(gpu, *bats[2]))  # an eager step at the fixed rate 5e-3, as step 3
    t.step(*_dev(gpu, *bats[2]))
    torch.cuda.synchronize()
    assert t.graphs is graphs
    a, b = _snapshot(m, t), _snapshot(twin_m, twin_t)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert any(not np.array_equal(a[k], before[k]) for k in a)
    t.close()
    twin_t.close()


def test_three_rowwise_steps_with_the_atomic_scatter(gpu):
    """deterministic=False (float-atomic scatter, arrival-order sums): the expectation is the host function on the
    trainer's OWN table gradients, read right before its table update (eager steps)."""
    _three_steps(gpu, "fm_deep", det=False, own_grads=True, use_graph=False)


def test_lazy_tables_may_be_passed_or_not(gpu):
    _, bats = _batches("qr_add", 37, 3)
    res = []
    for kw in (dict(), dict(lazy_tables=True)):
        m, t = _trainer("qr_add", gpu, rowwise_tables=True, **kw)
        for b in bats:
            t.step(*_dev(gpu, *b))
        torch.cuda.synchronize()
        res.append(_snapshot(m, t))
        t.close()
    assert res[0].keys() == res[1].keys() and "/row_state" in res[0]
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k


def test_no_categorical_table_makes_the_switch_a_no_op(gpu):
    _, bats = _batches("allnum", 37, 2)
    res = []
    for kw in (dict(), dict(rowwise_tables=True)):
        m, t = _trainer("allnum", gpu, **kw)
        assert not t.lazy and t.opt_state.numel() == t.grad.numel()
        assert (t.row_state is None) if not kw else t.row_state.numel() == 0
        for b in bats:
            t.step(*_dev(gpu, *b))
        torch.cuda.synchronize()
        res.append(_snapshot(m, t))
        t.close()
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k


def test_step_many_equals_single_steps_under_the_switch(gpu):
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    B, K = 37, 3
    cfg, params, xi, xv, y = tc.case("qr_add", B * (K + 1))
    bat = [_dev(gpu, xi[k * B:(k + 1) * B], xv[k * B:(k + 1) * B], y[k * B:(k + 1) * B]) for k in range(K + 1)]
    res = []
    for many in (False, True):
        m = build(cfg, params, gpu, is_deep_dropout=False)
        t = FusedTrainStep(m, B, lr=LR, weight_decay=WD, resident_inputs=True, deterministic=True, optimizer="adag",
                           rowwise_tables=True)
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
    assert res[0]["/counters"].tolist() == [K + 1, K + 1]
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k


def test_serving_copy_is_refreshed_after_rowwise_steps(gpu):
    """The eval forward over the f32 serving copy (pack_tables, the default), re-packed after the steps, equals the
    plain-table forward bit for bit."""
    cfg, params, xi, xv, y = tc.case("fm_deep")
    m, t = _trainer("fm_deep", gpu, rowwise_tables=True)
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


class _Counting:
    """The library handle with every call counted by symbol name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


def _counted_steps(gpu, monkeypatch, steps=3, **kw):
    """(snapshot, {symbol: calls}) of `steps` steps on fm_deep's batches by a trainer built with **kw."""
    from xsdeepfwfm_deprecated_amd import _lib
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, *_ = tc.case("fm_deep")
    _, bats = _batches("fm_deep", 37, steps)
    proxy = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", proxy)
    try:
        m = build(cfg, params, gpu, is_deep_dropout=False)
        t = FusedTrainStep(m, 37, lr=LR, weight_decay=WD, deterministic=True, **kw)
        t.seed = 12345
        assert t.L is proxy
        for b in bats:
            t.step(*_dev(gpu, *b))
        torch.cuda.synchronize()
        snap = _snapshot(m, t)
        t.close()
    finally:
        monkeypatch.undo()
    return snap, proxy.calls


def test_off_means_off(gpu, monkeypatch):
    """With the switch off no symbol of include/dfwfm_rowwise_adagrad.h is called and row_state is None; a default Adam
    trainer and an optimizer="adag", lazy_tables=True trainer built AFTER the new path has run give the bits of the
    ones built before it.  With the switch on, the tables go through the new entry point (the scheduled one under
    lr_schedule) and the rest through the dense one."""
    from xsdeepfwfm_deprecated_amd import _lib
    new = set(_lib.ROWWISE_ADAGRAD_SIGNATURES)
    assert len(new) == 4 and all(n.startswith("dfwfm_rowwise_adagrad_") for n in new)
    old = (dict(), dict(optimizer="adag", lazy_tables=True))
    first = [_counted_steps(gpu, monkeypatch, **kw) for kw in old]
    on, calls = _counted_steps(gpu, monkeypatch, optimizer="adag", rowwise_tables=True)
    assert calls.get("dfwfm_rowwise_adagrad_step_dev", 0) >= 2 and calls.get("dfwfm_optim_step_dev", 0) >= 2
    assert not {"dfwfm_lazy_optim_step_dev", "dfwfm_lazy_adam_step_dev", "dfwfm_adam_step_dev",
                "dfwfm_rowwise_adagrad_step_dev_sched"} & set(calls)
    _, calls = _counted_steps(gpu, monkeypatch, optimizer="adag", rowwise_tables=True,
                              lr_schedule=[(1, 1e-4), (3, 1e-3)])
    assert calls.get("dfwfm_rowwise_adagrad_step_dev_sched", 0) >= 2 and "dfwfm_rowwise_adagrad_step_dev" not in calls
    again = [_counted_steps(gpu, monkeypatch, **kw) for kw in old]
    for (a, ca), (b, cb), used in zip(first, again, ("dfwfm_adam_step_dev", "dfwfm_lazy_optim_step_dev")):
        assert ca == cb and ca.get(used, 0) >= 2 and not new & set(ca), sorted(ca)
        assert a.keys() == b.keys() and "/row_state" not in a
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    assert "/row_state" in on and first[1][0]["/opt_state"].size > on["/opt_state"].size
    assert any(not np.array_equal(on[k], first[1][0][k]) for k in on if "embeddings" in k)  # another optimizer


def test_constructor_refusals(gpu):
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, *_ = tc.case("fm_deep")
    m = build(cfg, params, gpu, is_deep_dropout=False)

    class FakeDist:  # refused before it is asked anything
        pass
    for kw in (dict(), dict(lazy_tables=True), dict(lazy_tables=True, lazy_exchange=True)):
        with pytest.raises(NotImplementedError, match="dfwfm_lazy_lists_span"):
            FusedTrainStep(m, 37, dist=FakeDist(), optimizer="adag", rowwise_tables=True, **kw)
    for opt in ("adam", "sgd", "rmsp"):
        with pytest.raises(ValueError, match="optimizer='adag'"):
            FusedTrainStep(m, 37, optimizer=opt, rowwise_tables=True)
    for opt in ("adam", "adag"):
        with pytest.raises(ValueError, match="lazy_table_adam"):
            FusedTrainStep(m, 37, optimizer=opt, rowwise_tables=True, lazy_table_adam=True)
    # a model whose only trainable parameters are tables raises as the lazy switches do
    for k, p in m.named_parameters():
        p.requires_grad_("embeddings" in k and int(k.split(".")[1]) >= cfg["numerical"])
    with pytest.raises(NotImplementedError, match="rowwise_tables: a model whose only trainable parameters are tables"):
        FusedTrainStep(m, 37, optimizer="adag", rowwise_tables=True)


def _fit_set(rows):
    from xsdeepfwfm_deprecated_amd import synth
    sizes = [1] * 13 + [50, 300, 7, 1000, 20, 5, 64, 9, 100, 3, 11, 17, 250, 4, 6, 30, 8, 2, 40, 12, 90, 5, 15,
                        300, 7, 60]
    xi, xv = synth.synth_inputs(sizes, 13, rows, seed=5)
    logit = ((xi[:, 0] % 7) - 3) * 0.6 + (xv[:, 0] > 30) * 1.0 - 0.5
    y = (np.random.default_rng(1).random(rows) < 1 / (1 + np.exp(-logit))).astype(np.float32)
    return sizes, xi, xv, y


def test_fit_with_rowwise_adagrad_learns(gpu, caplog):
    """fit() end to end under the switch on test_fit_with_lazy_adagrad_learns' synthetic set: the last logged training
    loss is below the first."""
    import logging
    from xsdeepfwfm_deprecated_amd import DeepFMs
    sizes, xi, xv, y = _fit_set(4096)
    log = logging.getLogger("test_rowwise_adagrad_fit")
    log.setLevel(logging.INFO)
    m = DeepFMs(field_size=39, feature_sizes=sizes, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1, n_epochs=3,
                batch_size=256, learning_rate=1e-2, weight_decay=3e-7, h_depth=2, deep_nodes=64, logger=log,
                optimizer_type="adag").to(gpu)
    m.fused_optimizer = True
    m.rowwise_adagrad = True
    with caplog.at_level(logging.INFO, logger="test_rowwise_adagrad_fit"):
        m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    losses = [float(r.getMessage().split("loss:")[1].split()[0]) for r in caplog.records
              if r.getMessage().startswith("Training [")]
    assert len(losses) == 3 and losses[-1] < losses[0], losses


def test_fit_refuses_the_switch_off_the_fused_adagrad_step(gpu):
    """fused_fit off, a teacher model, an optimizer_type other than 'adag', or fused_optimizer off: ValueError before
    the first batch."""
    from xsdeepfwfm_deprecated_amd import DeepFMs
    sizes, xi, xv, y = _fit_set(512)

    def model(opt, fused_optimizer=True):
        m = DeepFMs(field_size=39, feature_sizes=sizes, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1, n_epochs=1,
                    batch_size=256, h_depth=1, deep_nodes=16, optimizer_type=opt).to(gpu)
        m.rowwise_adagrad = True
        m.fused_optimizer = fused_optimizer
        return m
    m = model("adag")
    m.fused_fit = False
    with pytest.raises(ValueError, match="rowwise_adagrad"):
        m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    with pytest.raises(ValueError, match="rowwise_adagrad"):
        model("adag").fit(xi.reshape(-1, 26, 1), xv, y, [], [], [], teacher_model=model("adag"))
    for opt in ("adam", "sgd", "rmsp"):
        with pytest.raises(ValueError, match="rowwise_adagrad"):
            model(opt).fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    with pytest.raises(ValueError, match="rowwise_adagrad"):
        model("adag", fused_optimizer=False).fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
