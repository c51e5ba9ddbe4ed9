"""GPU: device-resident learning-rate schedules (include/dfwfm_lr_schedule.h).

The calls alone: dfwfm_adam_step_dev_sched / dfwfm_lazy_adam_step_dev_sched at step s (the state block's counter preset
to s - 1) against their unscheduled twins given lr = the schedule's value at s in exact rational arithmetic
(tests/lr_schedule_ref.py) -- every array, the stamps and the whole state block bit for bit; dfwfm_lr_schedule_write
inside and between captured graphs.

The step: FusedTrainStep(lr_schedule=...) against FusedTrainStep(lr=...) under a constant schedule, against a twin whose
rate the host sets before every step (set_lr: no recapture), step_many, fit(), and a trainer without a schedule calling
no scheduled symbol.  The trainer tests run train_cases' "num0" at B = 37: the smallest FUSED case that has categorical
tables ("allnum" is smaller but has none, so neither the tables' launch nor the lazy step would run)."""
import ctypes

import numpy as np
import pytest
import torch

import lazy_adam_ref as lref
import lr_schedule_ref as ref
import train_cases as tc
from test_gpu_lazy_adam import _clone, _new_state, _rand_table
from test_gpu_train import build

pytestmark = pytest.mark.gpu

WD, BETAS, EPS = 3e-7, (0.9, 0.999), 1e-8
# four knots: an ascending, a descending and another ascending segment
KNOTS = [(1, 1e-4), (5, 1e-3), (9, 2e-4), (12, 5e-4)]
STEPS = [1, 3, 5, 7, 9, 12, 20]  # the first step, mid-ascent, a knot, mid-descent, a knot, the last knot, past the end
CASE = "num0"


def _stream(gpu):
    return ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


def _block(gpu, knots=None):
    """A schedule block on the device (zero-filled), written with `knots` if given."""
    from xsdeepfwfm_deprecated_amd import _lib
    b = torch.zeros(_lib.LR_SCHEDULE_BYTES // 8, dtype=torch.int64, device=gpu)
    if knots is not None:
        _write(b, knots, gpu)
    return b


def _write(block, knots, gpu):
    from xsdeepfwfm_deprecated_amd import _lib
    arr, n = _lib.lr_knots(knots)
    _lib.check(_lib.lib().dfwfm_lr_schedule_write(ctypes.c_void_p(block.data_ptr()), arr, n, _stream(gpu)),
               "dfwfm_lr_schedule_write")


def _state_at(gpu, s):
    st = _new_state(gpu)
    st[0] = s - 1
    return st


# ------------------------------------------------------------------------------------------------ the dense call
DENSE_SHAPES = [(1,), (37, 11), (1029,)]  # one element; numel % 4 == 3: the element-wise tail; a second 1024-element run


def _rand_tensors(gpu, seed=7):
    """[(p, g, m, v)] of DENSE_SHAPES: gradient magnitudes 1e-8 .. 1, moments as after earlier steps."""
    r = np.random.default_rng(seed)
    out = []
    for shape in DENSE_SHAPES:
        p = r.standard_normal(shape).astype(np.float32)
        g = (r.standard_normal(shape) * 10.0 ** r.uniform(-8, 0, shape)).astype(np.float32)
        m = (0.1 * r.standard_normal(shape)).astype(np.float32)
        v = (0.01 * r.random(shape)).astype(np.float32)
        out.append(tuple(torch.from_numpy(a).to(gpu) for a in (p, g, m, v)))
    return out


def _dense_call(tensors, state, gpu, sched=None, lr=None):
    from xsdeepfwfm_deprecated_amd import _lib
    arr = (_lib.dfwfm_adam_tensor * len(tensors))()
    for i, (p, g, m, v) in enumerate(tensors):
        arr[i] = _lib.dfwfm_adam_tensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
    st = ctypes.c_void_p(state.data_ptr())
    if sched is not None:
        _lib.check(_lib.lib().dfwfm_adam_step_dev_sched(arr, len(tensors), ctypes.c_void_p(sched.data_ptr()), BETAS[0],
                                                        BETAS[1], EPS, WD, st, _stream(gpu)),
                   "dfwfm_adam_step_dev_sched")
    else:
        _lib.check(_lib.lib().dfwfm_adam_step_dev(arr, len(tensors), lr, BETAS[0], BETAS[1], EPS, WD, st,
                                                  _stream(gpu)), "dfwfm_adam_step_dev")


def _same_tensors(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        for k, x, y in zip("pgmv", a, b):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy()), (what, DENSE_SHAPES[i], k)


@pytest.fixture(scope="module")
def dense_start(gpu):
    """The dense tests' starting tensors: built once, cloned by every test, never written."""
    return _rand_tensors(gpu)


@pytest.mark.parametrize("s", STEPS)
def test_dense_scheduled_call_equals_the_unscheduled_one_at_the_reference_rate(gpu, dense_start, s):
    sched = _block(gpu, KNOTS)
    got = [tuple(t.clone() for t in ts) for ts in dense_start]
    want = [tuple(t.clone() for t in ts) for ts in dense_start]
    st_got, st_want = _state_at(gpu, s), _state_at(gpu, s)
    _dense_call(got, st_got, gpu, sched=sched)
    _dense_call(want, st_want, gpu, lr=ref.lr_at(KNOTS, s))
    torch.cuda.synchronize()
    _same_tensors(got, want, s)
    assert int(st_got[0].item()) == s
    assert np.array_equal(st_got.cpu().numpy(), st_want.cpu().numpy())  # the counter, the step's scalars, the ticket
    assert not np.array_equal(got[2][0].cpu().numpy(), dense_start[2][0].cpu().numpy())
    # the rate is the schedule's, not some constant: a neighbouring step's rate gives other parameters
    other = [tuple(t.clone() for t in ts) for ts in dense_start]
    _dense_call(other, _state_at(gpu, s), gpu, lr=ref.lr_at(KNOTS, s + 2 if s < 12 else 10))
    assert not np.array_equal(got[2][0].cpu().numpy(), other[2][0].cpu().numpy())


def test_dense_scheduled_call_with_64_knots_and_an_empty_list(gpu, dense_start):
    """Every lane holds a knot (the last segment sits in lanes 62 / 63); and a list without tensors still advances the
    counter, as the unscheduled call does."""
    knots = [(2 * i + 1, 1e-4 * (1 + (i * 7) % 13)) for i in range(64)]
    sched = _block(gpu, knots)
    for s in (1, 2, 64, 124, 126, 127, 128):
        got = [tuple(t.clone() for t in ts) for ts in dense_start]
        want = [tuple(t.clone() for t in ts) for ts in dense_start]
        st_got, st_want = _state_at(gpu, s), _state_at(gpu, s)
        _dense_call(got, st_got, gpu, sched=sched)
        _dense_call(want, st_want, gpu, lr=ref.lr_at(knots, s))
        _same_tensors(got, want, s)
        assert np.array_equal(st_got.cpu().numpy(), st_want.cpu().numpy())
    st_got, st_want = _state_at(gpu, 4), _state_at(gpu, 4)
    _dense_call([], st_got, gpu, sched=sched)
    _dense_call([], st_want, gpu, lr=ref.lr_at(knots, 4))
    assert int(st_got[0].item()) == 4 and np.array_equal(st_got.cpu().numpy(), st_want.cpu().numpy())


# ------------------------------------------------------------------------------------------------- the lazy call
def _lazy_tables(gpu):
    """Plain width 10, plain width 1, QR quotient with c = 4 on 23 keys (6 rows)."""
    return [_rand_table(50, 10, 11, gpu, column=0), _rand_table(7, 1, 12, gpu, column=1),
            _rand_table(6, 10, 13, gpu, key_range=23, kind=lref.QUOTIENT, c=4, column=2)]


def _lazy_keys():
    """37 keys per table that leave rows untouched in each: 5 of the 7 rows, quotient rows 0 .. 2 of 6; one key past
    the QR table's range, which counts as key 0."""
    r = np.random.default_rng(17)
    keys = np.stack([r.integers(0, 50, 37), r.integers(0, 5, 37), r.integers(0, 12, 37)], axis=1)
    keys[0, 2] = 23
    return keys


def _lazy_call(tabs, xi, batch, state, gpu, sched=None, lr=None):
    from xsdeepfwfm_deprecated_amd import _lib
    arr = (_lib.dfwfm_lazy_adam_table * max(len(tabs), 1))()
    for i, t in enumerate(tabs):
        arr[i] = _lib.dfwfm_lazy_adam_table(t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(),
                                            t["stamp"].data_ptr(), t["rows"], t["key_range"], t["c"], t["width"],
                                            t["column"], t["kind"], 0)
    st, x = ctypes.c_void_p(state.data_ptr()), ctypes.c_void_p(xi.data_ptr())
    if sched is not None:
        _lib.check(_lib.lib().dfwfm_lazy_adam_step_dev_sched(arr, len(tabs), x, xi.stride(0), batch,
                                                             ctypes.c_void_p(sched.data_ptr()), BETAS[0], BETAS[1],
                                                             EPS, WD, st, _stream(gpu)),
                   "dfwfm_lazy_adam_step_dev_sched")
    else:
        _lib.check(_lib.lib().dfwfm_lazy_adam_step_dev(arr, len(tabs), x, xi.stride(0), batch, lr, BETAS[0], BETAS[1],
                                                       EPS, WD, st, _stream(gpu)), "dfwfm_lazy_adam_step_dev")


@pytest.fixture(scope="module")
def lazy_start(gpu):
    return _lazy_tables(gpu), _lazy_keys()


@pytest.mark.parametrize("s", STEPS)
def test_lazy_scheduled_call_equals_the_unscheduled_one_at_the_reference_rate(gpu, lazy_start, s):
    start, keys = lazy_start
    xi = torch.from_numpy(keys).to(gpu)
    sched = _block(gpu, KNOTS)
    got, want = [_clone(t) for t in start], [_clone(t) for t in start]
    st_got, st_want = _state_at(gpu, s), _state_at(gpu, s)
    _lazy_call(got, xi, 37, st_got, gpu, sched=sched)
    _lazy_call(want, xi, 37, st_want, gpu, lr=ref.lr_at(KNOTS, s))
    torch.cuda.synchronize()
    assert int(st_got[0].item()) == s
    assert np.array_equal(st_got.cpu().numpy(), st_want.cpu().numpy())
    for i, (a, b, t0) in enumerate(zip(got, want, start)):
        for k in ("p", "g", "m", "v", "stamp"):
            assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), (s, i, k)
        rows = lref.touched_rows(keys[:, i], t0["key_range"], t0["kind"], max(t0["c"], 1))
        rest = np.setdiff1d(np.arange(t0["rows"]), rows)
        assert len(rows) and len(rest)
        for k in "pgmv":  # untouched rows keep their bits, touched ones moved
            assert np.array_equal(a[k].cpu().numpy()[rest], t0[k].cpu().numpy()[rest]), (s, i, k)
        assert not np.array_equal(a["p"].cpu().numpy()[rows], t0["p"].cpu().numpy()[rows])
        assert not a["g"].cpu().numpy()[rows].any()


def test_lazy_scheduled_call_on_an_empty_batch_advances_the_counter_only(gpu, lazy_start):
    start, keys = lazy_start
    xi = torch.from_numpy(keys).to(gpu)
    got = [_clone(t) for t in start]
    state = _state_at(gpu, 6)
    sched = _block(gpu, KNOTS)
    _lazy_call(got, xi, 0, state, gpu, sched=sched)
    _lazy_call([], xi, 37, state, gpu, sched=sched)
    torch.cuda.synchronize()
    assert int(state[0].item()) == 7
    for a, t0 in zip(got, start):
        for k in ("p", "g", "m", "v", "stamp"):
            assert np.array_equal(a[k].cpu().numpy(), t0[k].cpu().numpy())


# ------------------------------------------------------------------------------------------- writes and graphs
def test_write_fills_the_block_and_clears_the_knots_past_the_count(gpu):
    block = _block(gpu, [(i + 1, 1e-3 * (i + 1)) for i in range(64)])
    _write(block, KNOTS, gpu)
    torch.cuda.synchronize()
    raw = block.cpu().numpy()
    assert int(raw[:1].view(np.int32)[0]) == 4
    assert raw[2:10:2].tolist() == [k[0] for k in KNOTS]
    assert raw[3:11:2].view(np.float64).tolist() == [k[1] for k in KNOTS]
    assert not raw[10:].any()


def _graph_of(gpu, fn):
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fn()
    torch.cuda.current_stream(gpu).wait_stream(s)
    return g


def test_write_then_step_in_one_captured_graph(gpu, dense_start):
    """A capture records and does not run.  The graph holds the write of KNOTS and a dense step; between the replays the
    host writes OTHER knots into the block, which the captured write replaces again: three replays equal three eager
    (write, step) pairs, i.e. steps 1 .. 3 of KNOTS."""
    other = [(1, 7e-2)]
    eager = [tuple(t.clone() for t in ts) for ts in dense_start]
    st_e, blk_e = _new_state(gpu), _block(gpu)
    for _ in range(3):
        _write(blk_e, KNOTS, gpu)
        _dense_call(eager, st_e, gpu, sched=blk_e)
        _write(blk_e, other, gpu)
    replay = [tuple(t.clone() for t in ts) for ts in dense_start]
    st_r, blk_r = _new_state(gpu), _block(gpu, other)

    def pair():
        _write(blk_r, KNOTS, gpu)
        _dense_call(replay, st_r, gpu, sched=blk_r)
    g = _graph_of(gpu, pair)
    torch.cuda.synchronize()
    assert int(st_r[0].item()) == 0 and int(blk_r[2].item()) == 1 and int(blk_r[:1].view(torch.int32)[0].item()) == 1
    for _ in range(3):
        g.replay()
        _write(blk_r, other, gpu)
    torch.cuda.synchronize()
    assert int(st_r[0].item()) == int(st_e[0].item()) == 3
    _same_tensors(replay, eager, "write + step")
    assert np.array_equal(st_r.cpu().numpy(), st_e.cpu().numpy())
    # and both are the unscheduled call at the reference's rates of steps 1, 2, 3
    want = [tuple(t.clone() for t in ts) for ts in dense_start]
    st_w = _new_state(gpu)
    for s in (1, 2, 3):
        _dense_call(want, st_w, gpu, lr=ref.lr_at(KNOTS, s))
    _same_tensors(replay, want, "reference rates")


def test_block_rewritten_between_replays_of_a_captured_step(gpu, dense_start, lazy_start):
    """The graph holds a dense and a lazy scheduled step and no write; the host rewrites the block before each of three
    replays (a constant, a table whose segment the step falls into, a constant again): each replay takes the new rate --
    no recapture."""
    start, keys = lazy_start
    xi = torch.from_numpy(keys).to(gpu)
    tables = [[(1, 3e-3)], [(1, 1e-4), (4, 1e-3)], [(1, 5e-5)]]
    dense_r, lazy_r = [tuple(t.clone() for t in ts) for ts in dense_start], [_clone(t) for t in start]
    dense_w, lazy_w = [tuple(t.clone() for t in ts) for ts in dense_start], [_clone(t) for t in start]
    st_d, st_l, blk = _new_state(gpu), _new_state(gpu), _block(gpu, tables[0])

    def steps():
        _dense_call(dense_r, st_d, gpu, sched=blk)
        _lazy_call(lazy_r, xi, 37, st_l, gpu, sched=blk)
    g = _graph_of(gpu, steps)
    st_dw, st_lw = _new_state(gpu), _new_state(gpu)
    for s, knots in enumerate(tables, 1):
        _write(blk, knots, gpu)
        g.replay()
        for t, t0 in zip(lazy_r + lazy_w, start + start):  # the lazy step zeroed its rows' gradients
            t["g"].copy_(t0["g"])
        _dense_call(dense_w, st_dw, gpu, lr=ref.lr_at(knots, s))
        _lazy_call(lazy_w, xi, 37, st_lw, gpu, lr=ref.lr_at(knots, s))
    torch.cuda.synchronize()
    assert int(st_d[0].item()) == int(st_l[0].item()) == 3
    _same_tensors(dense_r, dense_w, "dense")
    for a, b in zip(lazy_r, lazy_w):
        for k in ("p", "m", "v", "stamp"):
            assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k


# ------------------------------------------------------------------------------------------------------ the step
def _trainer(gpu, lazy=False, B=37, **kw):
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, *_ = tc.case(CASE)
    m = build(cfg, params, gpu, is_deep_dropout=False)
    t = FusedTrainStep(m, B, weight_decay=WD, deterministic=True, lazy_table_adam=lazy, **kw)
    t.seed = 12345
    return m, t


def _batches(gpu, K, B=37):
    cfg, params, xi, xv, y = tc.case(CASE, B * K)
    return [tuple(torch.from_numpy(np.ascontiguousarray(a[k * B:(k + 1) * B])).to(gpu) for a in (xi, xv, y))
            for k in range(K)]


def _snapshot(m, t):
    d = {k: p.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    d["/exp_avg"] = t.exp_avg.cpu().numpy().copy()
    d["/exp_avg_sq"] = t.exp_avg_sq.cpu().numpy().copy()
    d["/counters"] = np.array([int(s[0].item()) for s in (t.state, t.state_t)])
    return d


def _equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("lazy", [False, True])
def test_trainer_with_a_constant_schedule_equals_the_fixed_rate(gpu, lazy):
    """One eager step and three graph replays each: parameters, both moments and the counters are array_equal."""
    bats = _batches(gpu, 4)
    snaps = []
    for kw in (dict(lr_schedule=[(1, 1e-3)]), dict(lr=1e-3)):
        m, t = _trainer(gpu, lazy, **kw)
        assert t.lazy is lazy and (t.sched is not None) is ("lr_schedule" in kw)
        for b in bats:
            t.step(*b)
        torch.cuda.synchronize()
        assert t.graphs is not None and t.steps == 4
        snaps.append(_snapshot(m, t))
        t.close()
    _equal(snaps[0], snaps[1])
    cfg, params, *_ = tc.case(CASE)
    assert any(not np.array_equal(params[k], snaps[0][k]) for k in params)


MOVING = [(1, 1e-4), (3, 1e-3), (5, 2e-4)]


@pytest.fixture(scope="module")
def moving_result(gpu):
    """Five single steps under MOVING (one eager, four graph replays): shared by the tests below, never written."""
    bats = _batches(gpu, 5)
    m, t = _trainer(gpu, lr_schedule=MOVING, resident_inputs=True)
    for b in bats:
        t.step(*b)
    torch.cuda.synchronize()
    snap = _snapshot(m, t)
    assert [t.lr_at(s) for s in range(1, 7)] == [ref.lr_at(MOVING, s) for s in range(1, 7)]
    t.close()
    return snap


def test_trainer_with_a_moving_schedule_equals_a_twin_set_from_the_host(gpu, moving_result):
    bats = _batches(gpu, 5)
    m, t = _trainer(gpu, lr_schedule=[(1, 1.0)])
    graphs = keys = None
    for s, b in enumerate(bats, 1):
        t.set_lr(ref.lr_at(MOVING, s))
        assert t.lr_schedule == [(1, ref.lr_at(MOVING, s))] and t.lr_at(s) == ref.lr_at(MOVING, s)
        t.step(*b)
        if s == 2:  # the first graph step: what it captured is what every later step replays
            graphs, keys = t.graphs, list(t._graph_sets)
            assert graphs is not None and len(keys) == 1
    torch.cuda.synchronize()
    assert t.graphs is graphs and all(a is b for a, b in zip(t.graphs, graphs))
    assert list(t._graph_sets) == keys and t._graph_sets[keys[0]][0] is graphs
    _equal(_snapshot(m, t), moving_result)
    t.close()
    # and a fixed rate does NOT give this result: the schedule moved the rate
    m, t = _trainer(gpu, lr=1e-3)
    for b in bats:
        t.step(*b)
    torch.cuda.synchronize()
    fixed = _snapshot(m, t)
    assert not np.array_equal(fixed["/exp_avg"], moving_result["/exp_avg"])  # other parameters, other gradients
    assert sum(not np.array_equal(fixed[k], moving_result[k]) for k in fixed) >= len(fixed) - 1  # (all but the counters)
    t.close()


def test_step_many_equals_single_steps_under_the_schedule(gpu, moving_result):
    bats = _batches(gpu, 5)
    m, t = _trainer(gpu, lr_schedule=MOVING, resident_inputs=True)
    t.step(*bats[0])
    t.step_many(bats[1:])
    torch.cuda.synchronize()
    assert any(k[0] == "many" for k in t._many_sets) and t.steps == 5
    _equal(_snapshot(m, t), moving_result)
    t.close()


def test_the_data_parallel_and_one_launch_call_sites_read_the_schedule(gpu):
    """The Adam call sites the one-process step of a model with tables does not take: _adam_main / _adam_mlp (the
    data-parallel step's two launches, on state and state_b) and _adam_all (no categorical table: one launch on
    state).  Called directly on the same random gradients, counters preset to 3 (step 4 is mid-segment in MOVING):
    equal to a fixed-rate trainer's calls at the reference's rates of steps 4 and 5."""
    snaps = []
    for kw in (dict(lr_schedule=MOVING), dict(lr=ref.lr_at(MOVING, 4))):
        m, t = _trainer(gpu, **kw)
        t.grad.copy_(torch.from_numpy(np.random.default_rng(8).standard_normal(t.grad.numel()).astype(np.float32)))
        t.state[0] = 3
        t.state_b[0] = 3
        t._adam_main()
        t._adam_mlp()
        torch.cuda.synchronize()
        assert int(t.state[0].item()) == int(t.state_b[0].item()) == 4
        if "lr" in kw:
            t.lr = ref.lr_at(MOVING, 5)
        t._adam_all()
        torch.cuda.synchronize()
        assert int(t.state[0].item()) == 5
        snaps.append(_snapshot(m, t))
        t.close()
    _equal(snaps[0], snaps[1])
    assert snaps[0]["/exp_avg"].any()


def test_set_lr_needs_a_schedule_and_rejects_bad_tables(gpu):
    from xsdeepfwfm_deprecated_amd import _lib
    m, t = _trainer(gpu, lr=1e-3)
    assert t.sched is None and t.lr_at(5) == 1e-3
    with pytest.raises(RuntimeError, match="lr_schedule"):
        t.set_lr(1e-4)
    t.close()
    m, t = _trainer(gpu, lr_schedule=MOVING)
    for bad in ([], [(0, 1e-3)], [(2, 1e-3), (2, 1e-4)], [(1, float("nan"))], [(1, -1e-3)],
                [(i + 1, 1e-3) for i in range(65)]):
        with pytest.raises(_lib.DfwfmError):
            t.set_lr_schedule(bad)
    assert t.lr_schedule == MOVING  # a refused table leaves the schedule as it was
    t.close()
    with pytest.raises(_lib.DfwfmError):
        _trainer(gpu, lr_schedule=[(3, 1e-3), (2, 1e-4)])


def test_fit_with_a_warm_up_schedule_learns(gpu, caplog):
    """fit() end to end on test_fit_with_lazy_table_adam_learns' synthetic set (16 steps per epoch, 3 epochs) with a
    warm-up over the first epoch and a decay after it: the last logged training loss is below the first."""
    import logging
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = [1] * 13 + [50, 300, 7, 1000, 20, 5, 64, 9, 100, 3, 11, 17, 250, 4, 6, 30, 8, 2, 40, 12, 90, 5, 15,
                        300, 7, 60]
    xi, xv = synth.synth_inputs(sizes, 13, 4096, seed=5)
    logit = ((xi[:, 0] % 7) - 3) * 0.6 + (xv[:, 0] > 30) * 1.0 - 0.5
    y = (np.random.default_rng(1).random(4096) < 1 / (1 + np.exp(-logit))).astype(np.float32)
    log = logging.getLogger("test_lr_schedule_fit")
    log.setLevel(logging.INFO)
    m = DeepFMs(field_size=39, feature_sizes=sizes, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1, n_epochs=3,
                batch_size=256, learning_rate=123.0, weight_decay=3e-7, h_depth=2, deep_nodes=64, logger=log).to(gpu)
    m.lr_schedule = [(1, 1e-3), (16, 1e-2), (48, 2e-3)]
    with caplog.at_level(logging.INFO, logger="test_lr_schedule_fit"):
        m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    losses = [float(r.getMessage().split("loss:")[1].split()[0]) for r in caplog.records
              if r.getMessage().startswith("Training [")]
    # (learning_rate = 123 is unused under a schedule: at that rate the loss would not fall)
    assert len(losses) == 3 and losses[-1] < losses[0], losses


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


@pytest.mark.parametrize("lazy", [False, True])
def test_off_means_off(gpu, monkeypatch, lazy):
    """A trainer built without a schedule calls no symbol of include/dfwfm_lr_schedule.h, from its construction through
    an eager step, a capture and replays; one built with a schedule calls no unscheduled Adam step."""
    from xsdeepfwfm_deprecated_amd import _lib
    new = {"dfwfm_lr_schedule_abi_version", "dfwfm_lr_schedule_eval", "dfwfm_lr_schedule_write",
           "dfwfm_adam_step_dev_sched", "dfwfm_lazy_adam_step_dev_sched"}
    assert new == set(_lib.LR_SCHEDULE_SIGNATURES)
    old = {"dfwfm_adam_step_dev", "dfwfm_lazy_adam_step_dev", "dfwfm_adam_step"}
    bats = _batches(gpu, 3)
    for kw, never, used in ((dict(lr=1e-3), new, "dfwfm_adam_step_dev"),
                            (dict(lr_schedule=MOVING), old, "dfwfm_adam_step_dev_sched")):
        proxy = _Counting(_lib.lib())
        monkeypatch.setattr(_lib, "_lib", proxy)
        m, t = _trainer(gpu, lazy, **kw)
        assert t.L is proxy
        for b in bats:
            t.step(*b)
        torch.cuda.synchronize()
        t.close()
        monkeypatch.undo()
        assert proxy.calls.get(used, 0) >= 2 and proxy.calls.get("dfwfm_train_forward", 0) >= 2, proxy.calls
        assert not never & set(proxy.calls), sorted(never & set(proxy.calls))
        if lazy:
            assert proxy.calls.get("dfwfm_lazy_adam_step_dev_sched" if "lr_schedule" in kw
                                   else "dfwfm_lazy_adam_step_dev", 0) >= 2, proxy.calls
