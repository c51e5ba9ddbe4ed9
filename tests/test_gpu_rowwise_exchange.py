"""GPU: row-wise Adagrad for the categorical tables under data parallelism (FusedTrainStep(rowwise_exchange=True),
include_dp/dfwfm_rowwise_lists.h), on spawned ranks that share cuda:0 (at most five GPU processes at once: this one and
four ranks).

Two gloo ranks (step 1 eager, steps 2 and 3 replayed graph pieces, step 4 a 49-row global batch) on the 64-row train
goldens, 32 rows per rank, deterministic: replicas bit-identical (row_state and opt_state included), the tables'
gradient region all zero after every step, rows no rank touched keep their bits in the tensor and in row_state, the
three counters equal; the same with lr_schedule, and with lazy_tables passed as well.  A world-size-1 RCCL group
(collectives inside the step's graph, and between its graphs): four deterministic steps, the last one partial, equal
the one-process rowwise_tables trainer bit for bit.  The exact-arithmetic witness (tests/dp_cases.py, the saturated
128-row case) on 3 ranks and on 4 with an empty shard: one step equals the one-process row-wise trainer on the whole
batch and dfwfm_rowwise_adagrad_row_ref on the float64 reference's gradient rows.  fit() on two gloo ranks.  The
refusals.

Each spawned job runs once per module (a fixture); the tests assert on what it returned."""
import os

import numpy as np
import pytest
import torch

import dp_cases as dc
import exact_train_cases as xc
import rowwise_adagrad_ref as rw
import train_cases as tc
from conftest import load_train_golden
from test_gpu_lazy_exchange import FakeDist, _differ, _digest, _port, _table_rows
from test_gpu_train import build

pytestmark = pytest.mark.gpu

NAMES = ["train_deepfwfm_lw", "train_qr_mult"]
G, BS, PARTIAL = 64, 32, 49
SCHEDULE = [(1, 1e-4), (3, 1e-3)]
ROWWISE = dict(optimizer="adag", rowwise_tables=True, weight_decay=3e-7)
RUNS = {
    "rowwise": dict(ROWWISE, rowwise_exchange=True),
    "rowwise_lazy_tables": dict(ROWWISE, rowwise_exchange=True, lazy_tables=True),
    "rowwise_sched": dict(ROWWISE, rowwise_exchange=True, lr_schedule=SCHEDULE),
}
WITNESS_PLANS = {3: "w3", 4: "w4-middle"}  # world -> plan of dc.B1_PLANS; w4-middle leaves rank 3 an empty shard
WITNESS_LR = xc.SGD_LR


# ------------------------------------------------------------------------------------------- what a rank runs
def _snap(m, t, logits=None):
    """Every tensor and state array of a trainer, on the host."""
    s = {"p/" + n: p.detach().cpu().numpy().copy() for n, p in m.named_parameters()}
    for k in ("opt_state", "row_state"):
        a = getattr(t, k)
        if a is not None:
            s["s/" + k] = a.detach().cpu().numpy().copy()
    if logits is not None:
        s["logits"] = logits
    return s


def _row_slices(m, t):
    """name -> (first row, rows) of each categorical table in row_state."""
    names = {id(p): n for n, p in m.named_parameters()}
    out, row0 = {}, 0
    for p in t.params[:t.n_cat]:
        out[names[id(p)]] = (row0, int(p.shape[0]))
        row0 += int(p.shape[0])
    return out


def _steps(name, kw, steps, dist, rank, world, partial=True):
    """`steps` deterministic FusedTrainSteps on the 64-row global batches of train golden `name`, this rank taking its
    contiguous share, then with `partial` a 49-row global batch (32 rows on rank 0, 17 on rank 1).  Returns the
    snapshots after every step and what was checked on the way."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, xi, xv, y, *_ = load_train_golden(name)
    dev = torch.device("cuda:0")
    bs = G // world
    m = build(cfg, params, dev, is_deep_dropout=False)
    t = FusedTrainStep(m, bs, **dict(dict(lr=1e-3, dist=dist, deterministic=True), **kw))
    start = _snap(m, t)
    assert t.row_state.numel() == sum(r for _, r in _row_slices(m, t).values())
    assert t.opt_state.numel() == t.grad.numel() - t.n_tables  # opt_state covers only the other parameters
    snaps, grad_zero = {}, []
    plan = [(k * G, G) for k in range(steps)] + ([(steps * G, PARTIAL)] if partial else [])
    for k, (g0, n_global) in enumerate(plan, 1):
        lo, hi = dc.fit_shards(n_global, bs, world, g0)[rank]
        xb, vb, yb = (torch.from_numpy(a[lo:hi]).to(dev) for a in (xi, xv, y))
        t.step(xb, vb, yb, n_global if dist is not None else None)
        torch.cuda.synchronize()
        nz = torch.nonzero(t.grad[:t.n_tables]).flatten()
        grad_zero.append(nz.numel() == 0 or (int(nz.numel()), nz[:4].tolist()))  # (on a failure: how many, where)
        snaps[k] = _snap(m, t, t.out[:hi - lo].detach().cpu().numpy().copy())
    info = {"grad_zero": grad_zero,
            "digest": {k: _digest({n: a for n, a in s.items() if n != "logits"}) for k, s in snaps.items()},
            "lazy_lists": bool(t.lazy_lists), "rowwise": bool(t.rowwise), "graphs": t.graphs is not None,
            "counters": [int(c[0].item()) for c in (t.state, t.state_b, t.state_t)]}
    # rows of the tables that no rank's slice of any batch touched keep their bits, in the tensor and in row_state
    touched = _table_rows(m, xi[:plan[-1][0] + plan[-1][1]])
    last, rows_of = snaps[len(plan)], _row_slices(m, t)
    bad, n_untouched, n_changed, n_fed = [], 0, 0, 0
    for n, p in m.named_parameters():
        if n not in touched:
            continue
        rest = np.setdiff1d(np.arange(p.shape[0]), touched[n])
        n_untouched += len(rest)
        acc = last["s/row_state"][rows_of[n][0]:rows_of[n][0] + rows_of[n][1]]
        if not np.array_equal(last["p/" + n][rest], start["p/" + n][rest]):
            bad.append(n)
        if acc[rest].any():
            bad.append(n + " row_state")
        n_changed += int(not np.array_equal(last["p/" + n][touched[n]], start["p/" + n][touched[n]]))
        n_fed += int(np.all(acc[touched[n]] >= 0) and acc[touched[n]].any())
    info.update(untouched_changed=bad, n_untouched=n_untouched, tables_changed=n_changed, tables_fed=n_fed,
                n_tables=len(touched))
    t.close()
    return snaps, info


def _fit_two_ranks():
    """fit() under the switches on the small synthetic set of test_fit_with_rowwise_adagrad_learns."""
    import logging
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = [1] * 13 + [50, 300, 7, 1000, 20, 5, 64, 9, 100, 3, 11, 17, 250, 4, 6, 30, 8, 2, 40, 12, 90, 5, 15,
                        300, 7, 60]
    xi, xv = synth.synth_inputs(sizes, 13, 4096, seed=5)
    logit = ((xi[:, 0] % 7) - 3) * 0.6 + (xv[:, 0] > 30) * 1.0 - 0.5
    y = (np.random.default_rng(1).random(4096) < 1 / (1 + np.exp(-logit))).astype(np.float32)
    lines = []

    class Keep(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    log = logging.getLogger("test_rowwise_exchange_fit")
    log.setLevel(logging.INFO)
    log.propagate = False
    log.addHandler(Keep())
    m = DeepFMs(field_size=39, feature_sizes=sizes, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1, n_epochs=3,
                batch_size=256, learning_rate=1e-2, weight_decay=3e-7, h_depth=2, deep_nodes=64, logger=log,
                optimizer_type="adag", random_seed=3).to("cuda:0")
    m.fused_optimizer = True
    m.rowwise_adagrad = True
    m.rowwise_exchange = True
    m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    torch.cuda.synchronize()
    losses = [float(s.split("loss:")[1].split()[0]) for s in lines if s.startswith("Training [")]
    return losses, _digest({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()})


def _witness_step(dist, rank, world, bs, exchange):
    """One Adagrad step (lr 2^-6, no weight decay) from a fresh row-wise trainer on the saturated witness: this rank
    on fit()'s shard of the 128-row batch (dist None: one process on all of it).  Host arrays."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    sat = xc.saturated()
    case = sat.case
    dev = torch.device("cuda:0")
    m = build(case.cfg, {k: np.array(v) for k, v in case.params.items()}, dev, is_deep_dropout=False)
    t = FusedTrainStep(m, bs, lr=WITNESS_LR, optimizer="adag", rowwise_tables=True, weight_decay=0.0, dist=dist,
                       deterministic=True, **(dict(rowwise_exchange=True) if exchange else {}))
    lo, hi = dc.fit_shards(xc.SAT_B, bs, world)[rank]
    xi, xv, y = (torch.from_numpy(np.array(x[lo:hi])).to(dev) for x in (case.xi, case.xv, sat.y))
    t.step(xi, xv, y, xc.SAT_B if dist is not None else None)
    torch.cuda.synchronize()
    res = {"params": {k: q.detach().cpu().numpy().copy() for k, q in m.named_parameters()},
           "row_state": t.row_state.cpu().numpy().copy(), "rows_of": _row_slices(m, t), "rows": hi - lo,
           "lazy_lists": bool(t.lazy_lists), "tables_grad_zero": not bool(t.grad[:t.n_tables].any()),
           "counters": [int(c[0].item()) for c in (t.state, t.state_b, t.state_t)]}
    t.close()
    return res


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    torch.set_num_threads(2)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {}
        if world == 2:
            for name in NAMES:
                for key, kw in RUNS.items():
                    _, res[name, key] = _steps(name, kw, 3, dist, rank, world)
            res["fit"] = _fit_two_ranks()
        else:
            res["witness"] = _witness_step(dist, rank, world, dc.B1_PLANS[WITNESS_PLANS[world]][1], True)
        q.put((rank, "ok", res))
    except Exception as e:  # report, do not hang the parent
        import traceback
        q.put((rank, "error", repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _rccl_worker(port, q):
    """A world-size-1 RCCL group: the row-wise data-parallel step (collectives inside the step's graph, then between
    its graphs) against the one-process row-wise trainer in the same process."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        res = {}
        one, _ = _steps(NAMES[0], ROWWISE, 3, None, 0, 1)
        for graph_comm in (True, False):
            os.environ["DFWFM_DP_GRAPH_COMM"] = "1" if graph_comm else "0"
            dp, info = _steps(NAMES[0], dict(ROWWISE, rowwise_exchange=True), 3, dist, 0, 1)
            info["differs_from_one_process"] = {k: _differ(dp[k], one[k]) for k in dp}
            info["moved"] = len(_differ(dp[1], dp[4]))
            res[graph_comm] = info
        q.put(("ok", res))
    except Exception as e:  # report, do not hang the parent
        import traceback
        q.put(("error", repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------- the jobs, run once
def _spawn_gloo(world):
    import torch.multiprocessing as mp
    port = _port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = [q.get(timeout=300) for _ in procs]
        for p in procs:
            p.join(60)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    for rank, status, res in got:
        assert status == "ok", (rank, res)
    assert all(p.exitcode == 0 for p in procs)
    return {rank: res for rank, _, res in got}


@pytest.fixture(scope="module")
def gloo(gpu):
    return _spawn_gloo(2)


@pytest.fixture(scope="module")
def witness(gpu):
    """world -> {rank: results} of the witness step, each world's job run once, one after the other."""
    done = {}

    def get(world):
        if world not in done:
            done[world] = _spawn_gloo(world)
        return done[world]
    return get


@pytest.fixture(scope="module")
def one_process_witness(gpu):
    return _witness_step(None, 0, 1, xc.SAT_B, False)


@pytest.fixture(scope="module")
def rccl(gpu):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_port(), q))
    p.start()
    try:
        status, res = q.get(timeout=300)
        p.join(60)
    finally:
        if p.is_alive():
            p.terminate()
    assert status == "ok", res
    assert p.exitcode == 0
    return res


# ------------------------------------------------------------------------------------------- two gloo ranks
@pytest.mark.parametrize("key", list(RUNS))
@pytest.mark.parametrize("name", NAMES)
def test_replicas_are_bit_identical_and_the_tables_gradient_stays_zero(gloo, name, key):
    """After every step (1 eager, 2 and 3 graph replays, 4 a partial batch) the two ranks hold the same bits in every
    tensor, in row_state and in opt_state, the tables' region of the gradient buffer is all zero, all three counters
    stand at the step, and the lists update ran (nothing fell back to another path)."""
    a, b = gloo[0][name, key], gloo[1][name, key]
    assert a["lazy_lists"] and b["lazy_lists"] and a["rowwise"] and a["graphs"]
    assert a["digest"] == b["digest"] and len(a["digest"]) == 4
    assert len(set(a["digest"].values())) == 4  # and every step moved something
    assert a["grad_zero"] == [True] * 4 and b["grad_zero"] == [True] * 4
    assert a["counters"] == [4, 4, 4] and b["counters"] == [4, 4, 4]


@pytest.mark.parametrize("key", list(RUNS))
@pytest.mark.parametrize("name", NAMES)
def test_rows_no_rank_touched_keep_their_bits(gloo, name, key):
    for rank in (0, 1):
        r = gloo[rank][name, key]
        assert r["untouched_changed"] == []
        assert r["n_untouched"] > 1000 and r["tables_changed"] >= r["n_tables"] // 2 > 0  # (and the touched ones moved)
        assert r["tables_fed"] == r["n_tables"]  # every table's touched accumulators were fed


@pytest.mark.parametrize("name", NAMES)
def test_lazy_tables_may_be_passed_or_not_and_the_schedule_is_read(gloo, name):
    r = gloo[0]
    assert r[name, "rowwise"]["digest"] == r[name, "rowwise_lazy_tables"]["digest"]
    assert r[name, "rowwise"]["digest"][1] != r[name, "rowwise_sched"]["digest"][1]  # step 1 at 1e-4, not 1e-3


def test_fit_two_ranks_under_the_switches_learns_with_identical_replicas(gloo):
    (l0, d0), (l1, d1) = gloo[0]["fit"], gloo[1]["fit"]
    assert d0 == d1
    assert len(l0) == 3 and l0[-1] < l0[0], l0
    assert l0 == l1


# ------------------------------------------------------------------------------------------- RCCL, world size 1
@pytest.mark.parametrize("graph_comm", [True, False], ids=["in-graph", "between-graphs"])
def test_rccl_world_one_rowwise_exchange_equals_one_process_rowwise_trainer(rccl, graph_comm):
    """Four deterministic steps through the exchange, the last one partial (a stale list tail would show), equal the
    one-process rowwise_tables trainer bit for bit: every parameter, row_state, opt_state and the logits."""
    r = rccl[graph_comm]
    assert r["lazy_lists"] and r["rowwise"] and r["graphs"]
    assert r["differs_from_one_process"] == {1: [], 2: [], 3: [], 4: []}
    assert r["grad_zero"] == [True] * 4 and r["counters"] == [4, 4, 4] and r["moved"] > 10
    assert r["untouched_changed"] == [] and r["n_untouched"] > 1000


# ------------------------------------------------------------------------------------------- the witness
@pytest.mark.parametrize("world", sorted(WITNESS_PLANS))
def test_exact_witness_step_equals_one_process_and_the_host_function(witness, one_process_witness, world):
    """On the saturated 128-row case every gradient sum is exact in any order, so after one step every rank's
    parameters and row_state equal, bit for bit, the one-process row-wise trainer's on the whole batch, and the tables
    equal dfwfm_rowwise_adagrad_row_ref applied to the float64 reference's gradient rows (untouched rows: their start,
    a zero accumulator)."""
    plan = WITNESS_PLANS[world]
    _, bs = dc.B1_PLANS[plan]
    sat, one = xc.saturated(), one_process_witness
    _, g64 = xc.ref64(sat.case)
    touched = dc.touched(sat.case, 0, xc.SAT_B)
    want_p, want_acc = {}, np.zeros_like(one["row_state"])
    for n, (row0, rows) in one["rows_of"].items():
        p = np.array(sat.case.params[n], np.float32).reshape(rows, -1)
        idx = touched.get(n, np.zeros(0, np.int64))
        if len(idx):
            g = g64[n].reshape(rows, -1)[idx]
            assert np.array_equal(g.astype(np.float32).astype(np.float64), g)  # the witness: float32s
            p[idx], want_acc[row0 + idx] = rw.lib_rows(rw.hyper(WITNESS_LR, 0.0, 1e-10), p[idx], g.astype(np.float32),
                                                       np.zeros(len(idx), np.float32))
        want_p[n] = p.reshape(sat.case.params[n].shape)
    assert len(want_p) >= 26 and sum(len(v) for v in touched.values()) > 100
    assert not one["lazy_lists"] and one["rows"] == xc.SAT_B
    res = witness(world)
    assert [res[r]["witness"]["rows"] for r in range(world)] == dc.B1_SIZES[plan]
    for rank in [None] + list(range(world)):
        r = one if rank is None else res[rank]["witness"]
        what = (plan, "one process" if rank is None else ("rank", rank))
        assert r["lazy_lists"] == (rank is not None) and r["tables_grad_zero"], what
        assert r["counters"] == ([1, 0, 1] if rank is None else [1, 1, 1]), what  # (one process: no MLP bucket's own)
        assert r["rows_of"] == one["rows_of"], what
        for n, w in want_p.items():
            assert np.array_equal(r["params"][n], w), (what, n, int(np.sum(r["params"][n] != w)), "elements differ")
        assert np.array_equal(r["row_state"], want_acc), what
        assert _differ(r["params"], one["params"]) == [], what
    moved = [n for n, w in want_p.items() if not np.array_equal(w, sat.case.params[n])]
    assert len(moved) >= len(want_p) // 2 and want_acc.any()


# ------------------------------------------------------------------------------------------- refusals
def test_refusals(gpu):
    from xsdeepfwfm_deprecated_amd import DeepFMs
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, *_ = tc.case("fm_deep")
    m = build(cfg, params, gpu, is_deep_dropout=False)
    adag = dict(optimizer="adag", rowwise_tables=True)
    # with the keyword off, dist still raises today's NotImplementedError
    for kw in (adag, dict(adag, lazy_tables=True, lazy_exchange=True)):
        with pytest.raises(NotImplementedError, match="dfwfm_lazy_lists_span") as e:
            FusedTrainStep(m, 37, dist=FakeDist(), **kw)
        assert "ONE offset" in str(e.value) and "state pointer per span" in str(e.value)
    with pytest.raises(ValueError, match="needs dist"):
        FusedTrainStep(m, 37, rowwise_exchange=True, **adag)
    with pytest.raises(ValueError, match="needs rowwise_tables"):
        FusedTrainStep(m, 37, dist=FakeDist(), optimizer="adag", lazy_tables=True, rowwise_exchange=True)
    with pytest.raises(ValueError, match="needs sparse_exchange"):
        FusedTrainStep(m, 37, dist=FakeDist(), rowwise_exchange=True, sparse_exchange=False, **adag)
    with pytest.raises(ValueError, match="optimizer='adag'"):
        FusedTrainStep(m, 37, dist=FakeDist(), rowwise_tables=True, rowwise_exchange=True, optimizer="rmsp")
    # fit(): the switch without a process group, without rowwise_adagrad, or off the fused step
    sizes = [1] * 13 + [7] * 26
    xi = np.zeros((64, 26, 1), np.int64)
    xv = np.ones((64, 13), np.float32)
    y = (np.arange(64) % 2).astype(np.float32)
    for rowwise_adagrad, fused_fit in ((True, True), (False, True), (True, False)):
        net = DeepFMs(field_size=39, feature_sizes=sizes, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1, n_epochs=1,
                      batch_size=32, h_depth=1, deep_nodes=16, optimizer_type="adag").to(gpu)
        net.fused_optimizer = True
        net.rowwise_adagrad, net.fused_fit, net.rowwise_exchange = rowwise_adagrad, fused_fit, True
        with pytest.raises(ValueError, match="rowwise_exchange" if fused_fit else "rowwise_adagrad"):
            net.fit(xi, xv, y, [], [], [])
