"""GPU: the row-lazy table optimizers under data parallelism (FusedTrainStep(lazy_exchange=True),
include/dfwfm_lazy_lists.h), on spawned ranks that share cuda:0 (at most three GPU processes at once).

Two gloo ranks (step 1 eager, steps 2 and 3 replayed graph pieces, step 4 a partial batch) on the 64-row train goldens,
32 rows per rank, deterministic: replicas bit-identical (state arrays included), the tables' gradient region all zero
after every step, rows no rank touched keep their bits, and where the lazy and the dense update coincide by the lazy
contracts -- Adam with weight_decay 0 after step 1, plain SGD and Adagrad with weight_decay 0 after 3 steps -- every
tensor and state array_equal to the dense data-parallel step's.  A world-size-1 RCCL group (collectives inside the
step's graph, and between its graphs): three deterministic lazy steps equal the one-process lazy trainer bit for bit.
The refusals.  fit() on two gloo ranks.

Each spawned job runs once per module (a fixture); the tests assert on what it returned."""
import hashlib
import os

import numpy as np
import pytest
import torch

import train_cases as tc
from conftest import load_train_golden
from test_gpu_train import build

pytestmark = pytest.mark.gpu

NAMES = ["train_deepfwfm_lw", "train_qr_mult"]
G, BS = 64, 32
SCHEDULE = [(1, 1e-4), (3, 1e-3)]
# key -> (FusedTrainStep keywords, steps); "_dense" runs are the dense data-parallel step a lazy run is compared with
RUNS = {
    "adam": (dict(lazy_table_adam=True, lazy_exchange=True, weight_decay=0.0), 3),
    "adam_dense": (dict(weight_decay=0.0), 1),
    "sgd": (dict(optimizer="sgd", lazy_tables=True, lazy_exchange=True, weight_decay=0.0), 3),
    "sgd_dense": (dict(optimizer="sgd", weight_decay=0.0), 3),
    "adag": (dict(optimizer="adag", lazy_tables=True, lazy_exchange=True, weight_decay=0.0), 3),
    "adag_dense": (dict(optimizer="adag", weight_decay=0.0), 3),
    "sgdm": (dict(optimizer="sgd", momentum=0.9, lazy_tables=True, lazy_exchange=True, weight_decay=3e-7), 3),
    "rmsp": (dict(optimizer="rmsp", lazy_tables=True, lazy_exchange=True, weight_decay=3e-7), 3),
    "adam_sched": (dict(lazy_table_adam=True, lazy_exchange=True, weight_decay=3e-7, lr_schedule=SCHEDULE), 3),
}
LAZY_RUNS = [k for k in RUNS if not k.endswith("_dense")]
# lazy run -> (dense run, the step after which the two coincide bit for bit)
COINCIDE = {"adam": ("adam_dense", 1), "sgd": ("sgd_dense", 3), "adag": ("adag_dense", 3)}


def _port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ------------------------------------------------------------------------------------------- what a rank runs
def _snap(m, t, logits=None):
    """Every tensor and state array of a trainer, on the host."""
    s = {"p/" + n: p.detach().cpu().numpy().copy() for n, p in m.named_parameters()}
    for k in ("exp_avg", "exp_avg_sq", "opt_state"):
        a = getattr(t, k)
        if a is not None:
            s["s/" + k] = a.detach().cpu().numpy().copy()
    if logits is not None:
        s["logits"] = logits
    return s


def _digest(s):
    h = hashlib.sha256()
    for k in sorted(s):
        h.update(k.encode())
        h.update(np.ascontiguousarray(s[k]).tobytes())
    return h.hexdigest()


def _differ(a, b):
    """Names of the arrays of two snapshots that are not array_equal."""
    assert set(a) == set(b)
    return sorted(k for k in a if not np.array_equal(a[k], b[k]))


def _table_rows(m, xi):
    """name -> the sorted rows of each categorical table that the keys xi [n, ncat] touch (plain: the key; QR:
    key // c in the quotient table and key % c in the remainder table)."""
    fields, _ = m._param_layout()
    names = {id(p): n for n, p in m.named_parameters()}
    out = {}
    for f in range(m.num, m.field_size):
        e2, e2r, e1, e1r = fields[f]
        k = xi[:, f - m.num]
        for q, r, bags in ((e2, e2r, m.fm_2nd_embeddings if e2 is not None else None),
                           (e1, e1r, m.fm_1st_embeddings if e1 is not None else None)):
            if q is None:
                continue
            if r is None:
                out[names[id(q)]] = np.unique(k)
            else:
                c = int(bags[f].num_collisions)
                out[names[id(q)]] = np.unique(k // c)
                out[names[id(r)]] = np.unique(k % c)
    return out


def _steps(name, kw, steps, dist, rank, world, partial=False):
    """`steps` deterministic FusedTrainSteps on the 64-row global batches of train golden `name`, this rank taking its
    contiguous share (then, with `partial`, a 49-row global batch: 32 rows on rank 0, 17 on rank 1).  Returns the
    snapshots after every step and what was checked on the way."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, xi, xv, y, *_ = load_train_golden(name)
    dev = torch.device("cuda:0")
    bs = G // world
    m = build(cfg, params, dev, is_deep_dropout=False)
    t = FusedTrainStep(m, bs, **dict(dict(lr=1e-3, dist=dist, deterministic=True), **kw))
    start = _snap(m, t)
    snaps, grad_zero = {}, []
    plan = [(k * G, G) for k in range(steps)] + ([(steps * G, 49)] if partial else [])
    for k, (g0, n_global) in enumerate(plan, 1):
        lo = min(g0 + n_global, g0 + rank * bs)
        hi = min(g0 + n_global, lo + bs)
        xb, vb, yb = (torch.from_numpy(a[lo:hi]).to(dev) for a in (xi, xv, y))
        t.step(xb, vb, yb, n_global if dist is not None else None)
        torch.cuda.synchronize()
        nz = torch.nonzero(t.grad[:t.n_tables]).flatten()
        grad_zero.append(nz.numel() == 0 or (int(nz.numel()), nz[:4].tolist()))  # (on a failure: how many, where)
        snaps[k] = _snap(m, t, t.out[:hi - lo].detach().cpu().numpy().copy())
    # (the replicas' digest is over the tensors and state arrays: each rank has its own rows' logits)
    info = {"grad_zero": grad_zero,
            "digest": {k: _digest({n: a for n, a in s.items() if n != "logits"}) for k, s in snaps.items()},
            "lazy_lists": bool(getattr(t, "lazy_lists", False)), "counters": [
                int(c[0].item()) for c in (t.state, t.state_b, t.state_t)], "graphs": t.graphs is not None}
    if getattr(t, "lazy_lists", False):
        # rows of the tables that no rank's slice of any batch touched keep their bits, in the tensor and in the state
        touched = _table_rows(m, xi[:plan[-1][0] + plan[-1][1]])
        last = snaps[len(plan)]
        offs = {id(p): o for p, o in zip(t.params, t.offs)}
        bad, n_untouched, n_changed = [], 0, 0
        for n, p in m.named_parameters():
            if n not in touched:
                continue
            rest = np.setdiff1d(np.arange(p.shape[0]), touched[n])
            n_untouched += len(rest)
            if not np.array_equal(last["p/" + n][rest], start["p/" + n][rest]):
                bad.append(n)
            n_changed += int(not np.array_equal(last["p/" + n][touched[n]], start["p/" + n][touched[n]]))
            for k in ("s/exp_avg", "s/exp_avg_sq", "s/opt_state"):
                if k in last:
                    rows = last[k][offs[id(p)]:offs[id(p)] + p.numel()].reshape(p.shape[0], -1)
                    if rows[rest].any():
                        bad.append(n + " " + k)
        info.update(untouched_changed=bad, n_untouched=n_untouched, tables_changed=n_changed, n_tables=len(touched))
    t.close()
    return snaps, info


def _fit_two_ranks():
    """fit() under the two switches on the small synthetic set of test_fit_with_lazy_table_adam_learns."""
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
    log = logging.getLogger("test_lazy_exchange_fit")
    log.setLevel(logging.INFO)
    log.propagate = False
    log.addHandler(Keep())
    m = DeepFMs(field_size=39, feature_sizes=sizes, use_fwfm=1, use_fm=0, use_deep=1, use_lw=1, n_epochs=3,
                batch_size=256, learning_rate=1e-2, weight_decay=3e-7, h_depth=2, deep_nodes=64, logger=log,
                random_seed=3).to("cuda:0")
    m.lazy_table_adam = True
    m.lazy_exchange = True
    m.fit(xi.reshape(-1, 26, 1), xv, y, [], [], [])
    torch.cuda.synchronize()
    losses = [float(s.split("loss:")[1].split()[0]) for s in lines if s.startswith("Training [")]
    return losses, _digest({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()})


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {}
        for name in NAMES:
            snaps = {}
            for key, (kw, steps) in RUNS.items():
                snaps[key], res[name, key] = _steps(name, kw, steps, dist, rank, world,
                                                    partial=not key.endswith("_dense"))
            for key, (dense, step) in COINCIDE.items():
                res[name, key]["differs_from_dense"] = _differ(snaps[key][step], snaps[dense][step])
                res[name, key]["moved"] = len(_differ(snaps[key][step], snaps[key][step + 1]))
        res["fit"] = _fit_two_ranks()
        q.put((rank, "ok", res))
    except Exception as e:  # report, do not hang the parent
        import traceback
        q.put((rank, "error", repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _rccl_worker(port, q):
    """A world-size-1 RCCL group: the lazy data-parallel step (collectives inside the step's graph, then between its
    graphs) against the one-process lazy trainer in the same process."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        res = {}
        for opt, kw in (("adam", dict(lazy_table_adam=True, weight_decay=3e-7)),
                        ("adag", dict(optimizer="adag", lazy_tables=True, weight_decay=3e-7))):
            one, _ = _steps(NAMES[0], kw, 3, None, 0, 1)
            for graph_comm in (True, False):
                os.environ["DFWFM_DP_GRAPH_COMM"] = "1" if graph_comm else "0"
                dp, info = _steps(NAMES[0], dict(kw, lazy_exchange=True), 3, dist, 0, 1)
                info["differs_from_one_process"] = {k: _differ(dp[k], one[k]) for k in dp}
                info["moved"] = len(_differ(dp[1], dp[3]))
                res[opt, graph_comm] = info
        q.put(("ok", res))
    except Exception as e:  # report, do not hang the parent
        import traceback
        q.put(("error", repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------- the jobs, run once
@pytest.fixture(scope="module")
def gloo(gpu):
    import torch.multiprocessing as mp
    port = _port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(60)
    for rank, status, res in got:
        assert status == "ok", (rank, res)
    assert all(p.exitcode == 0 for p in procs)
    return {rank: res for rank, _, res in got}


@pytest.fixture(scope="module")
def rccl(gpu):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_port(), q))
    p.start()
    status, res = q.get(timeout=300)
    p.join(60)
    assert status == "ok", res
    assert p.exitcode == 0
    return res


# ------------------------------------------------------------------------------------------- two gloo ranks
@pytest.mark.parametrize("key", LAZY_RUNS)
@pytest.mark.parametrize("name", NAMES)
def test_replicas_are_bit_identical_and_the_tables_gradient_stays_zero(gloo, name, key):
    """After every step (1 eager, 2 and 3 graph replays, 4 a partial batch) the two ranks hold the same bits in every
    tensor and state array, the tables' region of the gradient buffer is all zero, all three counters stand at the
    step, and the lists update ran (nothing fell back to another path)."""
    a, b = gloo[0][name, key], gloo[1][name, key]
    assert a["lazy_lists"] and b["lazy_lists"] and a["graphs"]
    assert a["digest"] == b["digest"] and len(a["digest"]) == 4
    assert len(set(a["digest"].values())) == 4  # and every step moved something
    assert a["grad_zero"] == [True] * 4 and b["grad_zero"] == [True] * 4
    assert a["counters"] == [4, 4, 4] and b["counters"] == [4, 4, 4]


@pytest.mark.parametrize("key", LAZY_RUNS)
@pytest.mark.parametrize("name", NAMES)
def test_rows_no_rank_touched_keep_their_bits(gloo, name, key):
    for rank in (0, 1):
        r = gloo[rank][name, key]
        assert r["untouched_changed"] == []
        assert r["n_untouched"] > 1000 and r["tables_changed"] >= r["n_tables"] // 2 > 0  # (and the touched ones moved)


@pytest.mark.parametrize("key", sorted(COINCIDE))
@pytest.mark.parametrize("name", NAMES)
def test_lazy_step_equals_dense_data_parallel_step_where_they_coincide(gloo, name, key):
    """Adam with weight_decay 0 after step 1, plain SGD and Adagrad with weight_decay 0 after 3 steps: every tensor,
    moment / state array and logit array_equal to the dense data-parallel step's (exact by the lazy contracts: no
    tolerance)."""
    for rank in (0, 1):
        r = gloo[rank][name, key]
        assert r["differs_from_dense"] == []
        assert r["moved"] > 10  # (the compared snapshot is not the last word: the next step moves most tensors)
        assert not gloo[rank][name, COINCIDE[key][0]]["lazy_lists"]  # the dense run was the dense step


def test_fit_two_ranks_under_the_switches_learns_with_identical_replicas(gloo):
    (l0, d0), (l1, d1) = gloo[0]["fit"], gloo[1]["fit"]
    assert d0 == d1
    assert len(l0) == 3 and l0[-1] < l0[0], l0
    assert l0 == l1


# ------------------------------------------------------------------------------------------- RCCL, world size 1
@pytest.mark.parametrize("graph_comm", [True, False], ids=["in-graph", "between-graphs"])
@pytest.mark.parametrize("opt", ["adam", "adag"])
def test_rccl_world_one_lazy_exchange_equals_one_process_lazy_trainer(rccl, opt, graph_comm):
    """Three deterministic lazy steps through the exchange equal the one-process lazy trainer bit for bit: parameters,
    moments or state, logits, after every step."""
    r = rccl[opt, graph_comm]
    assert r["lazy_lists"] and r["graphs"]
    assert r["differs_from_one_process"] == {1: [], 2: [], 3: []}
    assert r["grad_zero"] == [True] * 3 and r["counters"] == [3, 3, 3] and r["moved"] > 10
    assert r["untouched_changed"] == [] and r["n_untouched"] > 1000


# ------------------------------------------------------------------------------------------- refusals
class FakeDist:  # refused before it is asked anything
    pass


def test_refusals(gpu):
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, *_ = tc.case("fm_deep")
    m = build(cfg, params, gpu, is_deep_dropout=False)
    for kw, switch in ((dict(lazy_table_adam=True), "lazy_table_adam"), (dict(lazy_tables=True), "lazy_tables"),
                       (dict(lazy_tables=True, optimizer="adag"), "lazy_tables")):
        with pytest.raises(NotImplementedError, match=switch) as e:
            FusedTrainStep(m, 37, dist=FakeDist(), **kw)
        assert "lazy_exchange" in str(e.value)
    with pytest.raises(ValueError, match="needs dist"):
        FusedTrainStep(m, 37, lazy_table_adam=True, lazy_exchange=True)
    with pytest.raises(ValueError, match="lazy_table_adam or lazy_tables"):
        FusedTrainStep(m, 37, dist=FakeDist(), lazy_exchange=True)
    with pytest.raises(ValueError, match="sparse_exchange"):
        FusedTrainStep(m, 37, dist=FakeDist(), lazy_tables=True, lazy_exchange=True, sparse_exchange=False)
    # a model whose only trainable parameters are tables: the one-process refusal
    fields, _ = m._param_layout()
    cat = {id(t) for f, tup in enumerate(fields) if f >= m.num for t in tup if t is not None}
    for p in m.parameters():
        p.requires_grad_(id(p) in cat)
    with pytest.raises(NotImplementedError, match="only trainable parameters are tables"):
        FusedTrainStep(m, 37, dist=FakeDist(), lazy_table_adam=True, lazy_exchange=True)
