"""GPU: the data-parallel training step on 3, 4 and 8 ranks and on ranks without rows (tests/dp_cases.py: the shard
plans; tests/test_dp_cases.py: the CPU leg), where the other modules spawn two ranks with one half of a batch each.

A. Emulated ranks through the C ABI, one process: per shard of a 129-row witness case dfwfm_train_forward on the
shard's rows, the backward's DFWFM_BWD_TABLES into a local buffer, dfwfm_sparse_grads_local for both families into
slot r of a [W, nbytes] buffer laid out by training.packed_layout; then dfwfm_sparse_grads_apply over all W slots in
rank order.  The tables' gradients are the float64 reference's of the WHOLE batch bit for bit, the local buffer is zero
after every call, every list counts its shard's distinct rows per table with unique destinations, and an empty shard
writes count 0 over the full list a previous call left in its slot.

B. Real ranks: gloo, every rank a spawned process on cuda:0, one fixture per world (3, 4, 8), run one after the other.
B1: FusedTrainStep with plain SGD on the saturated witness case (128 rows): two rate-0 steps on full per-rank batches
(eager, then captured and replayed; every parameter keeps its bits), then one step at 2^-6 on fit()'s shards -- partial
and empty ranks take the eager path while their peers replay graphs -- after which every parameter on every rank is
p - 2^-6 g of the float64 reference on the global batch bit for bit, each rank's logits and dlogit are the reference's
rows and the ranks' loss sums add up to the reference's; with the touched-row exchange (sorted and atomic), the dense
all-reduce, and the list-driven lazy update.  B2: Adam and Adagrad on the train goldens, dense and lazy: three full
global batches and a 20-row one that leaves ranks empty; replicas array_equal on every rank after every step (moments
and state included), step-1 gradients and logits against one process on the global batch at the world-2 test's bars,
and the lazy runs' contracts.

Both legs run again with the deep tower's dropout 0.5 on (the model's default): the reference is then the float64 one
of the whole batch under the masks the ranks drew, rebuilt on the host from each rank's seed, the device counter and
its LOCAL row index (dc.shard_masks).  A: every plan on every model, a seed per emulated rank, both training forwards,
the MLP's weight gradients too.  B1: 43/43/42, 48/48/32/0 and 8 x 16 in all four modes inside the same jobs, the
rate-0 steps' logits under counters 0 and 1 included; and the same step through a world-size-1 RCCL group with the
collectives captured into the step's graph.  B2: Adam, dense and lazy, on the small-MLP golden against CPU steps under
the ranks' masks.  The ranks' seeds differ (training.rank_seed).

Each spawned job runs once per module (a fixture); the tests assert on what it returned."""
import ctypes
import functools
import hashlib
import os
import queue

import numpy as np
import pytest
import torch

import dp_cases as dc
import exact_train_cases as xc
import train_cases as tc
from conftest import load_train_golden, logit_close
from test_gpu_exact_train import Abi, _writable
from test_gpu_train import G_TOL, build

pytestmark = pytest.mark.gpu


# =================================================================================== A: shards through the C ABI
class Slots:
    """[W, nbytes] bytes on the device, one slot per emulated rank, laid out by training.packed_layout for the lists
    of both families at the capacity of the plan's largest shard."""

    def __init__(self, a, world, cap_batch):
        from xsdeepfwfm_deprecated_amd.training import packed_layout
        lib, m = a.lib, a.m
        self.fams = []
        for fam, (iq, ir) in ((lib.FAMILY_SECOND, (0, 1)), (lib.FAMILY_FIRST, (2, 3))):
            o = lambda t: -1 if t is None else a.off[id(t)]  # noqa: E731
            dest = (lib.dfwfm_sparse_dest * len(a.fields))(
                *[lib.dfwfm_sparse_dest(o(tup[iq]) if f >= m.num else -1, o(tup[ir]) if f >= m.num else -1)
                  for f, tup in enumerate(a.fields)])
            cap, w, wsb = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
            lib.check(a.L.dfwfm_sparse_grads_size(a.eng.handle, fam, cap_batch, ctypes.byref(cap), ctypes.byref(w),
                                                  ctypes.byref(wsb)), "size")
            if cap.value > 0:
                self.fams.append(dict(fam=fam, dest=dest, cap=int(cap.value), w=int(w.value)))
        self.nbytes = packed_layout(self.fams)
        self.buf = torch.zeros(world, self.nbytes, dtype=torch.uint8, device=a.gpu)
        assert self.buf.data_ptr() % 16 == 0 and self.nbytes % 16 == 0

    def ptrs(self, r, f):
        base = self.buf.data_ptr() + r * self.nbytes
        return tuple(ctypes.c_void_p(base + f[k]) for k in ("o_dest", "o_rows", "o_cnt"))

    def lists(self, r):
        """[(family, count, destinations[:count])] of slot r, on the host."""
        host = self.buf[r].cpu().numpy()
        out = []
        for f in self.fams:
            n = int(host[f["o_cnt"]:f["o_cnt"] + 4].view(np.int32)[0])
            assert 0 <= n <= f["cap"]
            out.append((f, n, host[f["o_dest"]:f["o_dest"] + 8 * f["cap"]].view(np.int64)[:n].copy()))
        return out


def _local_lists(a, slots, r, case, XI, XV, DL, lo, hi, det, stamp, seed=None):
    """One emulated rank: forward on rows lo .. hi - 1 (the slices' pointers) -- seed: with dropout 0.5 from that
    seed, the rank's own --, DFWFM_BWD_TABLES with the categorical tables scattered into the local buffer, then both
    families' lists into slot r."""
    a.eng.set_deterministic(det)
    a.xi, a.xv, a.dl = XI[lo:hi], XV[lo:hi], DL[lo:hi]  # kept alive: the backward re-reads them
    a.out = torch.empty(hi - lo, device=a.gpu)
    a.eng.train_forward(a.xi, a.xv, a.out, 0.0 if seed is None else 0.5, case.seed if seed is None else seed)
    a.phases(a.lib.BWD_TABLES)
    if seed is not None:  # the MLP's weight gradients too, added into the flat buffer shard after shard
        a.phases(a.lib.BWD_MLP_WEIGHTS)
    for f in slots.fams:
        od, orow, cnt = slots.ptrs(r, f)
        a.lib.check(a.L.dfwfm_sparse_grads_local(a.eng.handle, f["fam"], f["dest"], f["cap"],
                                                 ctypes.c_void_p(a.local.data_ptr()), ctypes.c_void_p(stamp.data_ptr()),
                                                 a.local.numel(), od, orow, cnt, a.stream()), "local lists")
    torch.cuda.synchronize()
    assert not bool(a.local.any()), ("local buffer not zero after the lists of rank", r)
    return a.out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _model(gpu, name):
    """One model per case for the module; the shards read its parameters, none writes them."""
    case = dc.a_case(name)
    return build(case.cfg, _writable(case.params), gpu, is_deep_dropout=True)


def _table_of(a, case):
    """[(offset, floats, rows, name)] of the categorical tables in the flat buffer."""
    names = set(dc.table_names(case))
    return sorted((a.off[id(p)], p.numel(), int(p.shape[0]), k) for k, p in a.m.named_parameters() if k in names)


@pytest.mark.parametrize("det", [True, False], ids=["sorted", "atomic"])
@pytest.mark.parametrize("plan", list(dc.A_PLANS))
@pytest.mark.parametrize("model", dc.A_MODELS)
def test_shards_through_the_c_abi(gpu, model, plan, det):
    _shards_through_the_c_abi(gpu, model, plan, det, dc.a_case(model), None)


# dropout: the base model has both training forwards (ftrain_kernel, and fwd_kernel<TRAIN> under DFWFM_DIAG=ftrain=0);
# the 2 x 64 variants have fwd_kernel<TRAIN> alone
A_DROP = [(m, "default") for m in dc.A_MODELS] + [("base", "fwd_kernel")]


@pytest.mark.parametrize("det", [True, False], ids=["sorted", "atomic"])
@pytest.mark.parametrize("plan", list(dc.A_PLANS))
@pytest.mark.parametrize("model,fwd", A_DROP)
def test_shards_through_the_c_abi_with_dropout(gpu, monkeypatch, model, fwd, plan, det):
    """The same with dropout 0.5, every emulated rank on a seed of its own (dc.SEEDS) and no step source attached:
    the logits, the applied table gradients and the dense gradients summed over the ranks are the float64 reference's
    of the WHOLE batch under the ranks' masks one after the other (dc.shard_masks: each rank's over its local rows
    from 0), bit for bit -- on both training forwards, the sorted and the atomic scatter, with 1-row and 0-row
    shards."""
    if fwd == "fwd_kernel":
        monkeypatch.setenv("DFWFM_DIAG", "ftrain=0")
    world, _ = dc.A_PLANS[plan]
    _shards_through_the_c_abi(gpu, model, plan, det, dc.a_drop_case(model, plan), dc.SEEDS[:world])


def _shards_through_the_c_abi(gpu, model, plan, det, case, seeds):
    world, bs = dc.A_PLANS[plan]
    shards = dc.fit_shards(dc.A_B, bs, world)
    assert [hi - lo for lo, hi in shards] == dc.A_SIZES[plan]
    a = Abi(_model(gpu, model), gpu, local=True)
    slots = Slots(a, world, max(dc.A_SIZES[plan]))
    stamp = torch.zeros(a.flat.numel() + 1, dtype=torch.int32, device=gpu)
    XI, XV, DL = (torch.from_numpy(x.copy()).to(gpu) for x in (case.xi, case.xv, case.dlogit))
    tables = _table_of(a, case)
    # a previous step's full list in the slot of every rank that holds no rows now: from a call, not written by hand
    empty = [r for r, (lo, hi) in enumerate(shards) if hi == lo]
    for r in empty:
        _local_lists(a, slots, r, case, XI, XV, DL, *shards[0], det, stamp, seeds and seeds[r])
        assert all(n > 0 for _, n, _ in slots.lists(r)), "no stale list to reset"
    a.flat.zero_()  # (what those backwards wrote outside the tables)
    z32, g32 = xc.ref32(case)
    fam_names = {a.lib.FAMILY_SECOND: "fm_2nd_embeddings", a.lib.FAMILY_FIRST: "fm_1st_embeddings"}
    for r, (lo, hi) in enumerate(shards):
        out = _local_lists(a, slots, r, case, XI, XV, DL, lo, hi, det, stamp, seeds and seeds[r])
        assert np.array_equal(out, z32[lo:hi]), (r, "logits")
        want = dc.touched(case, lo, hi)
        for f, n, dest in slots.lists(r):
            assert len(np.unique(dest)) == n, (r, "a destination twice in one list")
            if hi == lo:
                assert n == 0, (r, "an empty shard left its slot's previous list in place", n)
            per_table = {k: 0 for k in want if k.startswith(fam_names[f["fam"]])}
            for off, numel, rows, k in tables:
                if k in per_table:
                    mine = dest[(dest >= off) & (dest < off + numel)]
                    assert np.all((mine - off) % f["w"] == 0)
                    assert np.array_equal(np.sort((mine - off) // f["w"]), want[k]), (r, k, "rows of the list")
                    per_table[k] = len(mine)
            assert sum(per_table.values()) == n == sum(len(want[k]) for k in per_table), (r, f["fam"])
    for r in range(world):  # every rank's lists, in rank order, into the zero tables of the flat buffer
        for f in slots.fams:
            od, orow, cnt = slots.ptrs(r, f)
            a.lib.check(a.L.dfwfm_sparse_grads_apply(ctypes.c_void_p(a.flat.data_ptr()), f["w"], od, orow, cnt,
                                                     f["cap"], a.stream()), "apply")
    got = a.result()
    listed = {k for k in dc.table_names(case) if any(k.startswith(fam_names[f["fam"]]) for f in slots.fams)}
    for k in dc.table_names(case):
        assert k in listed or not np.any(g32[k]), (k, "a table with a gradient and no list")
        assert np.array_equal(got[k], g32[k]), (plan, k, int(np.sum(got[k] != g32[k])), "elements differ")
    # what DFWFM_BWD_TABLES adds straight into the flat buffer, shard after shard, is the whole batch's too
    for k, v in g32.items():
        if k not in listed and (seeds is not None or not k.startswith("net_1_linear_")):
            assert np.array_equal(got[k], v), (plan, k, "accumulated over the shards")


# =================================================================================== B: real ranks
B1_MODES = {
    "sparse-sorted": dict(sparse_exchange=True, deterministic=True),
    "sparse-atomic": dict(sparse_exchange=True, deterministic=False),
    "dense": dict(sparse_exchange=False, deterministic=True),
    "lazy": dict(lazy_tables=True, lazy_exchange=True, deterministic=True),
}
NAMES = ["train_deepfwfm_lw", "train_qr_mult"]
# key -> (FusedTrainStep keywords); "_dense" runs are the dense data-parallel step a lazy run is compared with
B2_RUNS = {
    "adam_dense": dict(weight_decay=0.0),
    "adam": dict(lazy_table_adam=True, lazy_exchange=True, weight_decay=0.0),
    "adag_dense": dict(optimizer="adag", weight_decay=0.0),
    "adag": dict(optimizer="adag", lazy_tables=True, lazy_exchange=True, weight_decay=0.0),
}
COINCIDE = {"adam": ("adam_dense", 1), "adag": ("adag_dense", 3)}  # lazy run -> (dense run, the step compared)
B2_DROP_NAME, B2_DROP_RUNS = "train_small_mlp", ("adam_dense", "adam")  # with dropout: a deep tower of 2 x 64
WORLDS = sorted(dc.B2_WORLDS)


def _port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _send_counts(t):
    """The counts of the lists in a trainer's send buffer (None without the touched-row exchange)."""
    if not t.sparse:
        return None
    return [int(t.sp_send[f["o_cnt"]:f["o_cnt"] + 4].view(torch.int32).item()) for f in t.sp_fams]


def _b1_run(plan, mode, dist, rank, drop=False):
    """Two rate-0 steps on the rank's full rate-0 batch, then the measured step on fit()'s shard: host arrays.  drop:
    the model's default, deep-tower dropout 0.5 on; the rank reports the seed its trainer drew."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    sat = xc.saturated()
    case = sat.case
    dev = torch.device("cuda:0")
    world, bs = dc.b1_plan(plan)
    m = build(case.cfg, _writable(case.params), dev, is_deep_dropout=drop)
    t = FusedTrainStep(m, bs, optimizer="sgd", momentum=0.0, weight_decay=0.0, lr_schedule=[(1, 0.0)], dist=dist,
                       **B1_MODES[mode])
    rate0 = []

    def step(rows):
        xi, xv, y = (torch.from_numpy(np.array(x[rows])).to(dev) for x in (case.xi, case.xv, sat.y))
        t.step(xi, xv, y, xc.SAT_B)

    t.set_lr(0.0)
    rows0 = dc.rate0_rows(rank, bs, xc.SAT_B)
    for _ in range(2):  # eager; then captured and replayed
        step(rows0)
        if drop:  # (the dropout-off run keeps its two steps back to back)
            rate0.append(t.out[:bs].cpu().numpy().copy())
    torch.cuda.synchronize()
    res = {"seed": int(t.seed), "drop": float(t.drop), "rate0_logits": rate0,
           "moved_at_rate_0": [k for k, q in m.named_parameters()
                               if not np.array_equal(q.detach().cpu().numpy(), case.params[k])],
           "captured": t.graphs is not None, "counts_before": _send_counts(t)}
    t.set_lr(xc.SGD_LR)
    t.loss_sum.zero_()  # (the trainer's loss sum runs over its steps)
    lo, hi = dc.fit_shards(xc.SAT_B, bs, world)[rank]
    step(slice(lo, hi))
    torch.cuda.synchronize()
    res.update(params={k: q.detach().cpu().numpy().copy() for k, q in m.named_parameters()},
               logits=t.out[:hi - lo].cpu().numpy().copy(), dlogit=t.dlogit[:hi - lo].cpu().numpy().copy(),
               loss=float(t.loss_sum.item()), graph_sets=len(t._graph_sets), counts_after=_send_counts(t),
               lazy_lists=bool(t.lazy_lists), sparse=bool(t.sparse), counter=int(t.state[0].item()),
               tables_grad_zero=not bool(t.grad[:t.n_tables].any()))
    t.close()
    return res


def _hashes(m, t):
    """{name: sha256} of every tensor and state array of a trainer, and the arrays themselves."""
    s = {"p/" + n: p.detach().cpu().numpy().copy() for n, p in m.named_parameters()}
    for k in ("exp_avg", "exp_avg_sq", "opt_state"):
        a = getattr(t, k)
        if a is not None:
            s["s/" + k] = a.detach().cpu().numpy().copy()
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in s.items()}, s


def _b2_rows(lo, hi, n):
    """Rows lo .. hi - 1 of a golden of n rows, taken cyclically (the small-MLP golden holds 128)."""
    return np.arange(lo, hi) % n


def _b2_steps(name, kw, dist, rank, world, g, bs, drop=False):
    """Deterministic FusedTrainSteps on train golden `name`: three global batches of g rows (step 1 eager, 2 and 3
    replayed), then one of 20 rows, this rank taking fit()'s shard.  dist None: one process on the global batch.
    drop: deep-tower dropout 0.5 on; the rank reports its seed and its parameters after step 3."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, xi, xv, y, *_ = load_train_golden(name)
    dev = torch.device("cuda:0")
    m = build(cfg, params, dev, is_deep_dropout=drop)
    t = FusedTrainStep(m, bs, **dict(dict(lr=1e-3, dist=dist, deterministic=True), **kw))
    _, start = _hashes(m, t)
    plan = [(k * g, g) for k in range(3)] + [(3 * g, dc.B2_PARTIAL)]
    res = {"hashes": {}, "logits": {}, "grad_zero": [], "rows": []}
    snaps = {}
    for k, (g0, n_global) in enumerate(plan, 1):
        lo, hi = dc.fit_shards(n_global, bs, world, g0)[rank]
        xb, vb, yb = (torch.from_numpy(a[_b2_rows(lo, hi, len(xi))]).to(dev) for a in (xi, xv, y))
        t.step(xb, vb, yb, n_global if dist is not None else None)
        torch.cuda.synchronize()
        if k == 1:
            res["grads"] = {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()}
        res["grad_zero"].append(not bool(t.grad[:t.n_tables].any()))
        res["rows"].append(hi - lo)
        res["logits"][k] = t.out[:hi - lo].detach().cpu().numpy().copy()
        res["hashes"][k], snaps[k] = _hashes(m, t)
    if drop:
        res.update(seed=int(t.seed), drop=float(t.drop),
                   params3={n[2:]: v for n, v in snaps[3].items() if n[:2] == "p/"})
    res.update(lazy_lists=bool(t.lazy_lists), graphs=t.graphs is not None,
               counters=[int(c[0].item()) for c in (t.state, t.state_b, t.state_t)])
    if t.lazy_lists:
        # rows of the tables that no rank's shard of any batch touched keep their bits, in the tensor and in the state
        last, offs = snaps[len(plan)], {id(p): o for p, o in zip(t.params, t.offs)}
        bad, n_untouched, n_changed, n_tables = [], 0, 0, 0
        named = dict(m.named_parameters())
        for n, mask in tc.table_rows(cfg, xi[_b2_rows(0, plan[-1][0] + plan[-1][1], len(xi))]).items():
            if n not in named:
                continue
            p = named[n]
            mask = np.isin(np.arange(p.shape[0]), np.flatnonzero(mask))  # (at the tensor's own row count)
            rest = np.flatnonzero(~mask)
            n_tables += 1
            n_untouched += len(rest)
            if not np.array_equal(last["p/" + n][rest], start["p/" + n][rest]):
                bad.append(n)
            n_changed += int(not np.array_equal(last["p/" + n][mask], start["p/" + n][mask]))
            for s in ("s/exp_avg", "s/exp_avg_sq", "s/opt_state"):
                if s in last and last[s][offs[id(p)]:offs[id(p)] + p.numel()].reshape(p.shape[0], -1)[rest].any():
                    bad.append(n + " " + s)
        res.update(untouched_changed=bad, n_untouched=n_untouched, tables_changed=n_changed, n_tables=n_tables)
    t.close()
    return res, snaps


def _differ(a, b):
    assert set(a) == set(b)
    return sorted(k for k in a if not np.array_equal(a[k], b[k]))


def _rank_worker(rank, world, port, q):
    import torch.distributed as dist
    torch.set_num_threads(2)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {}
        for plan, (w, _) in dc.B1_PLANS.items():
            if w == world:
                for mode in B1_MODES:
                    res["b1", plan, mode] = _b1_run(plan, mode, dist, rank)
                    if plan in dc.B1_DROP_PLANS:
                        res["b1-drop", plan, mode] = _b1_run(plan, mode, dist, rank, drop=True)
        g, bs = dc.B2_WORLDS[world]
        for name in NAMES:
            snaps = {}
            for key, kw in B2_RUNS.items():
                res["b2", name, key], snaps[key] = _b2_steps(name, kw, dist, rank, world, g, bs)
                if key != "adam_dense":
                    del res["b2", name, key]["grads"]  # (a lazy run's are the same sums, its tables' rows zeroed)
            for key, (dense, step) in COINCIDE.items():
                res["b2", name, key]["differs_from_dense"] = _differ(snaps[key][step], snaps[dense][step])
                res["b2", name, key]["moved"] = len(_differ(snaps[key][step], snaps[key][step + 1]))
        snaps = {}
        for key in B2_DROP_RUNS:
            res["b2-drop", key], snaps[key] = _b2_steps(B2_DROP_NAME, B2_RUNS[key], dist, rank, world, g, bs, True)
            del res["b2-drop", key]["grads"]
            if rank:
                del res["b2-drop", key]["params3"]  # (replicas are compared by their hashes)
        res["b2-drop", "adam"]["differs_from_dense"] = _differ(snaps["adam"][1], snaps["adam_dense"][1])
        q.put((rank, "ok", res))
    except Exception as e:  # report, do not hang the parent
        import traceback
        q.put((rank, "error", repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _spawn(world, budget=420):
    """`world` fresh gloo ranks on cuda:0, once; on a timeout, a failed rank or a nonzero exit code every child is
    terminated and the fixture fails (no second try)."""
    import time
    import torch.multiprocessing as mp
    port = _port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    t0 = time.monotonic()
    for p in procs:
        p.start()
    got, failure = [], None
    try:
        while len(got) < world and failure is None:
            try:
                got.append(q.get(timeout=max(1.0, min(5.0, budget - (time.monotonic() - t0)))))
                if got[-1][1] != "ok":
                    failure = f"rank {got[-1][0]}: {got[-1][2]}"
            except queue.Empty:
                dead = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (None, 0)]
                if dead:
                    failure = f"ranks exited without a result: {dead}"
                elif time.monotonic() - t0 > budget:
                    failure = (f"no result from ranks {sorted(set(range(world)) - {g[0] for g in got})} within "
                               f"{budget} s: a rank hangs (in a collective?)")
        for p in procs:
            p.join(60 if failure is None else 0.1)
        if failure is None and any(p.exitcode != 0 for p in procs):
            failure = f"exit codes {[p.exitcode for p in procs]}"
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(10)
            if p.is_alive():
                p.kill()
    assert failure is None, failure
    print(f"world {world}: {time.monotonic() - t0:.1f} s")
    return {rank: res for rank, _, res in got}


def _world_fixture(world):
    @pytest.fixture(scope="module", name=f"world{world}")
    def spawned(gpu):
        return _spawn(world)
    return spawned


world3, world4, world8 = (_world_fixture(w) for w in WORLDS)  # one job per world, each run once, one after the other


@pytest.fixture
def ranks(request):
    """world -> {rank: results} of that world's job."""
    return lambda world: request.getfixturevalue(f"world{world}")


@pytest.fixture(scope="module")
def one_process(gpu):
    """(name, global batch) -> one process's results on the global batches (no exchange), computed once."""
    done = {}

    def get(name, g):
        if (name, g) not in done:
            done[name, g] = _b2_steps(name, B2_RUNS["adam_dense"], None, 0, 1, g, g)[0]
        return done[name, g]
    return get


B1_CASES = [(plan, mode) for plan in dc.B1_PLANS for mode in B1_MODES]


@pytest.mark.parametrize("plan,mode", B1_CASES)
def test_exact_step_on_the_saturated_case(ranks, plan, mode):
    """On every rank: nothing moved at rate 0; after the measured step every parameter is p - 2^-6 g of the float64
    reference on the 128-row global batch bit for bit, the rank's logits and dlogit are the reference's rows, and the
    ranks' loss sums add up to the reference's.  Ranks with a full shard replayed their graphs (one graph set, no
    recapture); partial and empty ranks ran eager beside them, an empty rank resetting the list it had sent before."""
    _assert_b1(ranks(dc.B1_PLANS[plan][0]), "b1", plan, mode, xc.saturated())


def _assert_b1(res, leg, plan, mode, sat):
    """test_exact_step_on_the_saturated_case's assertions on the runs res[rank][leg, plan, mode] against `sat`."""
    world, bs = dc.b1_plan(plan)
    want, (z32, _) = xc.sgd_ref(sat), xc.ref32(sat.case)
    shards = dc.fit_shards(xc.SAT_B, bs, world)
    assert [hi - lo for lo, hi in shards] == dc.B1_SIZES.get(plan, [bs])
    for rank, (lo, hi) in enumerate(shards):
        r = res[rank][leg, plan, mode]
        what = (leg, plan, mode, "rank", rank)
        assert r["drop"] == (0.5 if leg == "b1-drop" else 0.0) and r["counter"] == 3, what
        assert r["moved_at_rate_0"] == [] and r["captured"], what
        assert r["graph_sets"] == 1, what
        assert r["sparse"] == (mode != "dense") and r["lazy_lists"] == (mode == "lazy"), what
        if r["sparse"]:
            assert all(n > 0 for n in r["counts_before"]), (what, "no list before the measured step")
            assert all((n > 0) == (hi > lo) for n in r["counts_after"]), (what, r["counts_after"])
        if mode == "lazy":
            assert r["tables_grad_zero"], what
        assert np.array_equal(r["logits"], z32[lo:hi]), (what, "logits")
        assert np.array_equal(r["dlogit"], sat.case.dlogit[lo:hi]), (what, "dlogit")
        for k, w in want.items():
            got = r["params"][k]
            assert np.array_equal(got, w), (what, k, int(np.sum(got != w)), "elements differ")
    losses = [np.float32(res[rank][leg, plan, mode]["loss"]) for rank in range(world)]
    assert float(np.sum(losses, dtype=np.float64)) == sat.loss_sum, (leg, plan, mode, losses)
    assert all(v == 0 for v, (lo, hi) in zip(losses, shards) if hi == lo)


B1_DROP_CASES = [(plan, mode) for plan in dc.B1_DROP_PLANS for mode in B1_MODES]


def _seeds(res, key):
    return tuple(res[rank][key]["seed"] for rank in range(len(res)))


@pytest.mark.parametrize("plan,mode", B1_DROP_CASES)
def test_exact_step_on_the_saturated_case_with_dropout(ranks, plan, mode):
    """The same step with the model's default, deep-tower dropout 0.5, on: the reference is the float64 one of the
    global batch under the masks the ranks drew -- each rank's from the seed it reports, the device counter (2 in the
    measured step) and its LOCAL row index, one after the other (dc.shard_masks).  Every assertion of the dropout-off
    test holds against it bit for bit: a backward that rebuilt the masks of another step, layer or row, a rank whose
    counter fell behind or a rank on another rank's seed changes a bit (tests/test_dp_cases.py).  The two rate-0
    steps' logits are the reference's under counters 0 (the eager step) and 1 (the captured one)."""
    _assert_b1_drop(ranks(dc.B1_PLANS[plan][0]), plan, mode)


def _assert_b1_drop(res, plan, mode):
    world, _ = dc.b1_plan(plan)
    seeds = _seeds(res, ("b1-drop", plan, mode))
    assert dc.b1_certificate(plan, seeds) < xc.LIMIT, "the reported seeds' masks leave the witness's bound"
    _assert_b1(res, "b1-drop", plan, mode, dc.b1_drop_case(plan, seeds))
    for rank in range(world):
        for counter, got in enumerate(res[rank]["b1-drop", plan, mode]["rate0_logits"]):
            want = dc.rate0_logits(plan, rank, seeds[rank], counter)
            assert np.array_equal(got, want), (plan, mode, "rank", rank, "rate-0 step at counter", counter)


@pytest.mark.parametrize("world", WORLDS)
def test_ranks_draw_different_dropout_seeds(ranks, world):
    """The ranks of a world report pairwise different seeds (training.rank_seed): the masks are a function of the
    LOCAL row, so one seed on every rank would repeat one mask pattern W times over the global batch.  Rank 0 keeps
    the seed one process draws, and rank r holds rank_seed of it."""
    from xsdeepfwfm_deprecated_amd.training import rank_seed
    res = ranks(world)
    keys = [k for k in res[0] if k[0] in ("b1-drop", "b2-drop")]
    assert len(keys) >= 6
    for key in keys:
        seeds = _seeds(res, key)
        assert len(set(seeds)) == world, (key, seeds)
        assert list(seeds) == [rank_seed(seeds[0], r) for r in range(world)], (key, seeds)


@pytest.mark.parametrize("key", list(B2_RUNS))
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("world", WORLDS)
def test_replicas_are_bit_identical_on_every_rank(ranks, world, name, key):
    """After every step (1 eager, 2 and 3 graph replays, 4 the 20-row global batch that leaves ranks empty) all W
    ranks hold the same bits in every tensor and every state array; every step moved something; all three counters
    stand at the step (the dense step never launches on state_t)."""
    res = ranks(world)
    first = res[0]["b2", name, key]
    assert first["rows"][3] == dc.B2_PARTIAL_SIZES[world][0] and first["graphs"]
    for rank in range(world):
        r = res[rank]["b2", name, key]
        assert r["rows"] == [dc.B2_WORLDS[world][1]] * 3 + [dc.B2_PARTIAL_SIZES[world][rank]]
        lazy = not key.endswith("_dense")  # (the dense step has no launch of the tables' own: state_t stays 0)
        assert r["counters"] == [4, 4, 4 if lazy else 0] and r["lazy_lists"] == lazy, (rank, r["counters"])
        for k in range(1, 5):
            bad = sorted(n for n in first["hashes"][k] if r["hashes"][k][n] != first["hashes"][k][n])
            assert bad == [] and set(r["hashes"][k]) == set(first["hashes"][k]), (rank, "step", k, bad[:4])
    assert all(first["hashes"][k] != first["hashes"][k + 1] for k in range(1, 4))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("world", WORLDS)
def test_first_step_matches_one_process_on_the_global_batch(ranks, one_process, world, name):
    """Step-1 gradients on every rank to G_TOL of each tensor's largest entry, and the ranks' logits, concatenated,
    to 1e-5 * max(1, |ref|): the bars of the world-2 test."""
    res, ref = ranks(world), one_process(name, dc.B2_WORLDS[world][0])
    for key in B2_RUNS:
        got = np.concatenate([res[rank]["b2", name, key]["logits"][1] for rank in range(world)])
        assert got.shape == ref["logits"][1].shape and logit_close(got, ref["logits"][1]) < 1e-5, key
    for rank in range(world):
        g = res[rank]["b2", name, "adam_dense"]["grads"]
        assert set(g) == set(ref["grads"])
        for k, gs in ref["grads"].items():
            sc = np.abs(gs).max()
            assert np.abs(g[k] - gs).max() <= G_TOL * sc + 1e-12, (rank, k)


@pytest.mark.parametrize("key", sorted(COINCIDE))
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("world", WORLDS)
def test_lazy_runs_keep_their_contracts(ranks, world, name, key):
    """What the world-2 module asserts of the list-driven update, on every rank: the tables' gradient region zero after
    every step, rows no rank touched keep their bits, and every tensor and state array array_equal to the dense
    data-parallel step's where the two coincide (Adam after step 1, Adagrad after step 3; weight_decay 0)."""
    res = ranks(world)
    for rank in range(world):
        r = res[rank]["b2", name, key]
        assert r["grad_zero"] == [True] * 4, rank
        assert r["untouched_changed"] == [], rank
        assert r["n_untouched"] > 1000 and r["tables_changed"] >= r["n_tables"] // 2 > 0
        assert r["differs_from_dense"] == [], rank
        assert r["moved"] > 10  # (the compared snapshot is not the last word: the next step moves most tensors)
        assert not res[rank]["b2", name, COINCIDE[key][0]]["lazy_lists"]  # the dense run was the dense step


def _lazy_adam_steps(cfg, params, batches, lr, mask_fn, drop_p, betas=(0.9, 0.999), eps=1e-8):
    """torch_port.train_steps with the categorical tables on the lazy Adam (include/dfwfm_lazy_adam.h: a table row
    that the step's batch does not read keeps its value and its moments; a row it reads takes Adam's step at the
    global step count), everything else on Adam as torch.optim.Adam computes it, weight_decay 0; float32 on the CPU."""
    from oracle import torch_port
    import torch.nn.functional as F
    leaf = {k: torch.tensor(v, requires_grad=True) for k, v in params.items()}
    m1 = {k: torch.zeros_like(v) for k, v in leaf.items()}
    m2 = {k: torch.zeros_like(v) for k, v in leaf.items()}
    for k, (Xi, Xv, y) in enumerate(batches):
        for v in leaf.values():
            v.grad = None
        out = torch_port.forward_graph(cfg, leaf, torch.as_tensor(Xi), torch.as_tensor(Xv), mask_fn(k, len(Xi)), drop_p)
        F.binary_cross_entropy_with_logits(out, torch.as_tensor(y, dtype=torch.float32)).backward()
        rows = tc.table_rows(cfg, Xi)
        bc1, bc2 = 1.0 - betas[0] ** (k + 1), 1.0 - betas[1] ** (k + 1)
        with torch.no_grad():
            for n, p in leaf.items():
                g = torch.zeros_like(p) if p.grad is None else p.grad
                on = slice(None)
                if n in rows:
                    on = torch.as_tensor(np.isin(np.arange(p.shape[0]), np.flatnonzero(rows[n])))
                m1[n][on] = betas[0] * m1[n][on] + (1.0 - betas[0]) * g[on]
                m2[n][on] = betas[1] * m2[n][on] + (1.0 - betas[1]) * g[on] * g[on]
                p[on] -= (lr / bc1) * m1[n][on] / (m2[n][on].sqrt() / np.sqrt(bc2) + eps)
    return {k: v.detach().numpy() for k, v in leaf.items()}


@functools.lru_cache(maxsize=None)
def _b2_drop_reference(world, seeds, lazy):
    """Parameters after three global batches on the CPU under the ranks' concatenated masks of each step."""
    from oracle import torch_port
    cfg, params, xi, xv, y, *_ = load_train_golden(B2_DROP_NAME)
    g, bs = dc.B2_WORLDS[world]
    batches = [tuple(a[_b2_rows(k * g, (k + 1) * g, len(xi))] for a in (xi, xv, y)) for k in range(3)]
    mask_fn = lambda k, n: dc.shard_masks(cfg, dc.fit_shards(n, bs, world, k * g), seeds, k)  # noqa: E731
    if lazy:
        return _lazy_adam_steps(cfg, params, batches, 1e-3, mask_fn, 0.5)
    return torch_port.train_steps(cfg, params, batches, 1e-3, 0.0, mask_fn, 0.5)[1]


@pytest.mark.parametrize("key", B2_DROP_RUNS)
@pytest.mark.parametrize("world", WORLDS)
def test_adam_steps_with_dropout_on_every_rank(ranks, world, key):
    """Adam, dense and with lazy_exchange, on the small-MLP golden with dropout 0.5 on: replicas array_equal on every
    rank after every step (three global batches, then the 20-row one that leaves ranks empty), all three counters at
    4, and rank 0's parameters after step 3 against three CPU steps on the global batches under the ranks' masks --
    every rank's from its reported seed, the step's counter and its local rows -- at the bars of
    test_gpu_train.test_fused_step_dropout_uses_device_step_seed (median error below 1e-3 lr, 99.9 % below 0.05 lr).
    The dense run's reference is torch.optim.Adam; the lazy run's is Adam with the tables' untouched rows left alone,
    which is what lazy_table_adam documents (NOT the dense Adam), and after step 1 the two runs hold the same bits."""
    res = ranks(world)
    first = res[0]["b2-drop", key]
    lazy = key == "adam"
    assert first["graphs"] and first["drop"] == 0.5
    for rank in range(world):
        r = res[rank]["b2-drop", key]
        assert r["rows"] == [dc.B2_WORLDS[world][1]] * 3 + [dc.B2_PARTIAL_SIZES[world][rank]]
        assert r["counters"] == [4, 4, 4 if lazy else 0] and r["lazy_lists"] == lazy, (rank, r["counters"])
        for k in range(1, 5):
            bad = sorted(n for n in first["hashes"][k] if r["hashes"][k][n] != first["hashes"][k][n])
            assert bad == [] and set(r["hashes"][k]) == set(first["hashes"][k]), (rank, "step", k, bad[:4])
        if lazy:
            assert r["differs_from_dense"] == [] and r["grad_zero"] == [True] * 4 and r["untouched_changed"] == [], rank
    assert all(first["hashes"][k] != first["hashes"][k + 1] for k in range(1, 4))
    want = _b2_drop_reference(world, _seeds(res, ("b2-drop", key)), lazy)
    e = np.concatenate([np.abs(first["params3"][n] - want[n]).reshape(-1) / 1e-3 for n in want])
    print(f"world {world} {key}: median {np.median(e):.2e} lr, 99.9 % {np.quantile(e, 0.999):.2e}, max {e.max():.2e}")
    assert np.median(e) < 1e-3 and np.quantile(e, 0.999) < 0.05, (np.median(e), np.quantile(e, 0.999))


# ---- RCCL, world size 1: the collectives captured into the step's graph
def _nccl_world1_worker(port, q):
    import torch.distributed as dist
    os.environ["DFWFM_DP_GRAPH_COMM"] = "1"
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        assert dist.get_backend() == "nccl"
        q.put(("ok", {("b1-drop", "w1", mode): _b1_run("w1", mode, dist, 0, drop=True) for mode in B1_MODES}))
    except Exception as e:  # report, do not hang the parent
        import traceback
        q.put(("error", repr(e) + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_rccl_world_one_exact_step_with_dropout(gpu):
    """The saturated step with dropout on through a world-size-1 RCCL group, whose collectives are captured into the
    step's one graph (the forward, the per-tile backward that rebuilds the masks, the exchange and the update in one
    replay): every assertion of the gloo ranks' test, bit for bit, in all four modes."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_world1_worker, args=(_port(), q))
    p.start()
    try:
        status, res = q.get(timeout=240)
        p.join(60)
    finally:
        if p.is_alive():
            p.kill()
    assert status == "ok", res
    assert p.exitcode == 0
    for mode in B1_MODES:
        _assert_b1_drop({0: res}, "w1", mode)
