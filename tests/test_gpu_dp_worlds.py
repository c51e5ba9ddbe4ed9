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


def _local_lists(a, slots, r, case, XI, XV, DL, lo, hi, det, stamp):
    """One emulated rank: forward on rows lo .. hi - 1 (the slices' pointers), DFWFM_BWD_TABLES with the categorical
    tables scattered into the local buffer, then both families' lists into slot r."""
    a.eng.set_deterministic(det)
    a.xi, a.xv, a.dl = XI[lo:hi], XV[lo:hi], DL[lo:hi]  # kept alive: the backward re-reads them
    a.out = torch.empty(hi - lo, device=a.gpu)
    a.eng.train_forward(a.xi, a.xv, a.out, 0.0, case.seed)
    a.phases(a.lib.BWD_TABLES)
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
    case = dc.a_case(model)
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
        _local_lists(a, slots, r, case, XI, XV, DL, *shards[0], det, stamp)
        assert all(n > 0 for _, n, _ in slots.lists(r)), "no stale list to reset"
    a.flat.zero_()  # (what those backwards wrote outside the tables)
    z32, g32 = xc.ref32(case)
    fam_names = {a.lib.FAMILY_SECOND: "fm_2nd_embeddings", a.lib.FAMILY_FIRST: "fm_1st_embeddings"}
    for r, (lo, hi) in enumerate(shards):
        out = _local_lists(a, slots, r, case, XI, XV, DL, lo, hi, det, stamp)
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
        if k not in listed and not k.startswith("net_1_linear_"):
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


def _b1_run(plan, mode, dist, rank):
    """Two rate-0 steps on the rank's full rate-0 batch, then the measured step on fit()'s shard: host arrays."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    sat = xc.saturated()
    case = sat.case
    dev = torch.device("cuda:0")
    world, bs = dc.B1_PLANS[plan]
    m = build(case.cfg, _writable(case.params), dev, is_deep_dropout=False)
    t = FusedTrainStep(m, bs, optimizer="sgd", momentum=0.0, weight_decay=0.0, lr_schedule=[(1, 0.0)], dist=dist,
                       **B1_MODES[mode])

    def step(rows):
        xi, xv, y = (torch.from_numpy(np.array(x[rows])).to(dev) for x in (case.xi, case.xv, sat.y))
        t.step(xi, xv, y, xc.SAT_B)

    t.set_lr(0.0)
    rows0 = dc.rate0_rows(rank, bs, xc.SAT_B)
    step(rows0)  # eager
    step(rows0)  # captured, then replayed
    torch.cuda.synchronize()
    res = {"moved_at_rate_0": [k for k, q in m.named_parameters()
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
               lazy_lists=bool(t.lazy_lists), sparse=bool(t.sparse),
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


def _b2_steps(name, kw, dist, rank, world, g, bs):
    """Deterministic FusedTrainSteps on train golden `name`: three global batches of g rows (step 1 eager, 2 and 3
    replayed), then one of 20 rows, this rank taking fit()'s shard.  dist None: one process on the global batch."""
    from xsdeepfwfm_deprecated_amd.training import FusedTrainStep
    cfg, params, xi, xv, y, *_ = load_train_golden(name)
    dev = torch.device("cuda:0")
    m = build(cfg, params, dev, is_deep_dropout=False)
    t = FusedTrainStep(m, bs, **dict(dict(lr=1e-3, dist=dist, deterministic=True), **kw))
    _, start = _hashes(m, t)
    plan = [(k * g, g) for k in range(3)] + [(3 * g, dc.B2_PARTIAL)]
    res = {"hashes": {}, "logits": {}, "grad_zero": [], "rows": []}
    snaps = {}
    for k, (g0, n_global) in enumerate(plan, 1):
        lo, hi = dc.fit_shards(n_global, bs, world, g0)[rank]
        xb, vb, yb = (torch.from_numpy(a[lo:hi]).to(dev) for a in (xi, xv, y))
        t.step(xb, vb, yb, n_global if dist is not None else None)
        torch.cuda.synchronize()
        if k == 1:
            res["grads"] = {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()}
        res["grad_zero"].append(not bool(t.grad[:t.n_tables].any()))
        res["rows"].append(hi - lo)
        res["logits"][k] = t.out[:hi - lo].detach().cpu().numpy().copy()
        res["hashes"][k], snaps[k] = _hashes(m, t)
    res.update(lazy_lists=bool(t.lazy_lists), graphs=t.graphs is not None,
               counters=[int(c[0].item()) for c in (t.state, t.state_b, t.state_t)])
    if t.lazy_lists:
        # rows of the tables that no rank's shard of any batch touched keep their bits, in the tensor and in the state
        last, offs = snaps[len(plan)], {id(p): o for p, o in zip(t.params, t.offs)}
        bad, n_untouched, n_changed, n_tables = [], 0, 0, 0
        named = dict(m.named_parameters())
        for n, mask in tc.table_rows(cfg, xi[:plan[-1][0] + plan[-1][1]]).items():
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
    world, bs = dc.B1_PLANS[plan]
    sat = xc.saturated()
    want, (z32, _) = xc.sgd_ref(sat), xc.ref32(sat.case)
    res = ranks(world)
    shards = dc.fit_shards(xc.SAT_B, bs, world)
    assert [hi - lo for lo, hi in shards] == dc.B1_SIZES[plan]
    for rank, (lo, hi) in enumerate(shards):
        r = res[rank]["b1", plan, mode]
        what = (plan, mode, "rank", rank)
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
    losses = [np.float32(res[rank]["b1", plan, mode]["loss"]) for rank in range(world)]
    assert float(np.sum(losses, dtype=np.float64)) == sat.loss_sum, (plan, mode, losses)
    assert all(v == 0 for v, (lo, hi) in zip(losses, shards) if hi == lo)


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
