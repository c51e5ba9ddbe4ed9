"""Training-step benchmark (BASELINE.json configs[4]: DeepFwFM training, DP over RCCL).

    python tools/bench_train.py [--gpus N] [--steps K] [--warmup W] [--batch 4096] [--first-order lw|fwlw]
                                [--lr-schedule 1:1e-4,2000:1e-3,200000:1e-4]
                                [--optimizer adam|sgd|adag|rmsp] [--momentum M] [--lazy-tables]
                                [--optimizer adag --rowwise-tables]
                                [--exchange-world1 [--lazy-adam|--lazy-tables] --lazy-exchange [--apply-worlds 1,2,4,8]]
                                [--exchange-world1 --optimizer adag --rowwise-tables --rowwise-exchange
                                 [--apply-worlds 1,2,4,8]]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 tools/bench_train.py

One step = the reference's fit() inner loop body (model/DeepFMs.py:619-637) on a resident synthetic
Criteo-39 batch: zero_grad, forward (train mode, deep dropout 0.5), BCE-with-logits mean, backward
(HIP), gradient all-reduce when WORLD_SIZE > 1, HIP Adam step (lr 1e-3, weight_decay 3e-7).
Prints one JSON line (samples/s over all ranks, ms/step, max over ranks).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--first-order", choices=["lw", "fwlw"], default="lw")
    ap.add_argument("--no-dropout", action="store_true")
    ap.add_argument("--deterministic", action="store_true",
                    help="fixed-order gradient sums (dfwfm_set_deterministic; the default): bit-identical runs")
    ap.add_argument("--atomic", action="store_true", help="float-atomic gradient sums (arrival order)")
    ap.add_argument("--copy-inputs", action="store_true",
                    help="copy every batch into the fused step's own input buffers (fit()'s path) instead of "
                         "reading the resident batches in place")
    ap.add_argument("--mode", choices=["fused", "autograd"], default="fused",
                    help="fused: FusedTrainStep (HIP-graph replay, what fit() runs); autograd: model() + "
                         "loss.backward() + HIP Adam")
    ap.add_argument("--exchange-world1", action="store_true",
                    help="one rank, but through the data-parallel step (a world-size-1 process group: touched-row "
                         "lists built, all-gathered and applied) -- the exchange kernels' cost without a second GPU")
    ap.add_argument("--apply-worlds", default="",
                    help="with --exchange-world1: afterwards time the apply of W ranks' lists (comma list of W; the "
                         "lists of W distinct batches built by the step itself)")
    ap.add_argument("--steps-per-graph", type=int, default=1,
                    help="fused, one rank: K > 1 replays K consecutive steps over the resident ring as one graph "
                         "(FusedTrainStep.step_many; --steps must be a multiple of K)")
    ap.add_argument("--lazy-adam", action="store_true",
                    help="fused, one rank: the categorical tables' Adam over the rows each batch touched only "
                         "(FusedTrainStep(lazy_table_adam=True); not the reference's dense semantics)")
    ap.add_argument("--lazy-tables", action="store_true",
                    help="fused, one rank: the categorical tables' update over the rows each batch touched only, "
                         "whichever --optimizer runs (FusedTrainStep(lazy_tables=True), include/dfwfm_lazy_optim.h; "
                         "with adam the same as --lazy-adam); composes with --momentum, --atomic and --lr-schedule")
    ap.add_argument("--rowwise-tables", action="store_true",
                    help="fused, one rank, --optimizer adag: row-wise Adagrad for the categorical tables, one "
                         "accumulator per table row over the rows each batch touched "
                         "(FusedTrainStep(rowwise_tables=True), include/dfwfm_rowwise_adagrad.h); composes with "
                         "--atomic and --lr-schedule")
    ap.add_argument("--lazy-exchange", action="store_true",
                    help="fused, with --exchange-world1 or --gpus N and --lazy-adam / --lazy-tables: the lazy update "
                         "under data parallelism, over the exchanged touched-row lists "
                         "(FusedTrainStep(lazy_exchange=True), include/dfwfm_lazy_lists.h); --apply-worlds then times "
                         "the lists update as well")
    ap.add_argument("--rowwise-exchange", action="store_true",
                    help="fused, with --rowwise-tables and --exchange-world1 or --gpus N: row-wise Adagrad under data "
                         "parallelism, over the exchanged touched-row lists (FusedTrainStep(rowwise_exchange=True), "
                         "include_dp/dfwfm_rowwise_lists.h); --apply-worlds then times the lists update as well")
    ap.add_argument("--lr-schedule", default=None, metavar="STEP:LR[,STEP:LR...]",
                    help="fused: the learning rate from a piecewise-linear schedule evaluated on the device every step "
                         "(FusedTrainStep(lr_schedule=...), e.g. \"1:1e-4,2000:1e-3,200000:1e-4\") instead of the "
                         "fixed 1e-3 baked into the graphs")
    ap.add_argument("--optimizer", choices=["adam", "sgd", "adag", "rmsp"], default="adam",
                    help="fused: FusedTrainStep(optimizer=...) (include/dfwfm_optim.h); autograd: torch.optim.SGD / "
                         "Adagrad / RMSprop as the reference constructs them (adam: the HIP Adam)")
    ap.add_argument("--momentum", type=float, default=0.0, help="--optimizer sgd: the momentum")
    ap.add_argument("--gpus", type=int, default=1, help="ranks (one process per GPU; started here unless "
                                                           "torchrun already set WORLD_SIZE)")
    a = ap.parse_args()
    schedule = None
    if a.lr_schedule is not None:
        from xsdeepfwfm_deprecated_amd.cli import parse_lr_schedule
        try:
            schedule = parse_lr_schedule(a.lr_schedule)
        except argparse.ArgumentTypeError as e:
            ap.error(str(e))
        if a.mode != "fused":
            ap.error("--lr-schedule needs --mode fused")
    if a.lazy_exchange and (a.mode != "fused" or not (a.lazy_adam or a.lazy_tables)
                            or not (a.exchange_world1 or a.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1)):
        ap.error("--lazy-exchange needs --mode fused, --lazy-adam or --lazy-tables, and --exchange-world1 or --gpus N")
    if a.rowwise_tables and (a.mode != "fused" or a.optimizer != "adag"):
        ap.error("--rowwise-tables needs --mode fused and --optimizer adag")
    if a.rowwise_exchange and (not a.rowwise_tables or not (
            a.exchange_world1 or a.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1)):
        ap.error("--rowwise-exchange needs --rowwise-tables, and --exchange-world1 or --gpus N")
    from xsdeepfwfm_deprecated_amd.launch import spawn_ranks
    rc = spawn_ranks(a.gpus)  # before any HIP call
    if rc is not None:
        sys.exit(rc)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1 or a.exchange_world1:
        import torch.distributed as dist
        backend = os.environ.get("DFWFM_BENCH_BACKEND", "nccl")  # gloo: rehearse N ranks on fewer GPUs
        if a.exchange_world1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group(backend, rank=0, world_size=1, **({"device_id": dev} if backend == "nccl" else {}))
        elif backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    from xsdeepfwfm_deprecated_amd.training import Adam, FusedTrainStep, allreduce_grads
    sizes = synth.CRITEO_FEATURE_SIZES
    fwlw = a.first_order == "fwlw"
    model = DeepFMs(field_size=39, feature_sizes=sizes, embedding_size=10, use_fwfm=1, use_fm=0, use_deep=1,
                    use_lw=1, use_fwlw=fwlw, numerical=13, is_deep_dropout=not a.no_dropout, use_cuda=True)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    params = synth.synth_state(shapes, 39, 10, 400, True, True, seed=1234)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model = model.to(dev).train()
    if a.optimizer == "adam":
        opt = Adam(model.parameters(), lr=1e-3, weight_decay=3e-7)
    elif a.mode != "fused":  # the autograd path's optimizers (training.make_optimizer)
        opt = {"sgd": lambda ps: torch.optim.SGD(ps, lr=1e-3, momentum=a.momentum, weight_decay=3e-7),
               "adag": lambda ps: torch.optim.Adagrad(ps, lr=1e-3, weight_decay=3e-7),
               "rmsp": lambda ps: torch.optim.RMSprop(ps, lr=1e-3, weight_decay=3e-7)}[a.optimizer](model.parameters())
    # bytes an update moves per parameter: parameter read + written, gradient read, each state array read + written
    opt_bytes = 28 if a.optimizer == "adam" else (12 if (a.optimizer == "sgd" and a.momentum == 0.0) else 20)
    B = a.batch
    batches = []
    for i in range(4):
        xi, xv = synth.synth_inputs(sizes, 13, B, seed=1000 * rank + i)
        y = synth.synth_labels(B, seed=1000 * rank + i)
        batches.append((torch.from_numpy(xi).to(dev), torch.from_numpy(xv).to(dev),
                        torch.from_numpy(y).float().to(dev)))

    trainer = None
    if a.mode == "fused":
        dist = torch.distributed if (world > 1 or a.exchange_world1) else None
        # the four resident batches are read in place (one captured graph set each), like a loader's ring of
        # device input buffers; --copy-inputs copies each batch into the step's own buffers first
        trainer = FusedTrainStep(model, B, lr=1e-3, weight_decay=3e-7, dist=dist, resident_inputs=not a.copy_inputs,
                                 deterministic=not a.atomic, lazy_table_adam=a.lazy_adam, lr_schedule=schedule,
                                 **(dict(lazy_tables=True) if a.lazy_tables else {}),
                                 **(dict(lazy_exchange=True) if a.lazy_exchange else {}),
                                 **(dict(rowwise_tables=True) if a.rowwise_tables else {}),
                                 **(dict(rowwise_exchange=True) if a.rowwise_exchange else {}),
                                 **({} if a.optimizer == "adam" else dict(optimizer=a.optimizer, momentum=a.momentum)))

    def step(i):
        xi, xv, y = batches[i % 4]
        if trainer is not None:
            return trainer.step(xi, xv, y, B * world if world > 1 else None)
        opt.zero_grad()
        out = model(xi, xv)
        loss = F.binary_cross_entropy_with_logits(out, y)
        loss.backward()
        allreduce_grads(model)
        opt.step()
        return loss

    K = a.steps_per_graph if (trainer is not None and world == 1 and not a.exchange_world1) else 1
    if K > 1:
        if a.steps % K or a.warmup % K:
            raise SystemExit("--steps and --warmup must be multiples of --steps-per-graph")
        step(0)  # the first step runs eagerly (step_many needs one behind it)

        def step_k(i):
            return trainer.step_many([batches[(i + j) % 4] for j in range(K)])
    for i in range(0, a.warmup, K):
        step(i) if K == 1 else step_k(i)
    torch.cuda.synchronize(dev)
    if world > 1:
        torch.distributed.barrier()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    wall0 = time.perf_counter()
    t0.record()
    for i in range(0, a.steps, K):
        loss = step(i) if K == 1 else step_k(i)
    host = time.perf_counter() - wall0  # the host's enqueue time (ahead of the GPU if well under the step time)
    t1.record()
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - wall0
    ms = t0.elapsed_time(t1)
    if world > 1:
        t = torch.tensor([ms], device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        ms = float(t.item())
        torch.distributed.barrier()
    opt_name = {"adam": "Adam", "sgd": "SGD", "adag": "Adagrad", "rmsp": "RMSprop"}[a.optimizer]
    res = {"metric": f"DeepFwFM training samples/sec (Criteo-39, {opt_name}, dropout 0.5)",
           "value": round(world * B * a.steps / (ms / 1e3), 1), "unit": "samples/s", "n_gpus": world,
           "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms / a.steps, 4), "per_gpu_batch": B,
           "first_order": a.first_order, "dropout": not a.no_dropout, "wall_s": round(wall, 3),
           "host_enqueue_us_per_step": round(host * 1e6 / a.steps, 1),
           "mode": a.mode, "deterministic": not a.atomic, "steps_per_graph": K, "inputs": "copied" if (a.copy_inputs or a.mode != "fused") else "resident (read in place)",
           "lazy_adam": bool(trainer is not None and getattr(trainer, "lazy", False) and a.optimizer == "adam"),
           "lazy_tables": bool(trainer is not None and getattr(trainer, "lazy", False)),
           "lazy_exchange": bool(trainer is not None and getattr(trainer, "lazy_lists", False)),
           "rowwise_tables": bool(trainer is not None and getattr(trainer, "rowwise", False)),
           "rowwise_exchange": bool(trainer is not None and getattr(trainer, "rowwise_exchange", False)),
           "lr_schedule": schedule, "optimizer": a.optimizer, "momentum": a.momentum,
           "optimizer_bytes_per_param": opt_bytes,
           "final_loss_sum": round(float(loss.item()), 4)}
    if res["lazy_tables"]:
        # distinct rows the four resident batches touch per step, per table family (what the lazy step updates)
        res["touched_rows_per_step"] = touched_rows(model, [b[0] for b in batches])
    if res["rowwise_tables"]:
        # the tables' optimizer state: one float per row, against the element-wise Adagrad's one per element
        res["table_state_bytes"] = {"rowwise": 4 * trainer.row_state.numel(),
                                    "elementwise": 4 * sum(p.numel() for p in trainer.params[:trainer.n_cat])}
    if trainer is not None and getattr(trainer, "sparse", False):
        # touched-row lists all-gathered per step (fixed capacity: sum over tables of min(batch, rows))
        res["exchange"] = {"backend": torch.distributed.get_backend(), "packed_bytes_per_rank": trainer.sp_bytes,
                           "dense_bucket_bytes": 4 * (trainer.n_bucket_a - trainer.n_tables),
                           "mlp_bucket_bytes": 4 * (trainer.grad.numel() - trainer.n_bucket_a)}
    if a.apply_worlds and trainer is not None and getattr(trainer, "sparse", False):
        res["apply"] = apply_bench(trainer, model, sizes, B, dev, [int(w) for w in a.apply_worlds.split(",")])
    if rank == 0:
        print(json.dumps(res), flush=True)
    if world > 1 or a.exchange_world1:
        torch.distributed.destroy_process_group()


def touched_rows(model, xis):
    """Distinct table rows per step over the batches' keys: second-order (width D) and first-order (width 1) tables
    (a QR field counts its quotient and its remainder rows), averaged over the batches; and the tables' total rows."""
    fields, _ = model._param_layout()
    per = []
    for xi in xis:
        n2 = n1 = 0
        for f in range(model.num, model.field_size):
            e2, e2r, e1, e1r = fields[f]
            k = xi[:, f - model.num]
            for q, r, fam in ((e2, e2r, 2), (e1, e1r, 1)):
                if q is None:
                    continue
                if r is None:
                    cnt = int(torch.unique(k).numel())
                else:
                    c = int(r.shape[0])
                    cnt = int(torch.unique(k // c).numel()) + int(torch.unique(k % c).numel())
                if fam == 2:
                    n2 += cnt
                else:
                    n1 += cnt
        per.append((n2, n1))
    rows = lambda i: sum(int(t.shape[0]) for f in range(model.num, model.field_size)  # noqa: E731
                         for t in fields[f][i:i + 2] if t is not None)
    return {"second_order": round(sum(p[0] for p in per) / len(per), 1),
            "first_order": round(sum(p[1] for p in per) / len(per), 1),
            "second_order_table_rows": rows(0), "first_order_table_rows": rows(2)}


def apply_bench(trainer, model, sizes, B, dev, worlds, reps=50):
    """The receive side of the touched-row exchange at world sizes the box cannot host: the step's own lists for
    max(worlds) distinct batches stacked as an all-gathered buffer and applied (one launch per rank and family, in
    rank order, as the step does) to a copy of the gradient buffer, graph-replayed."""
    import ctypes
    from xsdeepfwfm_deprecated_amd import _lib, synth
    L = _lib.lib()
    snaps = []
    for i in range(max(worlds)):
        xi, xv = synth.synth_inputs(sizes, 13, B, seed=7000 + i)
        y = synth.synth_labels(B, seed=7000 + i)
        trainer.step(*(torch.from_numpy(t).to(dev) for t in (xi, xv)), torch.from_numpy(y).float().to(dev))
        snaps.append(trainer.sp_send.clone())
    torch.cuda.synchronize(dev)
    counts = [[int(sn[f["o_cnt"]:f["o_cnt"] + 4].view(torch.int32).item()) for sn in snaps] for f in trainer.sp_fams]
    grad = trainer.grad.clone()
    out = {"entries_per_rank": {"width%d" % f["w"]: sum(c) / len(c) for f, c in zip(trainer.sp_fams, counts)},
           "capacity": {"width%d" % f["w"]: f["cap"] for f in trainer.sp_fams}}
    for w in worlds:
        recv = torch.stack(snaps[:w])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # the capture stream
            for r in range(w):
                rb = recv[r].data_ptr()
                for f in trainer.sp_fams:
                    _lib.check(L.dfwfm_sparse_grads_apply(
                        ctypes.c_void_p(grad.data_ptr()), f["w"], ctypes.c_void_p(rb + f["o_dest"]),
                        ctypes.c_void_p(rb + f["o_rows"]), ctypes.c_void_p(rb + f["o_cnt"]), f["cap"], st), "apply")
        for _ in range(3):
            g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize(dev)
        out["world%d_us" % w] = round(e0.elapsed_time(e1) * 1e3 / reps, 2)
        if getattr(trainer, "lazy_lists", False):
            out["world%d_lists_us" % w] = lists_bench(trainer, recv, w, grad, dev, reps)
            # the same rank's lists W times: every row claimed W times (the worst case for claims) but updated once
            # (the best case for traffic)
            out["world%d_lists_replicated_us" % w] = lists_bench(trainer, torch.stack([snaps[0]] * w), w, grad, dev,
                                                                 reps)
    return out


def lists_bench(trainer, recv, w, grad, dev, reps):
    """The list-driven lazy update (include/dfwfm_lazy_lists.h; under rowwise_exchange the row-wise one,
    include_dp/dfwfm_rowwise_lists.h) over W ranks' lists, graph-replayed on copies of the flat buffers with a state block
    and stamps of its own (the trainer's are not touched): every replay is a fresh step over the same rows.
    Microseconds per call."""
    import ctypes
    from xsdeepfwfm_deprecated_amd import _lib
    L = _lib.lib()
    P = ctypes.c_void_p
    if trainer.rowwise:
        return rowwise_lists_bench(trainer, recv, w, grad, dev, reps)
    spans = (_lib.dfwfm_lazy_lists_span * len(trainer.ll_spans))()
    stamp = torch.zeros_like(trainer.lazy_stamp)
    keep, row0 = [], 0
    for i, sp in enumerate(trainer.ll_spans):
        p = trainer.params[i].detach().clone()
        keep.append(p)
        spans[i] = _lib.dfwfm_lazy_lists_span(p.data_ptr(), stamp[row0:].data_ptr(), sp.offset, sp.rows, sp.width, 0)
        row0 += sp.rows
    lists = (_lib.dfwfm_lazy_lists_list * (w * len(trainer.sp_fams)))()
    for r in range(w):
        rb = recv[r].data_ptr()
        for k, f in enumerate(trainer.sp_fams):
            lists[r * len(trainer.sp_fams) + k] = _lib.dfwfm_lazy_lists_list(rb + f["o_dest"], rb + f["o_cnt"],
                                                                             f["cap"], f["w"], 0)
    state = torch.zeros_like(trainer.state_t)
    adam = trainer.optimizer == "adam"
    bufs = [torch.zeros_like(grad) for _ in range(2 if adam else (0 if trainer.opt_state is None else 1))]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = P(torch.cuda.current_stream(dev).cuda_stream)  # the capture stream
        if adam:
            b1, b2 = trainer.betas
            _lib.check(L.dfwfm_lazy_adam_lists_step_dev(spans, len(spans), lists, len(lists), P(grad.data_ptr()),
                                                        P(bufs[0].data_ptr()), P(bufs[1].data_ptr()), trainer.lr, b1,
                                                        b2, trainer.eps, trainer.wd, P(state.data_ptr()), st), "lists")
        else:
            _lib.check(L.dfwfm_lazy_optim_lists_step_dev(spans, len(spans), lists, len(lists), P(grad.data_ptr()),
                                                         P(bufs[0].data_ptr()) if bufs else None,
                                                         ctypes.byref(trainer.hyper), P(state.data_ptr()), st), "lists")
    for _ in range(3):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize(dev)
    return round(e0.elapsed_time(e1) * 1e3 / reps, 2)


def rowwise_lists_bench(trainer, recv, w, grad, dev, reps):
    """lists_bench for dfwfm_rowwise_adagrad_lists_step_dev: the spans carry a copy of row_state."""
    import ctypes
    from xsdeepfwfm_deprecated_amd import _lib
    L = _lib.lib()
    P = ctypes.c_void_p
    spans = (_lib.dfwfm_rowwise_lists_span * len(trainer.ll_spans))()
    stamp = torch.zeros_like(trainer.lazy_stamp)
    acc = torch.zeros_like(trainer.row_state)
    keep, row0 = [], 0
    for i, sp in enumerate(trainer.ll_spans):
        p = trainer.params[i].detach().clone()
        keep.append(p)
        spans[i] = _lib.dfwfm_rowwise_lists_span(p.data_ptr(), acc[row0:].data_ptr(), stamp[row0:].data_ptr(),
                                                 sp.offset, sp.rows, sp.width, 0)
        row0 += sp.rows
    lists = (_lib.dfwfm_lazy_lists_list * (w * len(trainer.sp_fams)))()
    for r in range(w):
        rb = recv[r].data_ptr()
        for k, f in enumerate(trainer.sp_fams):
            lists[r * len(trainer.sp_fams) + k] = _lib.dfwfm_lazy_lists_list(rb + f["o_dest"], rb + f["o_cnt"],
                                                                             f["cap"], f["w"], 0)
    state = torch.zeros_like(trainer.state_t)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = P(torch.cuda.current_stream(dev).cuda_stream)  # the capture stream
        _lib.check(L.dfwfm_rowwise_adagrad_lists_step_dev(spans, len(spans), lists, len(lists), P(grad.data_ptr()),
                                                          ctypes.byref(trainer.hyper), P(state.data_ptr()), st),
                   "rowwise lists")
    for _ in range(3):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize(dev)
    return round(e0.elapsed_time(e1) * 1e3 / reps, 2)


if __name__ == "__main__":
    main()
