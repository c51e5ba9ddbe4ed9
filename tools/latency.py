"""Forward latency, one call at a time (the reference's run_benchmark / time_forward_pass, model/DeepFMs.py:982-1019:
per-sample latency = single-sample forwards timed one by one; per-batch latency = one batch forward at a time).

Criteo-39 DeepFwFM (lw) and the FwFM-only model on one MI355X, synthetic inputs of the real field sizes, weights with
the init_weights scales.  Each call is one forward through the C ABI (eng.forward) on an otherwise idle GPU, timed
with HIP events around it (device time) and by the host clock around launch + synchronize (what a caller waits); a
batch's forward is also replayed from a one-forward hipGraph (launch overhead of a serving loop that captures).
Prints one JSON line.

  python tools/latency.py [--calls 1000] [--batches 1,16,64,256,1024,4096,8192] [--small] [--bf16] [--bf16-fused] [--int8]
  python tools/latency.py --half-tables [--rounds 7]
  python tools/latency.py --int8-tables [--rounds 7]

--small: the small-batch serving forward (eng.forward_small, include/dfwfm_serve.h) measured beside eng.forward at
every batch, same figures, under models["deepfwfm_small"] (the batch where it stops winning is the value to give
DeepFMs.small_batch_rows).

--bf16: the forward with a bf16 deep tower (eng.forward_bf16, include/dfwfm_bf16.h) beside eng.forward at every batch,
same figures, under models["deepfwfm_bf16"], plus bf16_mfma_frac_back_to_back = 952,800 tower FLOP per sample over
the back-to-back time, as a fraction of 2.5 PF/s.  A batch that is a multiple of 4096 rows and at least 8192 (up to
81920 = 20 x 4096, the headline's workload) is also timed as one eng.forward_batches call over its 4096-row slices:
forward_batches_4096_us (per call) and forward_batches_4096_us_per_batch in the f32 row.

--bf16-fused (implies --bf16): the one-launch bf16 forward (eng.forward_bf16_fused, include/dfwfm_bf16_fused.h) beside
eng.forward and eng.forward_bf16 in the same process, under models["deepfwfm_bf16_fused"]; and the batch-set leg also
through eng.forward_bf16_batches: forward_bf16_batches_4096_us and forward_bf16_batches_4096_us_per_batch in that row
(81920 rows: 20 resident batches of 4096, beside forward_batches_4096_us_per_batch of the f32 row).  The same calls
with the numerical fields folded into layer 1 (eng.sync_bf16_fold, include/dfwfm_bf16_fold.h) are measured right
behind the unfolded ones at every batch, same figures, under models["deepfwfm_bf16_fused_fold"].

--int8: the one-launch forward with an int8 deep tower (eng.forward_int8, include/dfwfm_int8.h) beside eng.forward (and
eng.forward_bf16_fused with --bf16-fused) in the same process at every batch, same figures, under
models["deepfwfm_int8"]; and the batch-set leg through eng.forward_int8_batches: forward_int8_batches_4096_us and
forward_int8_batches_4096_us_per_batch in that row.  DFWFM_DIAG int8rows=16|32 forces its row tile (A/B).

--half-tables: a measurement of its own (nothing above runs): the f32 serving copy of the categorical tables against
the fp16 one (DeepFMs.table_dtype, include/dfwfm_half_tables.h), two modules with the same weights in one process,
the two timed in turns (--rounds turns each, the median and the min-max spread reported), every call replayed from a
hipGraph so that launch overhead is not what is compared.  Rows, in us per 4096-row batch: the FwFM-only forward lone
and as a 20-batch set, the deep f32 forward, the fused bf16 forward and the int8 forward as 20-batch sets -- at the
Criteo-39 table sizes and with every categorical table 8 times as long (HBM-resident).  Also the copies' bytes and
the pack time.

--int8-tables: the same measurement over three modules, one per copy: f32, fp16 and the int8 one
(include/dfwfm_int8_tables.h), timed in turns f32, fp16, int8; the same rows, scales, copy bytes and pack times.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build(deep, dev):
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = synth.CRITEO_FEATURE_SIZES
    m = DeepFMs(field_size=39, feature_sizes=sizes, embedding_size=10, use_fwfm=1, use_fm=0, use_deep=deep,
                use_lw=1, numerical=13, use_cuda=True)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    params = synth.synth_state(shapes, 39, 10, 400, True, bool(deep), seed=1234)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev).eval()
    m.strict_index_check = False
    return m, sizes


def measure(fwd, xi, xv, out, calls, dev):
    """median / p99 device time per call (events), median host time per call (launch + synchronize), and the
    median device time of a one-forward graph replay"""
    st = torch.cuda.current_stream(dev)
    for _ in range(20):
        fwd(xi, xv, out)
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    host = []
    for e0, e1 in ev:
        t0 = time.perf_counter()
        e0.record(st)
        fwd(xi, xv, out)
        e1.record(st)
        e1.synchronize()
        host.append(time.perf_counter() - t0)
    dev_us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fwd(xi, xv, out)
    torch.cuda.synchronize(dev)
    ghost = []
    for _ in range(calls):
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize(dev)
        ghost.append(time.perf_counter() - t0)
    # back to back: 20 calls per graph, replayed without a host sync in between (a serving loop's steady state;
    # the idle gap of a synchronised call lets the chip lower its clock)
    g20 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g20):
        for _ in range(20):
            fwd(xi, xv, out)
    reps = max(5, calls // 20)
    for _ in range(reps):
        g20.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        g20.replay()
    e1.record(st)
    e1.synchronize()
    return {"device_us_median": round(float(np.median(dev_us)), 2), "device_us_p99": round(float(np.percentile(dev_us, 99)), 2),
            "host_us_median": round(float(np.median(host)) * 1e6, 2),
            "graph_host_us_median": round(float(np.median(ghost)) * 1e6, 2),
            "back_to_back_us": round(e0.elapsed_time(e1) * 1e3 / (reps * 20), 2)}


def measure_batch_set(call, xi, xv, out, dev, reps=10):
    """device time of one batch-set call (eng.forward_batches or eng.forward_bf16_batches) over the 4096-row slices of
    (xi, xv), calls issued back to back"""
    nb = xi.shape[0] // 4096
    batches = [(xi[i * 4096:(i + 1) * 4096], xv[i * 4096:(i + 1) * 4096]) for i in range(nb)]
    outs = [out[i * 4096:(i + 1) * 4096] for i in range(nb)]
    st = torch.cuda.current_stream(dev)
    for _ in range(5):
        call(batches, outs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        call(batches, outs)
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, nb


def half_tables(rounds, dev, dtypes=("f32", "fp16")):
    """--half-tables, and --int8-tables with dtypes = ("f32", "fp16", "int8"): see the module docstring."""
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    B, NB = 4096, 20
    if len(dtypes) == 2:
        what = ("f32 serving copy of the categorical tables against the fp16 one (DeepFMs.table_dtype), us per "
                "4096-row batch, hipGraph replays, the two copies timed in turns; median [min, max] over rounds")
    else:
        what = ("f32, fp16 and int8 serving copies of the categorical tables (DeepFMs.table_dtype), us per 4096-row "
                "batch, hipGraph replays, the three copies timed in turns; median [min, max] over rounds")
    res = {"what": what, "rounds": rounds, "batch": B, "set": NB, "scales": {}}

    def module(sizes, deep, dtype):
        m = DeepFMs(field_size=39, feature_sizes=sizes, embedding_size=10, use_fwfm=1, use_fm=0, use_deep=deep,
                    use_lw=1, numerical=13, use_cuda=True)
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        params = synth.synth_state(shapes, 39, 10, 400, True, bool(deep), seed=1234)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        m = m.to(dev).eval()
        m.strict_index_check = False
        m.table_dtype = dtype
        return m

    def graph_of(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(n):
                fn()
        torch.cuda.synchronize(dev)
        return g

    def timed(g, n, reps):
        st = torch.cuda.current_stream(dev)
        g.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            g.replay()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (reps * n)

    def summary(v):
        return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3)}

    for scale in (1, 8):
        sizes = [1] * 13 + [int(n) * scale for n in synth.CRITEO_FEATURE_SIZES[13:]]
        host = [synth.synth_inputs(sizes, 13, B, seed=7 + i) for i in range(NB)]
        dev_in = [(torch.from_numpy(xi).to(dev), torch.from_numpy(xv).to(dev)) for xi, xv in host]
        outs = [torch.empty(B, dtype=torch.float32, device=dev) for _ in range(NB)]
        sc = {"categorical_rows": int(sum(sizes[13:])), "table_bytes": int(sum(sizes[13:])) * 44, "copy_bytes": {},
              "pack_ms": {}, "us_per_batch": {}}
        with torch.no_grad():
            for deep in (0, 1):
                graphs = {}  # row -> {dtype: (graph, calls in it, batches per call)}
                keep = []
                for dtype in dtypes:
                    m = module(sizes, deep, dtype)
                    keep.append(m)
                    eng = m._sync_inference(dev)
                    torch.cuda.synchronize(dev)
                    ts = []
                    for _ in range(3):  # the pack alone: one launch and the wait the pack call makes
                        eng._packed_key = None
                        t0 = time.perf_counter()
                        m._sync_inference(dev)
                        torch.cuda.synchronize(dev)
                        ts.append(time.perf_counter() - t0)
                    sc["pack_ms"][dtype] = round(float(np.median(ts)) * 1e3, 3)
                    sc["copy_bytes"][dtype] = eng.serving_copy_bytes()
                    calls = {}
                    if not deep:
                        calls["fwfm_lone"] = (lambda e=eng: e.forward(dev_in[0][0], dev_in[0][1], outs[0]), 20, 1)
                        calls["fwfm_set20"] = (lambda e=eng: e.forward_batches(dev_in, outs), 5, NB)
                    else:
                        eng.sync_bf16(True)
                        eng.sync_int8(True)
                        if not (eng.bf16_fused_supported() and eng.int8_supported()):
                            raise RuntimeError("the Criteo-39 model must run the fused bf16 and int8 forwards")
                        calls["deep_f32_set20"] = (lambda e=eng: e.forward_batches(dev_in, outs), 2, NB)
                        calls["deep_bf16_fused_set20"] = (lambda e=eng: e.forward_bf16_batches(dev_in, outs), 2, NB)
                        calls["deep_int8_set20"] = (lambda e=eng: e.forward_int8_batches(dev_in, outs), 2, NB)
                    for row, (fn, n, per) in calls.items():
                        graphs.setdefault(row, {})[dtype] = (graph_of(fn, n), n, per)
                for row, by in graphs.items():
                    t = {dtype: [] for dtype in dtypes}
                    for _ in range(rounds):
                        for dtype in dtypes:
                            g, n, per = by[dtype]
                            t[dtype].append(timed(g, n, 20) / per)
                    sc["us_per_batch"][row] = {dtype: summary(t[dtype]) for dtype in dtypes}
                    for dtype in dtypes[1:]:
                        sc["us_per_batch"][row][dtype + "_over_f32"] = round(
                            float(np.median(t[dtype]) / np.median(t["f32"])), 4)
                del graphs, keep
                torch.cuda.empty_cache()
        res["scales"][str(scale)] = sc
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--batches", default="1,16,64,256,1024,4096,8192")
    ap.add_argument("--small", action="store_true", help="also measure eng.forward_small (deep model)")
    ap.add_argument("--bf16", action="store_true", help="also measure eng.forward_bf16 (deep model)")
    ap.add_argument("--bf16-fused", action="store_true",
                    help="also measure eng.forward_bf16_fused and eng.forward_bf16_batches (deep model; implies --bf16)")
    ap.add_argument("--int8", action="store_true",
                    help="also measure eng.forward_int8 and eng.forward_int8_batches (deep model)")
    ap.add_argument("--half-tables", action="store_true",
                    help="only this: the f32 serving copy of the tables against the fp16 one (see the docstring)")
    ap.add_argument("--int8-tables", action="store_true",
                    help="only this: the f32, fp16 and int8 serving copies of the tables (see the docstring)")
    ap.add_argument("--rounds", type=int, default=7, help="--half-tables / --int8-tables: timed turns per copy and row")
    a = ap.parse_args()
    if a.half_tables or a.int8_tables:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        return half_tables(a.rounds, dev, ("f32", "fp16", "int8") if a.int8_tables else ("f32", "fp16"))
    a.bf16 = a.bf16 or a.bf16_fused
    batches = [int(x) for x in a.batches.split(",")]
    if not batches or min(batches) < 1 or max(batches) > 81920:
        ap.error("--batches: sizes from 1 to 81920")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from xsdeepfwfm_deprecated_amd import synth
    res = {"what": "forward latency, one call at a time on an idle MI355X (reference run_benchmark per-sample / "
                   "per-batch latency, model/DeepFMs.py:982-1019); reference published 1.979 ms per sample on CPU "
                   "(data/results/criteo.md:5)", "calls": a.calls, "models": {}}
    for name, deep in (("deepfwfm", 1), ("fwfm", 0)):
        m, sizes = build(deep, dev)
        rows, small, bf16, fused, folded, int8 = {}, {}, {}, {}, {}, {}
        with torch.no_grad():
            eng = m._sync_engine(dev)
            if a.bf16 and deep:
                eng.sync_bf16(True)
            if a.int8 and deep:
                eng.sync_int8(True)
            num_tabs = [m.fm_2nd_embeddings[f].weight.detach() for f in range(13)]

            def fold(on):  # the folded layer 1 of the fused bf16 forward on / off (one pack launch)
                if eng.sync_bf16_fold(num_tabs, on) != on:
                    raise RuntimeError("the model did not fold")

            def stats(fwd, dst, b, xi, xv, out, calls):
                r = measure(fwd, xi, xv, out, calls, dev)
                r["samples_per_s_one_call_at_a_time"] = round(b / (r["device_us_median"] * 1e-6), 1)
                if deep and (dst is rows or dst is small):  # f32 MFMA fraction of the back-to-back rate (967,620 FLOP per sample, 157.3 TF/s)
                    r["mfma_frac_back_to_back"] = round(967620 * b / (r["back_to_back_us"] * 1e-6) / 157.3e12, 4)
                if dst is bf16 or dst is fused or dst is folded:  # the tower alone (952,800 FLOP per sample of the unfolded tower) against the bf16 MFMA peak
                    r["bf16_mfma_frac_back_to_back"] = round(952800 * b / (r["back_to_back_us"] * 1e-6) / 2.5e15, 4)
                dst[str(b)] = r
            for b in batches:
                xi, xv = synth.synth_inputs(sizes, 13, b, seed=7)
                xi, xv = torch.from_numpy(xi).to(dev), torch.from_numpy(xv).to(dev)
                out = torch.empty(b, dtype=torch.float32, device=dev)
                calls = a.calls if b <= 256 else (max(100, a.calls // 10) if b <= 8192 else max(40, a.calls // 25))
                for fwd, dst in ((eng.forward, rows),) + (((eng.forward_small, small),) if a.small and deep else ()) \
                        + (((eng.forward_bf16, bf16),) if a.bf16 and deep else ()) \
                        + (((eng.forward_bf16_fused, fused),) if a.bf16_fused and deep else ()):
                    stats(fwd, dst, b, xi, xv, out, calls)
                if a.bf16_fused and deep:
                    fold(True)
                    stats(eng.forward_bf16_fused, folded, b, xi, xv, out, calls)
                    fold(False)
                if a.int8 and deep:
                    stats(eng.forward_int8, int8, b, xi, xv, out, calls)
                if (a.bf16 or a.int8) and deep and b >= 8192 and b % 4096 == 0:
                    t, nb = measure_batch_set(eng.forward_batches, xi, xv, out, dev)
                    rows[str(b)]["forward_batches_4096_us"] = round(t, 2)
                    rows[str(b)]["forward_batches_4096_us_per_batch"] = round(t / nb, 2)
                    if a.int8:
                        t, nb = measure_batch_set(eng.forward_int8_batches, xi, xv, out, dev)
                        int8[str(b)]["forward_int8_batches_4096_us"] = round(t, 2)
                        int8[str(b)]["forward_int8_batches_4096_us_per_batch"] = round(t / nb, 2)
                    if a.bf16_fused:
                        t, nb = measure_batch_set(eng.forward_bf16_batches, xi, xv, out, dev)
                        fused[str(b)]["forward_bf16_batches_4096_us"] = round(t, 2)
                        fused[str(b)]["forward_bf16_batches_4096_us_per_batch"] = round(t / nb, 2)
                        fold(True)
                        t, nb = measure_batch_set(eng.forward_bf16_batches, xi, xv, out, dev)
                        fold(False)
                        folded[str(b)]["forward_bf16_batches_4096_us"] = round(t, 2)
                        folded[str(b)]["forward_bf16_batches_4096_us_per_batch"] = round(t / nb, 2)
        res["models"][name] = rows
        if bf16:
            res["models"][name + "_bf16"] = bf16
        if fused:
            res["models"][name + "_bf16_fused"] = fused
        if folded:
            res["models"][name + "_bf16_fused_fold"] = folded
        if int8:
            res["models"][name + "_int8"] = int8
        if small:
            res["models"][name + "_small"] = small
    print(json.dumps(res))


if __name__ == "__main__":
    main()
