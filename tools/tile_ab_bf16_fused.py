"""A/B of the fused bf16 forward's row tile (DFWFM_DIAG bf16rows=16|32|64) in one process: Criteo-39 DeepFwFM,
back-to-back time per call from 20-call graphs beside eng.forward and eng.forward_bf16, every form's logits compared
with forward_bf16's (equal bits), and at 81920 rows the 20-batch set through forward_batches / forward_bf16_batches.
Prints a line per batch size, then one JSON line.  --fold: the fused forms with the numerical fields folded into layer 1
(include/dfwfm_bf16_fold.h); their logits are then compared with one another (the folded contract is not the per-layer
path's).

  python tools/tile_ab_bf16_fused.py [--batches 256,1024,4096,8192,16384,32768,81920] [--fold]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

import latency  # noqa: E402


def back_to_back_us(fn, dev, reps=10):
    st = torch.cuda.current_stream(dev)
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(20):
            fn()
    for _ in range(3):
        g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        g.replay()
    e1.record(st)
    e1.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / (reps * 20), 2)


def forced(rows):
    if rows:
        os.environ["DFWFM_DIAG"] = f"bf16rows={rows}"  # read by the library at every call
    else:
        os.environ.pop("DFWFM_DIAG", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024,4096,8192,16384,32768,81920")
    ap.add_argument("--fold", action="store_true", help="the fused forms with the folded layer 1 (eng.sync_bf16_fold)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from xsdeepfwfm_deprecated_amd import synth
    m, sizes = latency.build(1, dev)
    res = {}
    with torch.no_grad():
        eng = m._sync_engine(dev)
        eng.sync_bf16(True)
        if a.fold and not eng.sync_bf16_fold([m.fm_2nd_embeddings[f].weight.detach() for f in range(13)], True):
            raise RuntimeError("the model did not fold")
        for b in [int(x) for x in a.batches.split(",")]:
            xi, xv = synth.synth_inputs(sizes, 13, b, seed=7)
            xi, xv = torch.from_numpy(xi).to(dev), torch.from_numpy(xv).to(dev)
            out = torch.empty(b, dtype=torch.float32, device=dev)
            forced(0)
            row = {"f32": back_to_back_us(lambda: eng.forward(xi, xv, out), dev),
                   "bf16": back_to_back_us(lambda: eng.forward_bf16(xi, xv, out), dev)}
            ref = (eng.forward_bf16_fused if a.fold else eng.forward_bf16)(xi, xv).clone()
            for t in (16, 32, 64):
                forced(t)
                row[f"fused{t}"] = back_to_back_us(lambda: eng.forward_bf16_fused(xi, xv, out), dev)
                torch.cuda.synchronize(dev)
                assert torch.equal(out, ref), (b, t)
            forced(0)
            row["fused_auto"] = back_to_back_us(lambda: eng.forward_bf16_fused(xi, xv, out), dev)
            if b == 81920:
                bs = [(xi[i * 4096:(i + 1) * 4096], xv[i * 4096:(i + 1) * 4096]) for i in range(20)]
                outs = [out[i * 4096:(i + 1) * 4096] for i in range(20)]
                row["set_f32_per_batch"] = round(back_to_back_us(lambda: eng.forward_batches(bs, outs), dev, 3) / 20, 2)
                for t in (16, 32, 64):
                    forced(t)
                    row[f"set_fused{t}_per_batch"] = round(
                        back_to_back_us(lambda: eng.forward_bf16_batches(bs, outs), dev, 3) / 20, 2)
                forced(0)
            res[b] = row
            print(b, row, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
