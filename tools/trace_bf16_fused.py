"""Workload for a kernel trace of the three forwards side by side (run it under `rocprofv3 --kernel-trace --stats`):
Criteo-39 DeepFwFM, eager calls of eng.forward, eng.forward_bf16 and eng.forward_bf16_fused at one batch size, then
20-batch sets of 4096 rows through eng.forward_batches and eng.forward_bf16_batches.  One batch size per process, so
the per-kernel averages of the trace belong to that size.  --fold: the fused calls run with the numerical fields
folded into layer 1 (include/dfwfm_bf16_fold.h; the kernel's name is the same, so folded and unfolded are runs of
their own).

  rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python3 tools/trace_bf16_fused.py --batch 4096
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

import latency  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sets", type=int, default=0, help="20-batch sets of 4096 rows through both batch-set calls")
    ap.add_argument("--fold", action="store_true", help="the fused calls with the folded layer 1 (eng.sync_bf16_fold)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from xsdeepfwfm_deprecated_amd import synth
    m, sizes = latency.build(1, dev)
    with torch.no_grad():
        eng = m._sync_engine(dev)
        eng.sync_bf16(True)
        if a.fold and not eng.sync_bf16_fold([m.fm_2nd_embeddings[f].weight.detach() for f in range(13)], True):
            raise RuntimeError("the model did not fold")
        xi, xv = synth.synth_inputs(sizes, 13, a.batch, seed=7)
        xi, xv = torch.from_numpy(xi).to(dev), torch.from_numpy(xv).to(dev)
        out = torch.empty(a.batch, dtype=torch.float32, device=dev)
        for fwd in (eng.forward, eng.forward_bf16, eng.forward_bf16_fused):
            for _ in range(a.calls):
                fwd(xi, xv, out)
            torch.cuda.synchronize(dev)
        if a.sets:
            xi, xv = synth.synth_inputs(sizes, 13, 81920, seed=7)
            xi, xv = torch.from_numpy(xi).to(dev), torch.from_numpy(xv).to(dev)
            out = torch.empty(81920, dtype=torch.float32, device=dev)
            bs = [(xi[i * 4096:(i + 1) * 4096], xv[i * 4096:(i + 1) * 4096]) for i in range(20)]
            outs = [out[i * 4096:(i + 1) * 4096] for i in range(20)]
            for call in (eng.forward_batches, eng.forward_bf16_batches):
                for _ in range(a.sets):
                    call(bs, outs)
                torch.cuda.synchronize(dev)


if __name__ == "__main__":
    main()
