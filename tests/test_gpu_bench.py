"""GPU: bench.py's plain run and --dump-outputs -- the result line of a plain run, and the dumped logits of the
timed path's last launches: their shape, that two runs with the same arguments give the same array, and that the
rows are the forward of the resident batches they stand for (float64 oracle, north-star bar)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, logit_close
from oracle import dfwfm_oracle

pytestmark = pytest.mark.gpu

STEPS = 40  # more than one batch set (32): two streams, one launch of 20 batches on each


@pytest.fixture(scope="module")
def runs(gpu, tmp_path_factory):
    """Two plain bench runs with the same arguments, side by side: [(result line, logits), ...]."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
              "DFWFM_BENCH_STUB_MS", "DFWFM_DIAG"):
        env.pop(k, None)
    dirs = [str(tmp_path_factory.mktemp(f"dump{i}")) for i in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                               "--warmup", "2", "--settle-ms", "0", "--dump-outputs", d], env=env, cwd=d,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for d in dirs]
    got = []
    for p, d in zip(procs, dirs):
        out, err = p.communicate(timeout=240)
        assert p.returncode == 0, err[-2000:]
        lines = [ln for ln in out.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out
        assert os.listdir(d) == ["logits.npy"]
        got.append((json.loads(lines[0]), np.load(os.path.join(d, "logits.npy"))))
    return got


def test_plain_run_result_line(runs):
    for r, _ in runs:
        assert r["steps"] == STEPS and r["unit"] == "samples/s" and r["higher_is_better"] is True
        assert r["dtype"] == "f32" and r["ms_per_step"] > 0
        assert abs(r["value"] - 4096 / (r["ms_per_step"] / 1e3)) <= 1e-3 * r["value"]
        assert "roofline" in r
        for leg in ("per_call", "roofline_gather", "cpu_baseline", "parity"):  # --full only
            assert leg not in r


def test_dump_shape_and_reproducible(runs):
    (_, a), (_, b) = runs
    assert a.shape == (STEPS, 4096) and a.dtype == np.float32 and np.isfinite(a).all()
    assert np.array_equal(a, b)


def test_dump_rows_match_oracle(runs):
    """Row k * 20 + j is stream k's j-th batch of its launch: resident batch k + 2 j (bench.py dump_outputs), whose
    inputs are synth_inputs(seed = batch index)."""
    from conftest import model_kwargs
    from xsdeepfwfm_deprecated_amd import DeepFMs, synth
    sizes = synth.CRITEO_FEATURE_SIZES
    cfg = dict(field_size=39, feature_sizes=sizes, embedding_size=10, use_fwfm=1, use_fm=0, use_logit=0,
               use_deep=1, use_lw=1, use_fwlw=0, h_depth=3, deep_nodes=400, numerical=13, embedding_bag=0,
               qr_flag=0, qr_operation="mult", qr_collisions=4, qr_threshold=200)
    shapes = {k: tuple(v.shape) for k, v in DeepFMs(**model_kwargs(cfg)).state_dict().items()}
    params = synth.synth_state(shapes, 39, 10, 400, True, True, seed=1234)
    logits = runs[0][1]
    rows = np.random.default_rng(0).choice(4096, 64, replace=False)
    for k, j in ((0, 0), (0, 19), (1, 0), (1, 19)):
        xi, xv = synth.synth_inputs(sizes, 13, 4096, seed=k + 2 * j)
        ref = dfwfm_oracle.forward(cfg, params, xi[rows], xv[rows])
        assert logit_close(logits[k * 20 + j][rows], ref) < 1e-5, (k, j)
