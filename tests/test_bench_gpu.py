"""bench.py --gpus 1: a plain run times the C2 headline and nothing else; --full adds the other input stream, parity against the
oracle and the rest. Both print the detail line, then the compact contract line last."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype", "data")


def bench(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"] + argv,
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    if r.returncode != 0:
        pytest.fail("bench.py exited %d\n--- stdout (tail)\n%s\n--- stderr (tail)\n%s" % (r.returncode, r.stdout[-1500:], r.stderr[-4000:]), pytrace=False)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2 and r.stdout.rstrip().endswith(lines[-1]), r.stdout[-2000:]
    detail, final = json.loads(lines[0])["bench_detail"], json.loads(lines[-1])
    for k in CONTRACT:
        assert final[k] == detail[k], k
    assert final["n_gpus"] == 1 and final["steps"] == 20 and final["warmup"] == 5 and final["dtype"] == "f32" and final["value"] > 0
    assert final["metric"].startswith("GFLOP/s on BRGEMM 1024^3 fp32")
    return detail, final


def test_plain_run_measures_the_headline_only(tmp_path):
    d, final = bench(["--dump-outputs", str(tmp_path)])
    assert d["cpu_baseline"] is None and d["per_launch"] is None and d["roofline"]["mfma_busy"] is None
    for k in ("parity", "roofline_uniform", "other_configs", "deployment"):
        assert k not in d, k
    assert "per_rank_step_us" not in d["mlp"]  # the MLP ran for its dumped output only
    c2, out = np.load(str(tmp_path / "c2_C.npy")), np.load(str(tmp_path / "mlp_out.npy"))
    assert c2.shape == (1024, 1024) and out.shape == (4096, 1024)
    assert c2.dtype == out.dtype == np.float32 and np.isfinite(c2).all() and np.isfinite(out).all()
    assert d["dumped_outputs"]["shapes"] == {"c2_C": [1024, 1024], "mlp_out": [4096, 1024]}


def test_full_run_adds_the_other_stream_and_parity():
    d, _ = bench(["--full", "--no-mlp", "--no-cpu-baseline", "--no-pmc"])
    assert set(d["parity"]) == {"reference", "uniform"} and all(p["pass"] for p in d["parity"].values()), d["parity"]
    assert d["roofline_uniform"]["kernel_us"] > 0 and d["per_launch"] is not None
