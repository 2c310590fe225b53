"""bench.py's plain run and its output dump, host side: a plain run refuses the measurements that belong to `--full`, its line
carries the contract's fields without the full record's, and `--dump-outputs` writes float32 arrays, samples long ones the same way
every time and stays inside its budget.  CPU only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = dict(os.environ, MCNERF_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), env=env, capture_output=True, text=True, timeout=120)


def test_plain_run_refuses_what_belongs_to_full():
    for opt in (["--also", "f16"], ["--occupancy", "0.25"], ["--extra"]):
        r = _bench("--selftest", *opt)
        assert r.returncode != 0 and "--full" in r.stderr, (opt, r.stderr[-800:])
    r = _bench("--selftest", "--also=", "--occupancy=", "--no-extra", "--no-cpu-baseline")
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1])["selftest"] is True, r.stderr[-800:]
    r = _bench("--selftest", "--full", "--also", "f16", "--occupancy", "0.25")
    assert r.returncode == 0, r.stderr[-800:]


def test_plain_record_line():
    import bench
    rec = {"metric": "train rays/sec (coarse+fine, 64+128 samples)", "value": 1.1e6, "unit": "rays/s", "n_gpus": 1, "steps": 20,
           "warmup": 5, "ms_per_step": 29.78, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": bench.DTYPE_TEXT["f16x3h"], "data": "synthetic",
           "config": {"workload": "w", "precision": "f16x3h", "rays_per_step_per_gpu": 32768, "fine_samples_per_ray": 97.7,
                      "selected_fraction": 0.76, "occupancy": None, "parallelism": "dp1 (cameras sharded, 1 flat all-reduce/step)"},
           "finite": True, "skipped_optimizer_steps": 0, "valid": True, "dist": {"world_size": 1, "backend": None, "rccl_ranks": 0,
                                                                                  "one_gpu_per_rank": True}}
    line = bench.compact_line(rec, None)
    for k in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "steps", "warmup", "valid"):
        assert line[k] == rec[k], k
    assert line["dtype"] == "f16x3h" and "roofline" not in line and "full_record" not in line


def test_write_outputs(tmp_path):
    import bench
    n = bench.DUMP_MAX_ROWS + 7
    long = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
    arrays = {"half": torch.ones(4, 2, dtype=torch.float16), "double": torch.zeros(3, dtype=torch.float64), "loss": torch.tensor(0.5),
              "long": long, "grad": torch.ones(5, requires_grad=True) * 2}
    for d in ("a", "b"):
        bench.write_outputs(os.path.join(str(tmp_path), d), arrays)
    a = {f: np.load(os.path.join(str(tmp_path), "a", f)) for f in os.listdir(os.path.join(str(tmp_path), "a"))}
    b = {f: np.load(os.path.join(str(tmp_path), "b", f)) for f in os.listdir(os.path.join(str(tmp_path), "b"))}
    assert sorted(a) == ["double.npy", "grad.npy", "half.npy", "long.npy", "loss.npy"]
    assert a["half.npy"].dtype == np.float32 and a["double.npy"].dtype == np.float64 and a["loss.npy"].shape == ()
    assert a["long.npy"].shape == (bench.DUMP_MAX_ROWS, 3) and np.array_equal(a["long.npy"], b["long.npy"])
    rows = a["long.npy"][:, 0] / 3
    assert np.all(np.diff(rows) > 0) and np.array_equal(a["long.npy"], long.numpy()[rows.astype(np.int64)])
    with pytest.raises(SystemExit):
        bench.write_outputs(os.path.join(str(tmp_path), "c"), {f"x{i}": torch.zeros(bench.DUMP_MAX_ROWS, 3) for i in range(6)})
    assert not os.path.exists(os.path.join(str(tmp_path), "c"))


def test_dump_train_outputs(tmp_path):
    import bench
    net = torch.nn.Linear(3, 2)
    net.weight.grad = torch.ones_like(net.weight)
    rgb = torch.rand(8, 3)
    last = {"loss": torch.tensor(1.5), "loss_dict": {"rgb": [rgb, rgb + 1, rgb], "intr": [torch.zeros(2, 5, 2), torch.ones(2, 5, 2)]}}
    bench.dump_train_outputs(str(tmp_path), net, last)
    assert sorted(os.listdir(str(tmp_path))) == ["grad.weight.npy", "loss.npy", "param.bias.npy", "param.weight.npy", "reproj_intr.npy",
                                                 "rgb_c.npy", "rgb_f.npy"]
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "rgb_f.npy")), (rgb + 1).numpy())
