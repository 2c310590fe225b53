"""Multi-process checks of the N > 1 path on the one-GPU box.  Collected LAST (file name) so that a multi-process failure can
never hide a kernel test (round 4: one hung rank cost the driver's run 92 tests), ordered cheapest first, each bounded well
inside its pytest timeout, and each child launched by scripts/_ranks.py, which prints a dead rank's traceback and exits
within seconds.  Reference behaviour under test: main.py:60-62, 78-89; utils/distributed_init.py:11-34;
data/data_read.py:358-360."""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _clean_env(**extra):
    env = dict(os.environ, **extra)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def _run_script(name, timeout_s):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", name)], capture_output=True, text=True, timeout=timeout_s,
                       env=_clean_env())
    assert r.returncode == 0 and "check: OK" in r.stdout, "rc %d\n--- stdout\n%s\n--- stderr\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-6000:])


pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release_this_process_gpu_memory(gpu_device):
    """The rank processes are CHILDREN of the pytest process, on the same GPU.  By the time this file runs the parent's caching
    allocator holds whatever the full-size tests before it ever touched -- measured on the driver's box: all 288 GB, "0 bytes
    free" -- and a child's first allocation fails with HIP out of memory (round 4's hidden rank-0 crash, GPUTEST_r04.json).
    Give the cache back before every test here and say how much the children will find."""
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    assert free > 24 << 30, f"only {free / 2**30:.1f} of {total / 2**30:.1f} GiB free for the rank processes after empty_cache()"
    yield


@pytest.mark.timeout(360)
def test_flat_grad_sync_through_rccl_with_one_rank(gpu_device):
    """backend="nccl" (= RCCL) with world_size 1 on the 1-GPU box: FlatGradSync(force_collective=True) takes the collective
    path -- arena assembly, the flat all_reduce on an RCCL communicator, the flag read-back, .grad re-pointing -- and must
    leave exactly the gradients a plain backward produces."""
    root = ROOT
    code = """
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(%d), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
from mc_nerf_amd import distributed as D, synthetic as S
from mc_nerf_amd.model import MC_Model, MC_NeRF_Loss
dev = torch.device("cuda", 0); torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1)
sp = S.make_sys_param(dev, samples=32, scale=2, batch=512, H=32, W=32, coarse=(4, 32, [2]), fine=(8, 64, [4]), precision="f16x3")
torch.manual_seed(1); model = MC_Model(sp).to(dev); S.init_cameras_near_gt(model, noise=1e-3)
wpts, pts = S.calibration_points(sp["gt_pose"], sp["intr_mat"][0]); wpts, pts = wpts.to(dev), pts.to(dev)
img = torch.rand(1, 32 * 32, 3, device=dev)
def grads(sync):
    torch.manual_seed(5)
    for p in model.parameters(): p.grad = None
    if sync: sync.prepare()
    loss_dict, *_ = model((img, torch.tensor([3]), wpts, pts, wpts, pts), 20, "GLOBAL_OPTIM_EPOCH", 0.6)
    MC_NeRF_Loss(sp)(loss_dict, "GLOBAL_OPTIM_EPOCH").backward()
    if sync: sync.sync()
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
plain = grads(None)
s = D.FlatGradSync(model, 1, force_collective=True)
via = grads(s)
assert dist.get_backend() == "nccl"
for n in plain:
    assert (plain[n] is None) == (via[n] is None), n
    if plain[n] is not None:
        assert torch.allclose(plain[n], via[n], rtol=1e-4, atol=1e-7), n      # (weight-gradient atomics: summation order)
assert s.asymmetric_steps() == 0
dist.destroy_process_group()
print("rccl-1-rank: OK")
""" % (root, _free_port())
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "rccl-1-rank: OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.timeout(460)
@pytest.mark.parametrize("world", [2, 8])
def test_bench_two_ranks_share_one_gpu(gpu_device, tmp_path, world):
    """`python bench.py --gpus 2` (and `--gpus 8`: the driver's largest form, eight rank processes sharing the GPU) end to end on the one-GPU box: the parent starts two rank processes, they rendezvous (gloo here:
    RCCL needs one GPU per rank), shard the cameras, run the step loop with the gradient sync, and rank 0 prints the JSON line with
    the multi-rank fields -- parameters bit-identical across ranks, no asymmetric gradient step, the all-reduce time."""
    import json
    root = ROOT
    env = dict(os.environ, MCNERF_SHARE_GPU="1", MCNERF_DIST_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    full = os.path.join(str(tmp_path), "bench_full.json")
    # world 2: the pinned-occupancy lines asked for explicitly (the DDP invariant on them); world 8: the full record's defaults, nothing but
    # --gpus / --steps / --warmup decided here -- at N > 1 bench.py --full then measures the headline mode + f16x3 only (no by_occupancy, no extra_lines)
    extra = ["--also=", "--occupancy=0.25,0.05"] if world == 2 else []
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--gpus", str(world), "--rays", "2048", "--steps", "6", "--warmup", "2",
                        "--no-cpu-baseline", "--full-json", full] + extra, capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    assert len(line) < 2048, len(line)                      # the stdout line the driver keeps is the compact one ...
    c = json.loads(line)
    assert c["n_gpus"] == world and c["dist"] == {"world_size": world, "backend": "gloo", "rccl_ranks": 0, "one_gpu_per_rank": False}
    assert c["params_identical_across_ranks"] is True and c["asymmetric_grad_steps"] == 0
    assert len(c["rank_ms_per_step"]) == world and c["allreduce_ms"] > 0 and c["roofline"]["frac"] > 0
    if world == 2:
        assert c["rho005_value"] > 0
    else:
        assert "rho005_value" not in c and c["f16x3_value"] > 0
    j = json.load(open(full))                               # ... and the whole record is the file it names
    assert c["full_record"] == "bench_full.json" and abs(j["value"] - c["value"]) < 1e-5 * j["value"]
    assert j["n_gpus"] == world and j["steps"] == 6 and j["scaling"] == "weak"
    assert j["params_identical_across_ranks"] is True and j["asymmetric_grad_steps"] == 0 and j["finite"] is True
    assert j["allreduce_ms"] > 0 and j["value"] > 0
    assert j["config"]["rays_per_step_per_gpu"] == 2048 and j["config"]["parallelism"].startswith(f"dp{world}")
    for rho, modes in j["by_occupancy"].items():          # the occupancy shift is rank 0's on every rank: the DDP invariant holds on these lines too
        for p, rec in modes.items():
            assert rec["params_identical_across_ranks"] is True and rec["asymmetric_grad_steps"] == 0 and rec["valid"], (rho, p, rec)
            assert abs(rec["selected_fraction"] - float(rho)) < 0.5 * float(rho), (rho, p, rec["selected_fraction"])


@pytest.mark.timeout(460)
def test_bench_under_torchrun_with_one_rank_is_the_plain_line(gpu_device, tmp_path):
    """The driver's N = 1 forms: `python bench.py` and `python -m torch.distributed.run --nproc-per-node 1 bench.py --gpus 1` must be
    the SAME path (no process group, no collective, no camera sharding) and report themselves so: n_gpus 1, dist.world_size 1,
    rccl_ranks 0 (no communicator exists), parallelism dp1 -- and agree on the step time to the run-to-run spread of a 2048-ray step."""
    import json
    args = ["--gpus", "1", "--rays", "2048", "--steps", "20", "--warmup", "5", "--also=", "--occupancy=", "--no-extra", "--no-cpu-baseline"]
    recs = []
    for k, launcher in enumerate(([sys.executable], [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                                                     "--master-addr", "127.0.0.1", "--master-port", str(_free_port())])):
        full = os.path.join(str(tmp_path), f"full{k}.json")
        r = subprocess.run(launcher + [os.path.join(ROOT, "bench.py")] + args + ["--full-json", full], capture_output=True, text=True,
                           timeout=400, env=_clean_env())
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        c = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert c["n_gpus"] == 1 and c["dist"]["world_size"] == 1 and c["dist"]["rccl_ranks"] == 0 and c["config"]["parallelism"] == "dp1"
        assert "allreduce_ms" not in c and c["valid"] is True
        recs.append(c)
    a, b = recs[0]["ms_per_step"], recs[1]["ms_per_step"]
    assert abs(a - b) < 0.5 * max(a, b), (a, b)           # (a 2048-ray step is ~2.5 ms and host-bound: a loose gate -- the claim is the PATH, checked above)


@pytest.mark.timeout(400)
def test_bench_plain_run_times_its_steps_and_dumps_the_last_one(gpu_device, tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` measures the headline and nothing else (no roofline pass, no other mode, no record
    file), and `--dump-outputs DIR` leaves what the last timed step computed: loss, both renders, every parameter after the RAdam step and
    its gradient, float32.  Two runs with the same arguments start from the same inputs, so their outputs agree to the weight-gradient
    atomics' order."""
    import json
    import numpy as np
    outs = []
    for k in range(2):
        dump = os.path.join(str(tmp_path), f"out{k}")
        full = os.path.join(str(tmp_path), f"full{k}.json")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rays", "2048", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", dump, "--full-json", full], capture_output=True, text=True, timeout=180, env=_clean_env())
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        c = json.loads(lines[0])
        assert c["steps"] == 3 and c["warmup"] == 1 and c["n_gpus"] == 1 and c["valid"] is True and c["dtype"] == "f16x3h"
        assert c["unit"] == "rays/s" and c["higher_is_better"] is True and abs(c["value"] - 2048 / (c["ms_per_step"] * 1e-3)) < 1e-3 * c["value"]
        assert "roofline" not in c and "f16x3_value" not in c and "cpu_baseline" not in c and not os.path.exists(full)
        files = sorted(os.listdir(dump))
        arrays = {f[:-4]: np.load(os.path.join(dump, f)) for f in files}
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20 and all(a.dtype == np.float32 for a in arrays.values())
        assert arrays["rgb_c"].shape == (2048, 3) and arrays["rgb_f"].shape == (2048, 3) and np.isfinite(arrays["loss"]).all()
        assert "param.nerf.nerf_fine.sh.2.weight" in arrays and "grad.nerf.nerf_fine.sh.2.weight" in arrays
        outs.append(arrays)
    assert outs[0].keys() == outs[1].keys()
    for name in outs[0]:                                    # (>= 99.9 % of the elements: a sample at the selection threshold may flip)
        a, b = outs[0][name], outs[1][name]
        assert a.shape == b.shape and np.mean(np.abs(a - b) <= 1e-3 * max(1.0, float(np.abs(a).max()))) >= 0.999, name


@pytest.mark.timeout(460)
def test_bench_under_the_drivers_torchrun_command_with_two_ranks(gpu_device, tmp_path):
    """The driver's N > 1 launch, verbatim -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1
    --master-port P bench.py --gpus 2 --steps K --warmup W` -- with the real kernels and `--full`: the ranks are torchrun's processes (bench.py
    starts none), they bind through LOCAL_RANK, and rank 0 alone prints the compact line with the multi-rank fields and (the N > 1 default
    of the full record) the headline mode + `f16x3` only.  (Two ranks share this box's one GPU over gloo, which they declare with MCNERF_SHARE_GPU=1; with one GPU
    per rank the same command runs over RCCL and bench.py refuses anything else.)"""
    import json
    env = dict(_clean_env(), MCNERF_SHARE_GPU="1", MCNERF_DIST_BACKEND="gloo")
    full = os.path.join(str(tmp_path), "bench_full.json")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6", "--warmup", "2",
                        "--rays", "2048", "--full", "--no-cpu-baseline", "--full-json", full], capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < 2048, (len(lines), [len(l) for l in lines])
    c = json.loads(lines[0])
    assert c["n_gpus"] == 2 and c["steps"] == 6 and c["warmup"] == 2 and c["scaling"] == "weak"
    assert c["dist"] == {"world_size": 2, "backend": "gloo", "rccl_ranks": 0, "one_gpu_per_rank": False}
    assert c["params_identical_across_ranks"] is True and c["asymmetric_grad_steps"] == 0 and c["allreduce_ms"] > 0
    assert len(c["rank_ms_per_step"]) == 2 and c["f16x3_value"] > 0 and "rho005_value" not in c and "f16_value" not in c
    # without the declaration a shared GPU is refused: the scaling line is one GPU per rank over RCCL or nothing
    env2 = dict(_clean_env(), MCNERF_DIST_BACKEND="gloo")
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                         "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                         "--rays", "2048", "--no-cpu-baseline", "--full-json", full], capture_output=True, text=True, timeout=300, env=env2)
    assert r2.returncode != 0, r2.stdout[-1500:]          # (rank 1 finds no cuda:1 on a one-GPU box, or rank 0 refuses the gloo backend)


@pytest.mark.timeout(420)
def test_two_ranks_share_one_gpu_data_parallel(gpu_device):
    """N > 1 path with the real HIP backward: two gloo ranks on one GPU (scripts/two_rank_one_gpu.py) - the arena
    is filled by the kernels, one all-reduce averages it, parameters stay bit-identical across ranks."""
    _run_script("two_rank_one_gpu.py", 360)


@pytest.mark.timeout(540)
def test_stock_ddp_nerf_stages_and_main_py_optimiser_protocol(gpu_device):
    """main.py:60-62 + :176-207 + :78-89 on the HIP path: MC_Model wrapped in stock DistributedDataParallel(find_unused_parameters=True),
    the three RAdam / ExponentialLR sets with the reference's requires_grad_ toggles, two steps of each stage on two gloo ranks
    sharing the GPU (scripts/two_rank_ddp_one_gpu.py): replicas bit-identical, and the result equal to FlatGradSync's."""
    _run_script("two_rank_ddp_one_gpu.py", 480)
