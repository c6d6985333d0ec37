"""Multi-rank runs of the REAL HIP path on the one GPU of the test box."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

import hands_amd
from hands_amd.weights import synthetic_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("bz,where", [(5, "host"), (4, "host"), (5, "device"), (6, "device")])
def test_two_ranks_of_the_real_model_equal_the_single_process_forward(tmp_path, recipe_model, bz, where):
    """Two rank processes (started fresh, each on cuda:0) shard a global batch -- bz=5 is UNEVEN (3 + 2
    samples) --, run hands_amd.HandsLight on their shard and all-gather the packed predictions; the gathered
    dict must equal the single-process forward of the global batch BIT FOR BIT (samples are independent and
    every kernel's summation order is batch-size invariant).  "device": the predictions stay on the GPU and the
    gather runs on its own stream behind the forward's asynchronous tail (the path RCCL takes on a multi-GPU node)."""
    out_path = str(tmp_path / "gathered.pt")
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HANDS_SYNTHETIC_MANO="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dp_worker.py"), out_path, str(bz), "11",
                                       where], env=env))
    for p in procs:
        assert p.wait(timeout=600) == 0
    got = torch.load(out_path)
    import copy
    model = copy.deepcopy(recipe_model).to("cuda")
    inputs, meta = synthetic_inputs(bz, 11, device="cuda")
    meta["is_flipped"] = (torch.arange(bz, device="cuda") % 3 == 1).long()
    ref = model(inputs, meta)
    torch.cuda.synchronize()
    assert list(got.keys()) == list(ref.keys()) and len(got) == 22
    for k in ref:
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k].cpu()), k


def test_bench_launcher_starts_its_own_ranks():
    """`python bench.py --gpus 2` with WORLD_SIZE unset must start 2 rank processes itself (the driver calls it
    that way) and print ONE line with n_gpus = 2.  Dry run of that path on the 1-GPU box: both ranks share
    cuda:0 and gather through gloo (HANDS_BENCH_SHARE_GPU / HANDS_BENCH_BACKEND; never set by the driver)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(HANDS_BENCH_SHARE_GPU="1", HANDS_BENCH_BACKEND="gloo", HANDS_BENCH_GLOO_DEVICE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--bz", "8", "--no-cpu-baseline", "--full"], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["rccl_ranks"] == 2 and d["config"]["global_batch"] == 16
    assert d["config"]["launched_by"] == "bench.py launcher" and d["value"] > 0
    assert d["roofline"]["kernel_ms_per_step"] <= d["roofline"]["step_ms_same_mode"]
    assert p.stdout.splitlines()[-1] == lines[0] and len(lines[0]) < 4096      # stdout is the headline alone, short
    # N > 1 keys (VERDICT r3 item 6 i): the collective alone, the host side of a step, every rank's own rate
    assert d["allgather_us"] > 0 and d["host_enqueue_ms_per_step"] > 0
    assert 0 < d["per_rank_hands_per_sec"]["min"] <= d["per_rank_hands_per_sec"]["max"]
    assert d["cpu_baseline"] is None          # rank 0 at N = 1 only


def test_bench_at_the_drivers_arguments_two_ranks():
    """The driver's SCALE command line -- `python bench.py --gpus 2 --steps 20 --warmup 5`, default workload and batch size
    (bz = 256 per rank) -- with --full (the roofline and all-gather keys checked below), end to end once, on the 1-GPU box
    (both ranks on cuda:0, gloo staging the device tensors): one parseable headline as the last stdout line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(HANDS_BENCH_SHARE_GPU="1", HANDS_BENCH_BACKEND="gloo", HANDS_BENCH_GLOO_DEVICE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5", "--full"],
                       env=env, capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-2000:]
    last = p.stdout.splitlines()[-1]
    assert len(last) < 4096
    d = json.loads(last)
    assert d["n_gpus"] == 2 and d["steps"] == 20 and d["warmup"] == 5 and d["scaling"] == "weak"
    assert d["config"]["per_gpu_batch"] == 256 and d["config"]["global_batch"] == 512 and d["config"]["rccl_ranks"] == 2
    assert d["value"] > 0 and abs(d["value"] - 2 * 2 * 256 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    assert d["roofline"]["frac"] > 0 and d["allgather_us"] > 0


def test_bench_default_run_prints_one_stdout_line():
    """`python bench.py --full` (N = 1, with the extra measurements of configs 3-5): stdout is exactly ONE line -- the headline with
    roofline, cpu_baseline and parity -- below 4 KB; the extra measurements are short JSON lines on stderr."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--bz", "16", "--full"], env=env,
                       capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.strip().splitlines()
    assert len(out) == 1 and len(out[0]) < 4096
    d = json.loads(out[0])
    assert d["n_gpus"] == 1 and d["metric"] == "hands/sec" and d["config"]["per_gpu_batch"] == 16 and d["dtype"] == "f32"
    assert d["roofline"]["frac"] > 0 and d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] == "port"
    assert d["parity"]["max_vertex_err_m"] < 1e-6 and d["parity"]["worst_vertex_err_m"] < 1e-6
    also = [json.loads(l) for l in p.stderr.splitlines() if l.startswith("{") and '"also"' in l]
    assert {a["also"] for a in also} >= {"hamer_light", "handoccnet_light", "mano_lbs"} and set(d["also"]) == {a["also"] for a in also}
    assert all(len(json.dumps(a)) < 2048 for a in also)


def test_bench_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path, recipe_model):
    """A plain `bench.py --gpus 1 --steps K --warmup W` (no --full): one headline line with the contract keys and nothing
    measured beyond the K steps; --dump-outputs writes the 22 outputs of the last timed step, identical in two runs (seeded
    inputs) and equal to the forward of the same inputs in this process."""
    import copy
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dumps = []
    for run in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--bz", "4", "--dump-outputs", str(tmp_path / run)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        out = p.stdout.strip().splitlines()
        assert len(out) == 1 and len(out[0]) < 4096
        d = json.loads(out[0])
        assert d["metric"] == "hands/sec" and d["unit"] == "hands/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["config"]["per_gpu_batch"] == 4
        assert d["value"] > 0 and abs(d["value"] - 2 * 4 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
        assert d["roofline"] is None and d["cpu_baseline"] is None and d["parity"] is None and "also" not in d
        dumps.append({f[:-4]: np.load(tmp_path / run / f) for f in os.listdir(tmp_path / run)})
    assert len(dumps[0]) == 22 and dumps[0].keys() == dumps[1].keys()
    for k, a in dumps[0].items():
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, dumps[1][k]), k
    model = copy.deepcopy(recipe_model).to("cuda")
    model.overlap_trunks = True                  # bench.py's timed mode
    inputs, meta = synthetic_inputs(4, 0, device="cuda")
    ref = {k: v.detach().cpu().double().numpy() for k, v in model(inputs, meta).items()}
    torch.cuda.synchronize()
    assert ref.keys() == dumps[0].keys()
    for k, a in dumps[0].items():
        assert a.shape == ref[k].shape and np.allclose(a, ref[k], rtol=1e-5, atol=1e-6), k


def test_bench_under_torchrun_two_ranks():
    """The driver's N > 1 command: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...` -- every process is a rank (no launcher), rank 0 prints the one headline.  Dry run on the
    1-GPU box (both ranks on cuda:0, gloo staging the device tensors)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(HANDS_BENCH_SHARE_GPU="1", HANDS_BENCH_BACKEND="gloo", HANDS_BENCH_GLOO_DEVICE="1")
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps",
                        "3", "--warmup", "1", "--bz", "8", "--no-cpu-baseline", "--full"], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and p.stdout.strip().splitlines()[-1] == lines[0]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["config"]["launched_by"] == "torchrun" and d["config"]["rccl_ranks"] == 2
    assert d["config"]["global_batch"] == 16 and d["value"] > 0 and d["allgather_us"] > 0


def test_bench_hamer_light_two_rank_dry_run():
    """`bench.py --workload hamer_light --gpus 2` (BASELINE configs[2], weak scaling; reduced to bz=4 per rank here)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(HANDS_BENCH_SHARE_GPU="1", HANDS_BENCH_BACKEND="gloo", HANDS_BENCH_GLOO_DEVICE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--workload", "hamer_light", "--bz", "4", "--no-cpu-baseline", "--full"], env=env, capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.splitlines()[-1])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["rccl_ranks"] == 2 and d["config"]["global_batch"] == 8
    assert d["config"]["workload"].startswith("hamer_light") and d["value"] > 0 and d["allgather_us"] > 0


@pytest.mark.parametrize("workload,global_bz", [("handoccnet_light", 256), ("mano_lbs", 1024)])
def test_bench_strong_scaling_dry_runs(workload, global_bz):
    """`bench.py --workload handoccnet_light|mano_lbs --gpus 2`: the fixed-global-batch configs (BASELINE configs[3] /
    [4]) split 256 / 1024 over the ranks ("scaling": "strong").  Dry run on the 1-GPU box: two ranks share cuda:0,
    gloo stages the device tensors (the stream-ordered gather path RCCL takes)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(HANDS_BENCH_SHARE_GPU="1", HANDS_BENCH_BACKEND="gloo", HANDS_BENCH_GLOO_DEVICE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--workload", workload, "--no-cpu-baseline", "--full"], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["rccl_ranks"] == 2
    assert d["config"]["global_batch"] == global_bz and d["config"]["per_gpu_batch"] == global_bz // 2
    assert d["value"] > 0 and d["roofline"]["frac"] > 0
    if workload == "handoccnet_light":           # N > 1: the hipGraph replay with four captured forwards in flight is the timed mode
        assert "hipgraph(depth=4)" in d["config"]["timed_mode"], d["config"]
