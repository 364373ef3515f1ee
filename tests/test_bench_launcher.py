"""bench.py's N>1 entry on CPU: `python bench.py --gpus 2` as a plain command starts its own two ranks (child processes
through torch.distributed.run, nothing exec'ed, the parent never touches a GPU), the ranks rendezvous on 127.0.0.1 and rank 0
prints ONE JSON line in the driver's format.  `--dry-run --backend gloo` stops after the rendezvous (no GPU here); the line's
content for real results is checked on synthetic per-mode dicts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err

import bench


def _last_json(text):
    lines = [ln for ln in text.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, text
    return json.loads(lines[0])


def test_plain_command_starts_its_own_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5",
                        "--dry-run", "--backend", "gloo"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = _last_json(r.stdout)
    assert line["n_gpus"] == 2 and line["steps"] == 20 and line["warmup"] == 5 and line["dry_run"] is True
    assert line["config"]["rccl_world_size"] == 2 and line["config"]["global_batch"] == 2 * line["config"]["batch_per_gpu"]
    assert line["metric"] == "BPR training triplets/sec" and line["scaling"] == "weak" and line["unit"] == "triplets/s"


def test_under_torch_distributed_run_it_uses_the_given_ranks():
    """the driver's own launch line: python -m torch.distributed.run ... bench.py --gpus N"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(bench.free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2",
                        "--steps", "4", "--warmup", "1", "--dry-run", "--backend", "gloo"], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _last_json(r.stdout)["n_gpus"] == 2


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry-run"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stdout + r.stderr)


def test_multi_gpu_line_carries_both_modes_and_the_single_gpu_definitions():
    args = bench.parse(["--gpus", "8", "--steps", "20", "--warmup", "5", "--emb", "128", "--users", "10000000", "--items",
                        "10000000"])
    rot = {"value": 8e9, "ms_per_step": 0.05, "parallelism": "stratified-rotation x8", "sampling": "stratified: ...",
           "roofline": {"bound": "hbm", "achieved": 3000.0, "peak": 8000.0, "unit": "GB/s", "frac": 0.375, "traffic": None,
                        "definition": "2*D*4*(unique users + unique items of the local batch) + 12*B, as at N=1"}}
    a2a = {"value": 2e9, "ms_per_step": 0.2, "parallelism": "row-sharded tables x8, RCCL all-to-all",
           "sampling": "reference rule", "roofline": dict(rot["roofline"], achieved=700.0, frac=0.0875)}
    line = bench.multi_line(args, 8, {"rotate": rot, "alltoall": a2a}, {"value": 1e6, "unit": "triplets/s", "cores": 1,
                                                                         "kind": "port", "sample": "x"})
    # the headline is the mode that keeps the reference's sampling (all-to-all); the rotation is reported beside it
    assert line["value"] == 2e9 and line["config"]["value_from_mode"] == "alltoall" and line["n_gpus"] == 8
    assert set(line["modes"]) == {"rotate", "alltoall"} and line["modes"]["alltoall"]["value"] == 2e9
    assert line["config"]["sampling"].startswith("reference rule") and line["config"]["rccl_world_size"] == 8
    assert line["config"]["emb_size"] == 128 and "10000000 users" in line["config"]["workload"]
    assert line["roofline"]["definition"].endswith("as at N=1") and line["cpu_baseline"]["kind"] == "port"
    json.dumps(line)


def test_plan_chunk_of_a_short_run_is_the_run():
    assert bench.plan_chunk(bench.parse(["--steps", "20", "--warmup", "5"])) == 20
    assert bench.plan_chunk(bench.parse([])) == 64
    assert bench.plan_chunk(bench.parse(["--steps", "20", "--chunk", "7"])) == 7


def test_full_and_dump_outputs_are_off_by_default():
    args = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not args.full and args.dump_outputs is None
    assert bench.parse(["--full"]).full


def test_dump_outputs_is_refused_off_the_single_gpu_path(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--backend", "gloo",
                        "--dump-outputs", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--dump-outputs" in (r.stdout + r.stderr) and not (tmp_path / "out").exists()


@pytest.mark.gpu
def test_plain_run_dumps_what_its_timed_steps_computed(tmp_path):
    """a plain one-GPU run prints the headline without the --full parts, and --dump-outputs writes the same arrays (float32 /
    float64, within 64 MB) from run to run: the timed steps' losses and a fixed sample of rows of both tables"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--batch", "16384",
           "--users", "300000", "--items", "300000"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    lines = []
    for k in range(2):
        r = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / str(k))], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines.append(_last_json(r.stdout))
    line = lines[0]
    assert line["steps"] == 6 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["roofline"] is None and "extra" not in line and "cpu_baseline" not in line
    names = {"losses", "user_ids", "user_rows", "item_ids", "item_rows"}
    assert {f[:-len(".npy")] for f in os.listdir(tmp_path / "0")} == names
    got = {nm: [np.load(tmp_path / str(k) / (nm + ".npy")) for k in range(2)] for nm in names}
    assert sum(a[0].nbytes for a in got.values()) <= 64e6
    for nm, (a, b) in got.items():
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape, nm
    assert got["losses"][0].shape == (6,) and float(got["losses"][0][-1]) == line["loss_last"]
    for nm in ("user", "item"):
        ids, rows = got[nm + "_ids"][0], got[nm + "_rows"][0]
        assert np.array_equal(ids, got[nm + "_ids"][1]) and np.all(np.diff(ids) > 0) and rows.shape == (ids.size, 64)
        assert rel_err(rows, got[nm + "_rows"][1]) < 1e-6
    assert rel_err(got["losses"][0], got["losses"][1]) < 1e-6

    # the rows are the trained tables' and line up with their ids: with the tables and the triplet stream rebuilt here as
    # bench.single_gpu seeds them, a sampled row that no warm-up or timed step touched still holds its initial value, every
    # row of the last batch's dumped triplets is there, and those rows moved
    import torch
    args = bench.parse(cmd[2:])
    dev = torch.device("cuda:0")
    B, D, K, W = args.batch, args.emb, args.steps, args.warmup
    g = torch.Generator(device=dev)
    g.manual_seed(3407)
    U0 = torch.randn(args.users, D, generator=g, device=dev) * float(np.sqrt(2.0 / (args.users + D)))
    I0 = torch.randn(args.items, D, generator=g, device=dev) * float(np.sqrt(2.0 / (args.items + D)))
    u, p, n = bench.synth_triplets((K + W + bench.plan_chunk(args)) * B, args.users, args.items, dev, 3407, args.zipf)
    trained = slice(0, (W + K) * B)
    last = slice((W + K - 1) * B, (W + K - 1) * B + min(B, bench.DUMP_TRIPLETS))
    for nm, T0, cols in (("user", U0, (u,)), ("item", I0, (p, n))):
        ids, rows = got[nm + "_ids"][0].astype(np.int64), got[nm + "_rows"][0]
        init = T0[torch.from_numpy(ids).to(dev)].cpu().numpy()
        touched = np.isin(ids, torch.cat([c[trained] for c in cols]).cpu().numpy())
        last_ids = np.unique(torch.cat([c[last] for c in cols]).cpu().numpy())
        in_last = np.isin(ids, last_ids)
        assert in_last.sum() == last_ids.size, nm
        assert (~touched).sum() > 1000 and np.array_equal(rows[~touched], init[~touched]), nm
        assert np.mean(np.any(rows[in_last] != init[in_last], axis=1)) > 0.99, nm
