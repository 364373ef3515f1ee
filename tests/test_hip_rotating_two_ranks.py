"""The stratified (rotating item blocks) schedule with TWO and THREE real ranks on ONE GPU: every rank is a process running the
product's step stream (hip_ops.PipelinedSgd, real kernels on cuda:0), the ring transfers go through torch.distributed over
gloo, staged through the host (RCCL refuses several ranks on one device; on a node every rank has its own GPU and the backend
is RCCL, whose point-to-point calls are ordered with the streams).  A whole
epoch — every item block visits every rank — must equal the single-process oracle on the global batches.  (Threads as ranks
with an in-process transport: tests/test_hip_rotating_loopback.py; the schedule alone on CPU: tests/test_rotating_gloo.py.)"""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import oracle
from conftest import rel_err
from oracle import parity
from rotating_ref import make_schedule
from test_sharded_gloo import _free_port

pytestmark = pytest.mark.gpu


class StagedGlooTransport:
    """rotating.DistTransport's interface over gloo with HOST staging: gloo's point-to-point calls take the device pointer as
    it is (the host reads the card's memory through the PCIe aperture, unordered with the GPU's streams), so every buffer is
    brought to the host behind a stream synchronisation, exchanged as a CPU tensor, and copied back on the current stream —
    the ordering RCCL's stream-ordered P2P gives on a node."""

    def __init__(self):
        import torch.distributed as dist
        self.dist = dist
        self.rank, self.world = dist.get_rank(), dist.get_world_size()

    def exchange(self, send_buf, dst, recv_buf, src):
        dist = self.dist
        cur = torch.cuda.current_stream()
        ops, host_recv = [], None
        if send_buf is not None:
            cur.synchronize()
            ops.append(dist.P2POp(dist.isend, send_buf.cpu(), dst))
        if recv_buf is not None:
            host_recv = torch.empty(recv_buf.shape, dtype=recv_buf.dtype)
            ops.append(dist.P2POp(dist.irecv, host_recv, src))
        for w in (dist.batch_isend_irecv(ops) if ops else []):
            w.wait()
        if host_recv is not None:
            recv_buf.copy_(host_recv)

    def all_gather(self, t):
        torch.cuda.current_stream().synchronize()
        out = [torch.empty(t.shape, dtype=t.dtype) for _ in range(self.world)]
        self.dist.all_gather(out, t.cpu().contiguous())
        return [o.to(t.device) for o in out]

    def all_reduce_sum(self, t):
        torch.cuda.current_stream().synchronize()
        h = t.cpu()
        self.dist.all_reduce(h, op=self.dist.ReduceOp.SUM)
        t.copy_(h)
        return t


def _worker(rank, world, port, payload, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from whisprrec_amd import hip_ops
        from whisprrec_amd.rotating import RotatingBprmf
        nU, nI, D, B, lr, parts, chunk = payload["shape"]
        local = hip_ops.PipelinedSgd(chunk)
        local.PLAN_TRIPLETS = 1                       # plans of exactly `chunk` batches: chunk ends inside and across the strata
        m = RotatingBprmf(nU, nI, D, dev, parts=parts, local=local, transport=StagedGlooTransport())
        t = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
        sched = [(t(u), t(p), t(n), pp) for (u, p, n, pp) in payload["strata"][rank]]
        for tag, run_lr in (("", lr), ("_probe", payload["probe_lr"])):   # the test's run, then the probe run from the same tables
            m.load_full(torch.from_numpy(payload["U"]), torch.from_numpy(payload["I"]))
            losses = m.run_strata(sched, B, run_lr)
            assert m.held == rank                     # a full epoch brings every block home
            gl = m.global_losses(losses)
            Uf, If = m.gather_full()
            torch.cuda.synchronize()
            if rank == 0:
                np.savez(os.path.join(out_dir, "out%s.npz" % tag), U=Uf.cpu().numpy(), I=If.cpu().numpy(), loss=gl.cpu().numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,parts,chunk", [(2, 2, 2), (3, 2, 64)])
def test_rotating_epoch_real_ranks_one_gpu_equals_single_process(tmp_path, world, parts, chunk):
    nU, nI, D, B, lr = 6000, 4000 + world, 64, 2048, 0.3
    steps_per_part = [3] * parts
    sch = make_schedule(world, parts, 1, nU, nI, D, B, steps_per_part, seed=world * 10 + parts, scale=0.3)
    U, I, strata = sch.U, sch.I, sch.strata
    payload = dict(shape=(nU, nI, D, B, lr, parts, chunk), U=U, I=I, strata=strata, probe_lr=parity.probe_lr(B * world))
    mp.spawn(_worker, args=(world, _free_port(), payload, str(tmp_path)), nprocs=world, join=True)
    got = np.load(tmp_path / "out.npz")
    Uo, Io = U.copy(), I.copy()
    ref = []
    GB = B * world
    for k in range(world * sum(steps_per_part)):
        sl = slice(k * GB, (k + 1) * GB)                                                 # the ranks' k-th batches side by side
        ref.append(oracle.bprmf_step_sgd(Uo, Io, sch.gu[sl], sch.gp[sl], sch.gn[sl], lr, 0.0))   # ONE step over the global batch
    assert rel_err(got["loss"], np.asarray(ref)) < 1e-5
    assert rel_err(got["U"], Uo) < 1e-5
    assert rel_err(got["I"], Io) < 1e-5
    # probe run (oracle/parity.py): the global batch is B * world, so lr = probe_lr(B * world)
    got = np.load(tmp_path / "out_probe.npz")
    parity.check_sgd_run("rotating %d real ranks, %d parts, plans of %d" % (world, parts, chunk), U, I, sch.gu, sch.gp, sch.gn, GB,
                         parity.probe_lr(GB), got["U"], got["I"], got["loss"])
