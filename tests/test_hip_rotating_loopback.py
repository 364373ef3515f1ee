"""The stratified multi-GPU schedule with several VIRTUAL ranks on one GPU: every rank is a thread with its own streams,
the ring transfers are in-process device copies ordered by events exactly like the RCCL P2P calls (the receiver's stream
waits for the sender's data, the sender's stream waits for the receiver's copy).  Unlike the CPU/gloo test this runs the real
kernels asynchronously, so a missing wait in the rotation (a part trained before it landed, a part overwritten before it was
sent) shows up as a mismatch with the single-process oracle on the GLOBAL batches.

Every run is made twice from the same tables: at lr = 0.3 against the fp32 C oracle (conftest.rel_err on the tables), and at
parity.probe_lr(B * world) against the float64 reference, measured on the UPDATE (oracle/parity.py) — the first metric passes
an update that is 1 % off and a stale read of a rewritten row, the second does not (tests/test_rotating_power.py)."""
import queue
import threading

import numpy as np
import pytest
import torch

import oracle
from conftest import rel_err
from oracle import parity
from rotating_ref import make_schedule

pytestmark = pytest.mark.gpu


class _Shared:
    def __init__(self, world):
        self.world = world
        self.q = {(a, b): queue.Queue() for a in range(world) for b in range(world)}
        self.ack = {(a, b): queue.Queue() for a in range(world) for b in range(world)}
        self.barrier = threading.Barrier(world, timeout=120)
        self.slots = [None] * world


class LoopbackTransport:
    def __init__(self, shared, rank):
        self.sh, self.rank, self.world = shared, rank, shared.world

    def exchange(self, send_buf, dst, recv_buf, src):
        cur = torch.cuda.current_stream()
        if send_buf is not None:
            ev = torch.cuda.Event(); ev.record(cur)
            self.sh.q[(self.rank, dst)].put((send_buf, ev))
        if recv_buf is not None:
            buf, ev = self.sh.q[(src, self.rank)].get(timeout=120)
            cur.wait_event(ev)
            torch.cuda._sleep(40_000_000)     # a slow link (~20 ms): whoever touches the part without waiting reads stale rows
            recv_buf.copy_(buf)
            ack = torch.cuda.Event(); ack.record(cur)
            self.sh.ack[(src, self.rank)].put(ack)
        if send_buf is not None:
            cur.wait_event(self.sh.ack[(self.rank, dst)].get(timeout=120))   # send buffer free from here on (stream order)

    def all_gather(self, t):
        torch.cuda.current_stream().synchronize()
        # every rank is a thread with a stream of its own: a copy is finished, not merely queued, before another rank may read
        # it (first barrier) or its owner may drop it (second barrier)
        cur = torch.cuda.current_stream()
        self.sh.slots[self.rank] = t.clone()
        cur.synchronize()
        self.sh.barrier.wait()
        out = [self.sh.slots[r].clone() for r in range(self.world)]
        cur.synchronize()
        self.sh.barrier.wait()
        return out

    def all_reduce_sum(self, t):
        return torch.stack(self.all_gather(t)).sum(0)


def _oracle_run(sch, lr, n_steps=None):
    """the fp32 C oracle on the first n_steps global batches (default: all): (losses, U, I)"""
    Uo, Io = sch.U.copy(), sch.I.copy()
    GB = sch.B * sch.world
    ref = [oracle.bprmf_step_sgd(Uo, Io, sch.gu[k * GB:(k + 1) * GB], sch.gp[k * GB:(k + 1) * GB], sch.gn[k * GB:(k + 1) * GB],
                                 lr, 0.0) for k in range(sch.n_steps if n_steps is None else n_steps)]
    return np.asarray(ref), Uo, Io


@pytest.mark.parametrize("world,parts,chunk", [(2, 2, 2), (3, 2, 64), (4, 3, 1)])
def test_virtual_ranks_epoch_equals_single_process(world, parts, chunk):
    from whisprrec_amd import hip_ops
    from whisprrec_amd.rotating import RotatingBprmf
    dev = torch.device("cuda:0")
    nU, nI, D, B, lr, epochs = 6000, 4000 + world, 64, 2048, 0.3, 2
    steps_per_part = [3] * parts
    sch = make_schedule(world, parts, epochs, nU, nI, D, B, steps_per_part, seed=world * 7 + parts, scale=0.3)
    U, I, strata = sch.U, sch.I, sch.strata
    probe_lr = parity.probe_lr(B * world)
    shared = _Shared(world)
    results, probes, errors = [None] * world, [None] * world, []

    def worker(rank):
        try:
            main = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(main):
                local = hip_ops.PipelinedSgd(chunk)
                local.PLAN_TRIPLETS = 1      # plans of exactly `chunk` batches: chunk ends fall inside and across the strata
                m = RotatingBprmf(nU, nI, D, dev, parts=parts, local=local, transport=LoopbackTransport(shared, rank))
                m.load_full(torch.from_numpy(U), torch.from_numpy(I))
                t = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
                sched = [(t(u), t(p), t(n), steps_per_part) for (u, p, n, _) in strata[rank]]
                losses = m.run_strata(sched, B, lr)
                gl = m.global_losses(losses)
                Uf, If = m.gather_full()
                main.synchronize()
                results[rank] = (gl.cpu().numpy(), Uf.cpu().numpy(), If.cpu().numpy(), m.held)
                m.load_full(torch.from_numpy(U), torch.from_numpy(I))      # probe run (oracle/parity.py) from the same tables
                gl = m.global_losses(m.run_strata(sched, B, probe_lr))
                Uf, If = m.gather_full()
                main.synchronize()
                probes[rank] = (gl.cpu().numpy(), Uf.cpu().numpy(), If.cpu().numpy(), m.held)
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append((rank, repr(e)))
            try:
                shared.barrier.abort()
            except Exception:
                pass

    threads = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
    assert not errors, errors
    assert all(not th.is_alive() for th in threads), "a virtual rank hangs"
    ref, Uo, Io = _oracle_run(sch, lr)
    for rank in range(world):
        gl, Uf, If, held = results[rank]
        assert held == rank
        assert rel_err(gl, np.asarray(ref)) < 1e-5
        assert rel_err(Uf, Uo) < 1e-5 and rel_err(If, Io) < 1e-5
    _check_probe("rotating %d virtual ranks, %d parts, plans of %d" % (world, parts, chunk), sch, probes)
    assert all(pr[3] == rank for rank, pr in enumerate(probes))


def _check_probe(tag, sch, probes, n_steps=None):
    """the probe run's tables as every rank gathered them: rank 0's against the float64 reference, the others' equal to them
    (gather_full hands every rank the same bytes)"""
    gl, Uf, If = probes[0][:3]
    for other in probes[1:]:
        assert np.array_equal(other[0], gl) and np.array_equal(other[1], Uf) and np.array_equal(other[2], If)
    GB = sch.B * sch.world
    return parity.check_sgd_run(tag, sch.U, sch.I, sch.gu, sch.gp, sch.gn, GB, parity.probe_lr(GB), Uf, If, gl, n_steps=n_steps)


def _virtual_ranks(sch, chunk, lrs, drive):
    """Every rank a thread with its own streams; for every lr in turn a fresh RotatingBprmf over PipelinedSgd(chunk,
    min_triplets=1) — bench.py's runner: plans of exactly `chunk` batches — is loaded with the schedule's tables and driven by
    drive(m, rank, lr, to_device) -> this rank's local losses.  Returns out[lr index][rank] = (global losses, U, I, held,
    the runner's stats) as gather_full and global_losses gave them on that rank."""
    from whisprrec_amd import hip_ops
    from whisprrec_amd.rotating import RotatingBprmf
    dev = torch.device("cuda:0")
    world = sch.world
    shared = _Shared(world)
    out, errors = [[None] * world for _ in lrs], []

    def worker(rank):
        try:
            main = torch.cuda.Stream(device=dev)
            keep = []                                   # no buffer is given back while a side stream may still write to it
            with torch.cuda.stream(main):
                t = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)
                for j, lr in enumerate(lrs):
                    local = hip_ops.PipelinedSgd(chunk, min_triplets=1)
                    m = RotatingBprmf(sch.nU, sch.nI, sch.D, dev, parts=sch.parts, local=local,
                                      transport=LoopbackTransport(shared, rank))
                    keep.append(m)
                    m.load_full(torch.from_numpy(sch.U), torch.from_numpy(sch.I))
                    gl = m.global_losses(drive(m, rank, lr, t))
                    Uf, If = m.gather_full()
                    torch.cuda.synchronize()            # every rank's transfers are queued by now (gather_full's barriers)
                    out[j][rank] = (gl.cpu().numpy(), Uf.cpu().numpy(), If.cpu().numpy(), m.held, dict(local.stats))
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append((rank, repr(e)))
            try:
                shared.barrier.abort()
            except Exception:
                pass

    threads = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=300)
    assert not errors, errors
    assert all(not th.is_alive() for th in threads), "a virtual rank hangs"
    return out


@pytest.mark.parametrize("ends", ["epoch_end", "mid_epoch"])
@pytest.mark.parametrize("world,parts,chunk", [(2, 2, 2), (3, 2, 64)])
def test_virtual_ranks_pieces_as_the_benchmark_cuts_them(world, parts, chunk, ends):
    """bench.py --gpus N, mode 'rotate' (rotating.bench_run): ONE continuous run cut into pieces at the same steps on every
    rank.  The pieces carry per-part end flags and part-relative ids and leave their last hand-over to the next call
    (defer_last); the last trained piece is prepare()d together with a spare piece that is planned and never trained, and run
    with run_prepared(n_strata=); complete_rotation() closes the ring.  The trained steps end on an epoch's last step (every
    block is home again) or in the middle of an epoch, on a part's last step with its stratum still open (gather_full
    re-assembles the item table by `held`; the reference stops at the trained steps)."""
    nU, nI, D, B, lr, epochs = 6000, 4000 + world, 64, 2048, 0.3, 2
    steps_per_part = [3] * parts
    # one epoch more than is trained: the spare piece needs ids too
    sch = make_schedule(world, parts, epochs + 1, nU, nI, D, B, steps_per_part, seed=world * 7 + parts, scale=0.3)
    S = sch.S
    trained = world * epochs * S - (0 if ends == "epoch_end" else S - steps_per_part[0])
    n_timed, n_spare = 5, min(chunk, S)
    lengths = [2, 1, 3, 4]                              # ends: inside part 0, on part 0's last step, on a stratum's last step,
    while sum(lengths) < trained - n_timed:             # inside part 1; then pieces of 7 steps across the rotations
        lengths.append(min(7, trained - n_timed - sum(lengths)))
    part_end = set(np.cumsum(steps_per_part)[:-1].tolist())
    kinds = {"stratum" if g % S == 0 else "part" if g % S in part_end else "inside" for g in np.cumsum(lengths + [n_timed]).tolist()}
    assert kinds == {"stratum", "part", "inside"} and sum(lengths) + n_timed == trained
    held_after = lambda rank: (rank + trained // S) % world

    def drive(m, rank, run_lr, t):
        entries = lambda g0, count: [(t(u), t(p), t(n), per_part, flags) for (u, p, n, per_part, flags) in sch.cut(rank, g0, count)]
        losses, g0 = [], 0
        for length in lengths:
            losses.append(m.run_strata(entries(g0, length), B, run_lr, part_relative=True, defer_last=True))
            g0 += length
        timed, spare = entries(g0, n_timed), entries(g0 + n_timed, n_spare)
        prep = m.prepare(timed + spare, B, part_relative=True)
        losses.append(m.run_prepared(prep, run_lr, n_strata=len(timed), defer_last=True))
        m.complete_rotation()
        assert m.held == held_after(rank)
        return torch.cat(losses)

    got, probes = _virtual_ranks(sch, chunk, [lr, parity.probe_lr(B * world)], drive)
    ref, Uo, Io = _oracle_run(sch, lr, trained)
    for rank in range(world):
        gl, Uf, If, held, _ = got[rank]
        assert held == held_after(rank) and (ends != "epoch_end" or held == rank)
        assert rel_err(gl, ref) < 1e-5
        assert rel_err(Uf, Uo) < 1e-5 and rel_err(If, Io) < 1e-5
    # all columns, n_steps = the trained steps: the rows only the spare piece names are in the comparison, and untouched
    _check_probe("rotating pieces, %d virtual ranks, plans of %d, %s" % (world, chunk, ends), sch, probes, n_steps=trained)


def test_virtual_ranks_epoch_on_the_chained_launch():
    """The rotation under the chained step launch (run_sgd_chain: step k-1's item phase inside step k's launch).  PipelinedSgd
    takes it from B = CHAIN_MIN_BATCH = 8,192 on and only when every part has 6 B item rows: parts of 49,153 and 49,152 rows
    (6 B = 49,152), blocks of 98,305 rows = 25 MB per buffer.  Plans of two batches, two steps per part: every launch sequence
    ends where a part is handed to the ring."""
    world, parts, chunk = 2, 2, 2
    nU, nI, D, B, lr = 40_000, 196_610, 64, 8192, 0.3
    steps_per_part = [2, 2]
    sch = make_schedule(world, parts, 1, nU, nI, D, B, steps_per_part, seed=5, scale=0.3)

    def drive(m, rank, run_lr, t):
        return m.run_strata([(t(u), t(p), t(n), steps_per_part) for (u, p, n, _) in sch.strata[rank]], B, run_lr)

    got, probes = _virtual_ranks(sch, chunk, [lr, parity.probe_lr(B * world)], drive)
    for rank in range(world):
        assert got[rank][4]["chain_calls"] > 0 and probes[rank][4]["chain_calls"] > 0, (got[rank][4], probes[rank][4])
    ref, Uo, Io = _oracle_run(sch, lr)
    for rank in range(world):
        gl, Uf, If, held, _ = got[rank]
        assert held == rank
        assert rel_err(gl, ref) < 1e-5
        assert rel_err(Uf, Uo) < 1e-5 and rel_err(If, Io) < 1e-5
    _check_probe("rotating chained launch, %d virtual ranks, B %d" % (world, B), sch, probes)
