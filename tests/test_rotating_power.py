"""What the parity checks of the stratified (rotating item blocks) schedule can and cannot see (CPU only; oracle/parity.py,
tests/rotating_ref.py; the pattern of tests/test_parity_power.py).

The schedule's GPU tests compare with the single-process step on the GLOBAL batches.  Floor: the fp32 C oracle on those batches
at probe_lr(B * world) against the float64 reference — never the code under test — with the ids, seeds and table scales of the
GPU tests.  Every floor leaves the factor 4 under the unchanged parity.TOL_UPDATE / TOL_ROW.

Power: seven wrong runs exceed TOL_ROW at the probe rate — the five of test_parity_power and two that only a ring can make (a
part trained before it landed or sent before its last step: one step's update of a whole part lost; a row at a part boundary
that the hand-over missed).  conftest.rel_err < 1e-5 at lr = 0.3, the only bound these tests had, passes an update that is 1 %
too large and a stale read of a row the step before rewrote — that is asserted, as the recorded reason for the probe runs."""
import functools

import numpy as np
import pytest

import oracle
from conftest import rel_err
from oracle import parity
from rotating_ref import make_schedule
from test_parity_power import _c_oracle_run, _mutants

OLD_LR = 0.3

# name -> make_schedule arguments of the GPU test the case stands for
CASES = {
    # test_hip_rotating_loopback.py::test_virtual_ranks_epoch_equals_single_process (seed world * 7 + parts)
    "loopback_w2_p2": dict(world=2, parts=2, epochs=2, nU=6000, nI=4002, D=64, B=2048, steps_per_part=[3, 3], seed=16, scale=0.3),
    "loopback_w3_p2": dict(world=3, parts=2, epochs=2, nU=6000, nI=4003, D=64, B=2048, steps_per_part=[3, 3], seed=23, scale=0.3),
    "loopback_w4_p3": dict(world=4, parts=3, epochs=2, nU=6000, nI=4004, D=64, B=2048, steps_per_part=[3, 3, 3], seed=31,
                           scale=0.3),
    # test_hip_rotating_two_ranks.py (seed world * 10 + parts, one epoch)
    "real_ranks_w2_p2": dict(world=2, parts=2, epochs=1, nU=6000, nI=4002, D=64, B=2048, steps_per_part=[3, 3], seed=22,
                             scale=0.3),
    "real_ranks_w3_p2": dict(world=3, parts=2, epochs=1, nU=6000, nI=4003, D=64, B=2048, steps_per_part=[3, 3], seed=32,
                             scale=0.3),
    # test_hip_sharded.py::test_rotating_world1_matches_oracle
    "world1": dict(world=1, parts=2, epochs=3, nU=3000, nI=2001, D=64, B=4096, steps_per_part=[2, 3], seed=21, scale=0.3,
                   neg_from_one=True),
    # test_hip_rotating_loopback.py::test_virtual_ranks_epoch_on_the_chained_launch
    "chain_shape": dict(world=2, parts=2, epochs=1, nU=40_000, nI=196_610, D=64, B=8192, steps_per_part=[2, 2], seed=5,
                        scale=0.3),
}
POWER = ("loopback_w2_p2", "loopback_w3_p2")


@functools.lru_cache(maxsize=None)
def _case(name):
    s = make_schedule(**CASES[name])
    return s, s.B * s.world, parity.probe_lr(s.B * s.world)


@functools.lru_cache(maxsize=None)
def _floor(name):
    s, GB, lr = _case(name)
    ref = parity.bprmf_sgd_f64(s.U, s.I, s.gu, s.gp, s.gn, GB, lr)
    fig = parity.sgd_run_errors(s.U, s.I, ref, *_c_oracle_run(s.U, s.I, s.gu, s.gp, s.gn, GB, lr))
    print("floor rotating %s: lr %.4g update/table %.1e update_err %.2e row_update_err %.2e table_err %.2e" % (
        name, lr, fig["update_over_table"], fig["update_err"], fig["row_update_err"], fig["table_err"]))
    return fig, ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_floor_leaves_a_factor_four(name):
    f = _floor(name)[0]
    assert 4 * f["update_err"] < parity.TOL_UPDATE and 4 * f["row_update_err"] < parity.TOL_ROW
    assert f["table_err"] < parity.TOL_TABLE


def _ring_run(s, lr, mutant):
    """the fp32 C oracle on the global batches, step by step, with one of the ring's own mistakes:
    part_step_lost: after the first step of stratum 1 on part 0, the rows of that part of the block rank 0 holds are put back
    to their values from before that step (the part was trained before it had landed, or sent before its last step);
    boundary_row_stale: one row at a part boundary keeps, through stratum 1, the value it had before that stratum — the row of
    a block whose size differs from a ring neighbour's where there is one (the hand-over sends part_range(held, k) and receives
    part_range(next, k): those ranges differ exactly there), of block 0 otherwise."""
    G, GB, S = s.world, s.B * s.world, s.S
    U, I = s.U.copy(), s.I.copy()
    if mutant == "part_step_lost":
        lo, hi = s.part_range(1 % G, 0)
        rows = np.arange(lo, hi) * G + 1 % G
        first, last = S, S                                   # saved before, put back after this step
    else:
        sizes = [s.part_range(b, s.parts - 1)[1] for b in range(G)]
        b = next((b for b in range(G) if sizes[b] != sizes[(b + 1) % G] or sizes[b] != sizes[(b - 1) % G]), 0)
        rows = np.array([s.part_range(b, 1)[0] * G + b])
        first, last = S, 2 * S - 1
        sl = slice(first * GB, (last + 1) * GB)
        assert np.isin(rows, np.concatenate([s.gp[sl], s.gn[sl]])).all(), "the stratum never touches the boundary row"
    for k in range(s.n_steps):
        sl = slice(k * GB, (k + 1) * GB)
        if k == first:
            kept = I[rows].copy()
        oracle.bprmf_step_sgd(U, I, s.gu[sl], s.gp[sl], s.gn[sl], lr, 0.0)
        if k == last:
            I[rows] = kept
    return U, I


def _all_mutants(s, lr):
    yield from _mutants(s.U, s.I, s.gu, s.gp, s.gn, s.B * s.world, lr)
    for mutant in ("part_step_lost", "boundary_row_stale"):
        yield mutant, _ring_run(s, lr, mutant)


@pytest.mark.parametrize("name", POWER)
def test_wrong_runs_are_rejected_at_probe_lr_and_were_not_before(name):
    s, GB, lr = _case(name)
    ref = _floor(name)[1]
    for mutant, (Um, Im) in _all_mutants(s, lr):
        f = parity.sgd_run_errors(s.U, s.I, ref, Um, Im)
        print("rotating %s %s at probe lr: update_err %.2e row_update_err %.2e" % (name, mutant, f["update_err"],
                                                                                   f["row_update_err"]))
        assert f["row_update_err"] > parity.TOL_ROW, (mutant, f)
    Uo, Io = _c_oracle_run(s.U, s.I, s.gu, s.gp, s.gn, GB, OLD_LR)
    for mutant, (Um, Im) in _all_mutants(s, OLD_LR):
        e = max(rel_err(Um, Uo), rel_err(Im, Io))
        print("rotating %s %s at lr %g: rel_err %.2e" % (name, mutant, OLD_LR, e))
        if mutant in ("update_x_1.01", "stale_read"):
            assert e < 1e-5, (mutant, e)


def test_cut_pieces_are_the_continuous_run():
    """Schedule.cut: whatever the cuts, every step is handed out once and in order, every part ends once per stratum, and the
    part-relative columns are the strata's columns minus their part's first row"""
    s = _case("loopback_w3_p2")[0]
    B, S = s.B, s.S
    for rank in range(s.world):
        pos, seen, ended = 0, [[], [], []], []
        for length in (2, 1, 3, 4, 7, 5, 6, 8):
            for entry in s.cut(rank, pos, length):
                per_part, ends = entry[3], entry[4]
                r = pos // S
                assert entry[0].size == sum(per_part) * B and pos % S + sum(per_part) <= S
                ended += [(r, k) for k in range(s.parts) if ends[k]]
                for j in range(3):
                    seen[j].append(entry[j])
                pos += sum(per_part)
        assert pos == s.n_steps and ended == [(r, k) for r in range(s.n_strata) for k in range(s.parts)]
        first_row = np.concatenate([np.repeat([s.part_range((rank + r) % s.world, k)[0] for k in range(s.parts)],
                                              np.asarray(s.steps_per_part) * B) for r in range(s.n_strata)])
        for j in range(3):
            whole = np.concatenate([st[j] for st in s.strata[rank]])
            assert np.array_equal(np.concatenate(seen[j]), whole - first_row if j else whole)
