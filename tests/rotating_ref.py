"""Inputs of the stratified (rotating item blocks) schedule for its tests — one builder instead of one per test file:
per-rank strata with LOCAL ids (whisprrec_amd/rotating.py: user u of rank g is global user u * G + g, row i of block b is
global item i * G + b), and the same steps as GLOBAL batches (the union of the ranks' k-th local batches), which is what the
single-process references — the fp32 C oracle and oracle/parity.py's float64 loop — are run on.  Plain NumPy, no GPU."""
import numpy as np

from whisprrec_amd.sharded import n_local_rows


def part_range(nI, world, parts, block, k):
    """RotatingBprmf.part_range without the object: local-row range [lo, hi) of part k of `block`"""
    n = n_local_rows(nI, block, world)
    per = (n + parts - 1) // parts
    return min(n, k * per), min(n, (k + 1) * per)


class Schedule:
    """U, I: the start tables (float32).  strata[rank][r] = (u, p, n, steps_per_part): stratum r of `rank`, local ids (int64),
    in batch order, the steps of part 0 first; rank trains it on block (rank + r) % world.  gu, gp, gn: the global id columns
    of all world * epochs * S steps in step order, `world * B` ids per step (rank 0's batch first)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def S(self):
        return sum(self.steps_per_part)

    @property
    def n_steps(self):
        return self.n_strata * self.S

    def part_range(self, block, k):
        return part_range(self.nI, self.world, self.parts, block, k)

    def cut(self, rank, g0, count):
        """Steps [g0, g0 + count) of `rank`'s ONE continuous run as the entries rotating.bench_run.make_pieces hands to
        run_strata / prepare: [(u, p, n, per_part, ends)], one entry per stratum the window meets.  per_part[k]: steps of part k
        inside the window; ends[k]: part k's last step lies inside it; p and n count rows from the start of their part
        (part_relative=True).  A window never hands a part over twice: a part ends in the entry that holds its last step."""
        S, B = self.S, self.B
        part_end = np.cumsum(self.steps_per_part)
        pieces, gs, g1 = [], int(g0), int(g0) + int(count)
        while gs < g1:
            r, o0 = gs // S, gs % S
            o1 = min(S, o0 + (g1 - gs))
            u, p, n, spp = self.strata[rank][r]
            held = (rank + r) % self.world
            per_part, ends, cols = [], [], []
            for k in range(self.parts):
                a, b = int(part_end[k] - spp[k]), int(part_end[k])
                lo_s, hi_s = max(o0, a), min(o1, b)
                per_part.append(max(0, hi_s - lo_s))
                ends.append(bool(o0 < b <= o1) if spp[k] > 0 else bool(o1 == S))
                if hi_s > lo_s:
                    lo = self.part_range(held, k)[0]
                    sl = slice(lo_s * B, hi_s * B)
                    cols.append((u[sl], p[sl] - lo, n[sl] - lo))
            pieces.append(tuple(np.concatenate([c[j] for c in cols]) for j in range(3)) + (per_part, ends))
            gs += o1 - o0
        return pieces


def make_schedule(world, parts, epochs, nU, nI, D, B, steps_per_part, seed, scale, neg_from_one=False):
    """world * epochs strata per rank, steps_per_part[k] batches of B triplets on part k of the held block, positives and
    negatives uniform inside the part; tables N(0, scale^2).  One RandomState(seed), drawn in the order the tests have
    always drawn: U, I, then rank by rank, stratum by stratum, part by part: users, positives, negatives.
    neg_from_one: negatives never hit global item 0 (the reference never draws it as a negative; world 1 only)."""
    rng = np.random.RandomState(seed)
    steps_per_part = [int(s) for s in steps_per_part]
    assert len(steps_per_part) == parts and (world == 1 or not neg_from_one)
    U = (rng.standard_normal((nU, D)) * scale).astype(np.float32)
    I = (rng.standard_normal((nI, D)) * scale).astype(np.float32)
    n_strata, S = world * epochs, sum(steps_per_part)
    strata = [[None] * n_strata for _ in range(world)]
    glob = [[None] * world for _ in range(n_strata)]
    for rank in range(world):
        n_loc_u = n_local_rows(nU, rank, world)
        for r in range(n_strata):
            held = (rank + r) % world
            us, ps, ns = [], [], []
            for k in range(parts):
                lo, hi = part_range(nI, world, parts, held, k)
                hi = max(hi, lo + 1)
                cnt = steps_per_part[k] * B
                us.append(rng.randint(0, n_loc_u, cnt))
                ps.append(rng.randint(lo, hi, cnt))
                ns.append(rng.randint(max(lo, 1) if neg_from_one else lo, hi, cnt))
            u, p, n = (np.concatenate(c).astype(np.int64) for c in (us, ps, ns))
            strata[rank][r] = (u, p, n, steps_per_part)
            glob[r][rank] = (u * world + rank, p * world + held, n * world + held)        # back to global ids
    # step k of stratum r = the ranks' k-th local batches side by side
    gu, gp, gn = (np.concatenate([np.stack([glob[r][rank][j].reshape(S, B) for rank in range(world)], axis=1).reshape(-1)
                                  for r in range(n_strata)]) for j in range(3))
    return Schedule(U=U, I=I, strata=strata, gu=gu, gp=gp, gn=gn, world=world, parts=parts, epochs=epochs, n_strata=n_strata,
                    nU=nU, nI=nI, D=D, B=B, steps_per_part=steps_per_part)
