"""CPU checks of the DISTRIBUTION of the device epoch preparation (wr_sample_negatives* / draw_negative, shuffle_index) through
its NumPy restatement.  tests/test_hip_sampler.py holds the kernels equal to the restatement bit for bit; that says nothing
about a rule that is biased on both sides.  Here the restatement faces the law the reference's rule implies (uniform over the
items of [1, n_items) the user has not clicked, src/models/BaseModel.py:167-177; a uniform random order of the rows,
src/helpers/BaseRunner.py:188-193) with the battery of tests/epoch_prep_ref.py.

* Calibration: every case runs twice, at the same sizes and under the same bound: on the reference's own generators
  (`oracle.sample_negatives(..., rng=RandomState(s))`, `RandomState(s).permutation(n)`; the arm "numpy") and on the
  restatement (the arm "restated").  The first proves the battery and its expectations before they judge anything of ours.
* Bound: |z| <= 4.9 per statistic (two-sided 1e-6).  Seeds are fixed: the tests are deterministic.  Run with -rP for every z.
* Power: every wrong generator must exceed TWICE the bound on some statistic.
* The two known deviations from the rule are pinned with their size: the cyclic walk after 64 failed attempts,
  and the single-position marginals of the shuffle below n = 16.

Measured (this file's output; "numpy" / "restated"):

  population (2,000 users with 1-60 clicked of 5,000 items, 200,000 rows), item_chi2        +1.38 / +0.57
  one user of 51 items, 200,000 rows: user_chi2 / equal_rate epochs 0, 1 / seeds 3407, 3408
      20 % clicked                                                                          -0.26 -0.46 -0.46 / -1.24 +0.26 -2.88
      80 % clicked                                                                          +1.43 +0.95 +0.07 / -0.58 -1.45 -0.64
      empty list                                                                            +0.05 +1.09 -0.42 / -2.06 +0.06 -1.58
  190 pairs of 20 streams (empty list, 1,000 items, 200,000 rows), equal_rate min / max     -2.91 +2.74 / -2.28 +3.10
  shuffle, K epochs: bucket_chi2 (G = 32) / successor_count / fixed_points / same_as_previous
      n = 1,000    K = 2,000                  -0.67 +1.63 -0.58 -1.10 / -0.36 +0.40 +1.23 -2.37
      n = 4,097    K = 1,000                  -0.90 -1.07 -0.25 +0.85 / -0.22 -1.16 +0.85 +0.35
      n = 8,192    K = 500                    -0.43 +1.43 -0.67 -0.27 / +0.86 +0.41 +0.72 +0.40
      n = 65,536   K = 200                    -0.20 -1.48 +1.91 -1.49 / +0.71 -0.49 +0.35 +0.43
      n = 100,003  K = 200                    +0.92 +1.27 -0.42 -0.14 / -1.86 +0.07 +1.20 -1.70
  batch_composition, n = 100,003, B = 2,048, G = 16, 8 epochs, min / max                    -1.06 +1.74 / -1.67 +1.40
  marginals (n x n cell table, 20,000 epochs), n = 16, 17, 32, 33, 64
                                              +1.17 -1.31 +0.72 +0.39 +0.75 / +0.38 +0.59 +1.60 -0.42 -1.55
  fallback share of item 10 (expects 0.548768, sd 0.001113)                                 0.54928, z +0.46

Wrong generators, the statistic that separates each (bound to exceed: 9.8):

  collision_next      user_chi2 +2542.6 (and 4,007 forbidden draws of 200,000)
  last_item_missing   user_chi2 +579.8
  zero_included       user_chi2 +564.8 (and 5,062 draws of item 0)
  epoch_ignored       equal_rate epochs 0, 1 +2792.9
  attempt_ignored     user_chi2 +3468.1
  rounds = 2          successor_count +428.9 (mean 10.59 where 1 is expected)
  rounds = 3          successor_count +14.3 (mean 1.319)
  rounds = 4          successor_count +12.9 (mean 1.288)
  rounds = 6          NOT separable at these sizes: successor_count +0.58, fixed_points +2.08, bucket_chi2 +1.70 (printed only)

The known deviation of the marginals, printed and not asserted (seed 3407 / seed 11; numpy at the same size): n = 5: +7.24 /
+3.46 (+0.56); n = 6: +4.64 / +3.35 (-0.72); n = 9: +2.62 / +0.99 (+0.77).  These carry the factor (n - 1) / n of a table with
both margins fixed (epoch_prep_ref._fixed_margin_chi2: Pearson's statistic of such a table expects n / (n - 1) times its
degrees of freedom); without the factor the figures at seed 3407 are 9.8, 6.3 and 3.6, and NumPy's own permutations move from
+0.56 to +1.41 at n = 5.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epoch_prep_ref as E  # noqa: E402

BOUND = E.BOUND
ROWS = 200_000
ARMS = ("numpy", "restated")
NI_USER = 51                                            # the single-user cases: 50 items to draw from
STREAMS = [(s, e) for s in (0, 1, 2, 3407, 3408) for e in (0, 1, 2, 3)]
SHUFFLE_K = {1000: 2000, 4097: 1000, 8192: 500, 65536: 200, 100003: 200}


def say(name, z, extra=""):
    print("z %-72s %+8.2f %s" % (name, z, extra))
    return z


def inside(name, z, extra=""):
    say(name, z, extra)
    assert abs(z) <= BOUND, "%s: z = %.2f outside %.1f sigma" % (name, z, BOUND)


def negatives(arm, users, n_items, ptr, idx, seed, epoch, wrong=None):
    if arm == "numpy":                                  # the reference's generator; (seed, epoch) only name the stream
        return oracle.sample_negatives(users, n_items, ptr, idx, rng=np.random.RandomState(seed * 16 + epoch))
    return E.sample_negatives_counter(users, n_items, ptr, idx, seed, epoch, wrong)


def orders(arm, n, seed, K, rounds=8):
    if arm == "numpy":
        rng = np.random.RandomState(seed)
        return np.stack([rng.permutation(n) for _ in range(K)])
    return E.permutations(n, seed, np.arange(K), rounds)


@functools.lru_cache(maxsize=None)
def population():
    """the large case of tests/test_hip_sampler.py, its first 200,000 rows"""
    rng = np.random.RandomState(0)
    n_users, n_items = 2000, 5000
    sets = {u: set(rng.randint(0, n_items, rng.randint(1, 60)).tolist()) for u in range(n_users)}
    users = rng.randint(0, n_users, 1_000_000)[:ROWS]
    return users, sets, E.csr(sets, n_users), n_items


@functools.lru_cache(maxsize=None)
def one_user(percent):
    """one user who clicked `percent` of the 50 items of [1, 51) -> (users, sets, (ptr, idx), allowed)"""
    clicked = set(np.random.RandomState(1).permutation(np.arange(1, NI_USER))[:percent * (NI_USER - 1) // 100].tolist())
    allowed = np.array(sorted(set(range(1, NI_USER)) - clicked))
    return np.zeros(ROWS, np.int64), {0: clicked}, E.csr({0: clicked}, 1), allowed


# ------------------------------------------------------------------------------------------------ the restatements are the oracle's
def test_vectorised_restatements_equal_the_oracle():
    users, _, (ptr, idx), n_items = population()
    for seed, epoch in ((1, 0), (3407, 3)):
        assert np.array_equal(E.sample_negatives_counter(users[:10000], n_items, ptr, idx, seed, epoch),
                              oracle.sample_negatives_counter(users[:10000], n_items, ptr, idx, seed, epoch))
    u, _, (ptr, idx), _ = one_user(80)                                  # long redraw chains
    assert np.array_equal(E.sample_negatives_counter(u[:5000], NI_USER, ptr, idx, 3407, 1),
                          oracle.sample_negatives_counter(u[:5000], NI_USER, ptr, idx, 3407, 1))
    ptr, idx = E.csr({0: set(range(57)) - {10, 11}, 1: set(range(57))}, 2)   # the walk, and a user with nothing left
    u = np.array([0] * 600 + [1] * 3)
    assert np.array_equal(E.sample_negatives_counter(u, 57, ptr, idx, 5, 0), oracle.sample_negatives_counter(u, 57, ptr, idx, 5, 0))
    for n in (1, 2, 3, 5, 17, 1000, 4097, 8192, 65536, 100003):
        for rounds in (2, 3, 4, 8):
            got = E.permutations(n, 3407, [0, 5, 2 ** 40 + 9], rounds)
            for k, epoch in enumerate((0, 5, 2 ** 40 + 9)):
                assert np.array_equal(got[k], oracle.epoch_permutation(n, 3407, epoch, rounds)), (n, rounds, epoch)


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize("arm", ARMS)
def test_population_item_histogram(arm):
    users, sets, (ptr, idx), n_items = population()
    neg = negatives(arm, users, n_items, ptr, idx, 1, 0)
    assert E.forbidden(neg, users, sets, n_items) == 0                  # never item 0, never a clicked pair
    inside("%s population item_chi2" % arm, E.item_chi2(neg, users, sets, n_items))


@pytest.mark.parametrize("percent", [20, 80, 0])
@pytest.mark.parametrize("arm", ARMS)
def test_one_user_is_uniform_over_the_allowed_items(arm, percent):
    users, sets, (ptr, idx), allowed = one_user(percent)
    a, b, c = (negatives(arm, users, NI_USER, ptr, idx, s, e) for s, e in ((3407, 0), (3407, 1), (3408, 0)))
    for neg in (a, b, c):
        assert E.forbidden(neg, users, sets, NI_USER) == 0
    tag = "%s user %d%% clicked" % (arm, percent)
    inside(tag + " user_chi2", E.user_chi2(a, allowed))
    inside(tag + " equal_rate epochs 0, 1", E.equal_rate(a, b, len(allowed)))
    inside(tag + " equal_rate seeds 3407, 3408", E.equal_rate(a, c, len(allowed)))


@pytest.mark.parametrize("arm", ARMS)
def test_two_items_leave_item_one(arm):
    ptr, idx = E.csr({1: {0}}, 2)
    users = np.arange(1000) % 2
    neg = negatives(arm, users, 2, ptr, idx, 3407, 0)
    assert (neg == 1).all() and E.forbidden(neg, users, {1: {0}}, 2) == 0
    assert E.item_chi2(neg, users, {1: {0}}, 2) == 0.0 and E.equal_rate(neg, neg, 1) == 0.0


@pytest.mark.parametrize("arm", ARMS)
def test_streams_are_pairwise_unrelated(arm):
    """20 (seed, epoch) streams, all 190 pairs: among them (s, e + 1) against (s + 1, e), which a key seed + epoch would alias"""
    ptr, idx = E.csr({}, 1)
    users = np.zeros(ROWS, np.int64)
    draws = [negatives(arm, users, 1000, ptr, idx, s, e) for s, e in STREAMS]
    zs = {}
    for i in range(len(STREAMS)):
        for j in range(i):
            zs[STREAMS[j], STREAMS[i]] = E.equal_rate(draws[j], draws[i], 999)
    assert len(zs) == 190 and ((0, 1), (1, 0)) in zs and ((3407, 1), (3408, 0)) in zs
    lo, hi = min(zs, key=zs.get), max(zs, key=zs.get)
    say("%s streams equal_rate min, pair %s" % (arm, lo), zs[lo])
    say("%s streams equal_rate max, pair %s" % (arm, hi), zs[hi])
    say("%s streams equal_rate (3407, 1) against (3408, 0)" % arm, zs[(3407, 1), (3408, 0)])
    bad = {k: v for k, v in zs.items() if abs(v) > BOUND}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the shuffle
@pytest.mark.parametrize("n", sorted(SHUFFLE_K))
@pytest.mark.parametrize("arm", ARMS)
def test_shuffle_is_a_uniform_order(arm, n):
    """n: 10, 13, 13, 16 and 17 bits (even and odd), 1000 / 4097 / 100003 with cycle walking, 8192 / 65536 without"""
    K = SHUFFLE_K[n]
    perms = orders(arm, n, 3407, K)
    assert np.array_equal(np.sort(perms, axis=1), np.broadcast_to(np.arange(n), (K, n)))
    tag = "%s shuffle n=%d K=%d" % (arm, n, K)
    inside(tag + " bucket_chi2 G=32", E.bucket_chi2(perms, 32))
    for name, fn in (("successor_count", E.successor_count), ("fixed_points", E.fixed_points),
                     ("same_as_previous", E.same_as_previous)):
        z, mean = fn(perms)
        inside("%s %s" % (tag, name), z, "mean %.4f" % mean)


@pytest.mark.parametrize("arm", ARMS)
def test_batches_are_uniform_samples_of_an_ordered_epoch(arm):
    """the reference's training rows are ordered by user: a batch must hold every block of them in proportion"""
    perms = orders(arm, 100003, 3407, 8)
    for e, perm in enumerate(perms):
        inside("%s batch_composition n=100003 B=2048 G=16 epoch %d" % (arm, e), E.batch_composition(perm, 2048, 16))


@pytest.mark.parametrize("n", [16, 17, 32, 33, 64])
@pytest.mark.parametrize("arm", ARMS)
def test_single_position_marginals(arm, n):
    inside("%s marginals n=%d, 20,000 epochs" % (arm, n), E.bucket_chi2(orders(arm, n, 3407, 20000), n))


# ------------------------------------------------------------------------------------------------ the two known deviations
def test_fallback_walk_is_pinned():
    """After 64 failed attempts draw_negative walks cyclically forward from the last draw.  With allowed items {10, 11} of
    [1, 57) every walk starts on a clicked item and meets 10 first, so item 10 gains the whole probability of reaching the
    walk, (54 / 56)^64 = 0.0975, over the uniform 1/2 of the redraws: 0.5488 against 0.4512.  Asserted, so that a change of
    rule is noticed."""
    sets = {0: set(range(57)) - {10, 11}}
    ptr, idx = E.csr(sets, 1)
    users = np.zeros(ROWS, np.int64)
    neg = E.sample_negatives_counter(users, 57, ptr, idx, 5, 0)
    assert E.forbidden(neg, users, sets, 57) == 0 and set(np.unique(neg).tolist()) == {10, 11}
    reach = (54.0 / 56.0) ** 64
    p = 0.5 + reach / 2.0
    share = float((neg == 10).mean())
    inside("fallback share of item 10", (share - p) / math.sqrt(p * (1.0 - p) / ROWS), "share %.5f expects %.5f" % (share, p))
    assert abs(share - 0.5) / math.sqrt(0.25 / ROWS) > 2 * BOUND          # and it is not the uniform law
    # the reference's own rule at the same case: uniform
    ref = oracle.sample_negatives(users[:20000], 57, ptr, idx, rng=np.random.RandomState(5))
    inside("numpy fallback case user_chi2 (20,000 rows)", E.user_chi2(ref, [10, 11]))


def test_small_n_marginals_are_printed():
    """Below n = 16 the single-position marginals of the 8-round network are measurably not uniform (cell probabilities off by
    up to 6 %): known, documented (wr_shuffle.h), not asserted: no epoch has fewer than 16 rows.  The control
    arm at the same sizes is asserted."""
    for n in (5, 6, 9):
        for seed in (3407, 11):
            say("restated marginals n=%d seed %d, 20,000 epochs (known deviation)" % (n, seed),
                E.bucket_chi2(orders("restated", n, seed, 20000), n))
        inside("numpy marginals n=%d, 20,000 epochs" % n, E.bucket_chi2(orders("numpy", n, 3407, 20000), n))


# ------------------------------------------------------------------------------------------------ power
@pytest.mark.parametrize("wrong", E.WRONG)
def test_wrong_samplers_are_caught(wrong):
    """the user with 20 % clicked; each wrong rule must leave the bound behind by a factor of two on some statistic"""
    users, sets, (ptr, idx), allowed = one_user(20)
    a, b = (E.sample_negatives_counter(users, NI_USER, ptr, idx, 3407, e, wrong) for e in (0, 1))
    zs = {"user_chi2": E.user_chi2(a, allowed), "equal_rate epochs 0, 1": E.equal_rate(a, b, len(allowed))}
    for name, z in zs.items():
        say("WRONG %s %s" % (wrong, name), z, "forbidden draws %d" % E.forbidden(a, users, sets, NI_USER))
    assert max(abs(z) for z in zs.values()) > 2 * BOUND


@pytest.mark.parametrize("rounds", [2, 3, 4])
def test_fewer_feistel_rounds_are_caught(rounds):
    perms = np.stack([oracle.epoch_permutation(1000, 3407, e, rounds=rounds) for e in range(SHUFFLE_K[1000])])
    z, mean = E.successor_count(perms)
    say("WRONG rounds=%d successor_count n=1000 K=2000" % rounds, z, "mean %.4f" % mean)
    say("WRONG rounds=%d bucket_chi2 G=32" % rounds, E.bucket_chi2(perms, 32))
    assert z > 2 * BOUND


def test_six_rounds_are_not_separable():
    """printed for the record: at sizes that fit this file's time 6 rounds pass every statistic"""
    perms = E.permutations(1000, 3407, np.arange(SHUFFLE_K[1000]), rounds=6)
    for name, fn in (("successor_count", E.successor_count), ("fixed_points", E.fixed_points)):
        say("rounds=6 %s n=1000 K=2000 (not asserted)" % name, fn(perms)[0])
    say("rounds=6 bucket_chi2 G=32 (not asserted)", E.bucket_chi2(perms, 32))
