"""Device negative sampler (wr_sample_negatives) vs its NumPy restatement in the oracle: bit-exact indices, the
reference's rule (range [1, n_items), never an item of the user's train set — src/models/BaseModel.py:167-177), and
reproducibility.  The restatement is the project's own generator, so equality alone would pass a biased rule on both sides:
the device's own output also faces the distribution battery of tests/epoch_prep_ref.py (uniform over the allowed items, a
uniform order; |z| <= 4.9 per statistic, calibrated in tests/test_epoch_prep_contract.py).  Run with -rP for every z."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epoch_prep_ref as E  # noqa: E402

pytestmark = pytest.mark.gpu


def _inside(name, z, extra=""):
    print("z %-72s %+8.2f %s" % (name, z, extra))
    assert abs(z) <= E.BOUND, "%s: z = %.2f outside %.1f sigma" % (name, z, E.BOUND)


def _csr(sets, nU):
    ptr = np.zeros(nU + 1, np.int64); chunks = []
    for u in range(nU):
        it = sorted(sets.get(u, ()))
        ptr[u + 1] = ptr[u] + len(it)
        chunks.append(np.asarray(it, np.int32))
    idx = np.concatenate(chunks) if chunks else np.zeros(0, np.int32)
    return ptr, (idx if len(idx) else np.zeros(1, np.int32))


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_matches_oracle_bit_exact(g3, dtype):
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    nI = int(g3["n_items"][0])
    ptr = g3["clicked_ptr"].astype(np.int64); idx = g3["clicked_idx"].astype(np.int32)
    users = g3["users"]
    nU = len(ptr) - 1
    for epoch in (0, 1, 7):
        neg, err = hip_ops.sample_negatives(torch.from_numpy(users).to(dev).to(dtype), nU, nI, torch.from_numpy(ptr).to(dev),
                                            torch.from_numpy(idx).to(dev), 3407, epoch)
        ref = oracle.sample_negatives_counter(users, nI, ptr, idx, 3407, epoch)
        got = neg.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, ref)                      # indices bit-exact
        assert int(err.item()) == 0
        assert got.min() >= 1 and got.max() < nI              # item 0 is never a negative (BaseModel.py:168)
        for uu, nn in zip(users, got):
            assert nn not in idx[ptr[uu]:ptr[uu + 1]]         # user 3 clicked 55 of 57 items: long redraw chains
    a, _ = hip_ops.sample_negatives(torch.from_numpy(users).to(dev), nU, nI, torch.from_numpy(ptr).to(dev),
                                    torch.from_numpy(idx).to(dev), 3407, 0)
    b, _ = hip_ops.sample_negatives(torch.from_numpy(users).to(dev), nU, nI, torch.from_numpy(ptr).to(dev),
                                    torch.from_numpy(idx).to(dev), 3408, 0)
    assert not torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def _large_case():
    """2,000 users with 1 to 60 clicked of 5,000 items, 1 M rows; the restatement of the first 200,000, computed once"""
    rng = np.random.RandomState(0)
    nU, nI, n = 2000, 5000, 1_000_000
    sets = {u: set(rng.randint(0, nI, rng.randint(1, 60)).tolist()) for u in range(nU)}
    ptr, idx = _csr(sets, nU)
    users = rng.randint(0, nU, n)
    ref = oracle.sample_negatives_counter(users[:200_000], nI, ptr, idx, 1, 0)
    ref.setflags(write=False)
    return nU, nI, n, sets, ptr, idx, users, ref


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("form", ["lists", "pairs"])
def test_large_uniformity_and_exclusion(form, dtype):
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    nU, nI, n, sets, ptr, idx, users, ref = _large_case()
    tptr, tidx = torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)
    tu = torch.from_numpy(users).to(dev).to(dtype)
    if form == "pairs":
        neg, err = hip_ops.sample_negatives(tu, nU, nI, None, None, 1, 0, pairs=hip_ops.pair_set(tptr, tidx, nU))
    else:
        neg, err = hip_ops.sample_negatives(tu, nU, nI, tptr, tidx, 1, 0)
    assert neg.dtype == dtype
    got = neg.cpu().numpy().astype(np.int64)
    assert int(err.item()) == 0 and got.min() >= 1 and got.max() < nI
    # exclusion, vectorised: (user, item) pairs of the train set never appear
    train_keys = np.concatenate([np.full(ptr[u + 1] - ptr[u], u, np.int64) * nI + idx[ptr[u]:ptr[u + 1]] for u in range(nU)])
    assert not np.isin(users.astype(np.int64) * nI + got, train_keys).any()
    assert E.forbidden(got, users, sets, nI) == 0
    counts = np.bincount(got, minlength=nI)[1:]
    assert abs(counts.mean() - n / (nI - 1)) < 1e-6 and counts.std() / counts.mean() < 0.15   # flat histogram
    # ... and against its expectation under the rule (each row uniform over its user's allowed items), which needs no oracle
    # run: the Poisson noise of this case alone is a std / mean of 0.0707
    _inside("device %s %s 1 M rows item_chi2" % (form, str(dtype)[6:]), E.item_chi2(got, users, sets, nI),
            "std / mean %.4f" % (counts.std() / counts.mean()))
    assert np.array_equal(got[:len(ref)], ref)


@pytest.mark.parametrize("percent", [20, 80, 0])
def test_one_user_is_uniform_over_the_allowed_items(percent):
    """200,000 rows of one user who clicked 20 % / 80 % / none of 50 items: uniform over the allowed ones, and unrelated between
    epochs and between seeds (the share of equal draws is 1 / |allowed|)"""
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    nI, n = 51, 200_000
    clicked = set(np.random.RandomState(1).permutation(np.arange(1, nI))[:percent * (nI - 1) // 100].tolist())
    allowed = np.array(sorted(set(range(1, nI)) - clicked))
    ptr, idx = _csr({0: clicked}, 1)
    users = np.zeros(n, np.int64)
    tu, tptr, tidx = torch.from_numpy(users).to(dev), torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)
    draws = []
    for seed, epoch in ((3407, 0), (3407, 1), (3408, 0)):
        neg, err = hip_ops.sample_negatives(tu, 1, nI, tptr, tidx, seed, epoch)
        got = neg.cpu().numpy()
        assert int(err.item()) == 0 and E.forbidden(got, users, {0: clicked}, nI) == 0
        assert np.array_equal(got, E.sample_negatives_counter(users, nI, ptr, idx, seed, epoch))
        draws.append(got)
    tag = "device user %d%% clicked" % percent
    _inside(tag + " user_chi2", E.user_chi2(draws[0], allowed))
    _inside(tag + " equal_rate epochs 0, 1", E.equal_rate(draws[0], draws[1], len(allowed)))
    _inside(tag + " equal_rate seeds 3407, 3408", E.equal_rate(draws[0], draws[2], len(allowed)))


def test_user_who_clicked_everything_is_flagged():
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    nI = 20
    sets = {0: set(range(nI)), 1: {3}}
    ptr, idx = _csr(sets, 2)
    neg, err = hip_ops.sample_negatives(torch.tensor([0, 1, 1], device=dev), 2, nI, torch.from_numpy(ptr).to(dev),
                                        torch.from_numpy(idx).to(dev), 5, 0)
    assert int(err.item()) == 2
    assert neg[1].item() != 3 and neg[2].item() != 3


# ----------------------------------------------------------------------------------------------- epoch shuffle
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
# 512 / 8192 / 131072: exact powers of two on an odd number of bits; 513 / 8193 / 131073: 2^k + 1 on an even number, the longest
# cycle walks (the domain is almost 2 n)
@pytest.mark.parametrize("n", [1, 2, 3, 17, 511, 512, 513, 1000, 4097, 8191, 8192, 8193, 65536, 100003, 131071, 131072, 131073])
def test_epoch_shuffle_matches_oracle_bit_exact(dtype, n):
    """wr_epoch_shuffle: out_k[i] = col_k[perm(i)] with perm = oracle.epoch_permutation, a bijection of [0, n) — the
    device's epoch order (reference: DataLoader(shuffle=True), BaseRunner.py:188-193)."""
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(n)
    cols = [rng.randint(0, 1 << 30, n) for _ in range(3)]
    perm = oracle.epoch_permutation(n, 3407, 5)
    assert np.array_equal(np.sort(perm), np.arange(n))
    outs, order = hip_ops.epoch_shuffle([torch.from_numpy(c).to(dtype).to(dev) for c in cols], 3407, 5, want_order=True)
    assert np.array_equal(order.cpu().numpy(), perm)
    for c, o in zip(cols, outs):
        assert o.dtype == dtype and np.array_equal(o.cpu().numpy(), c[perm])
    # fewer columns, no order; another epoch gives another order; the same call twice the same one
    (o0,) = hip_ops.epoch_shuffle([torch.from_numpy(cols[0]).to(dtype).to(dev)], 3407, 5)
    assert torch.equal(o0, outs[0])
    if n >= 1000:
        (o1,) = hip_ops.epoch_shuffle([torch.from_numpy(cols[0]).to(dtype).to(dev)], 3407, 6)
        assert not torch.equal(o1, o0)


def test_epoch_shuffle_order_is_uniform():
    """The device's own orders of 64 epochs at n = 100003 under the battery for the order: position bucket against source
    bucket, neighbours kept together, epochs repeating each other, and batches of 2,048 rows as uniform samples of an epoch
    whose rows are ordered (the reference's are, by user)."""
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    n, K = 100003, 64
    col = torch.arange(n, dtype=torch.int32, device=dev)
    perms = np.empty((K, n), np.int64)
    for e in range(K):
        (out,), order = hip_ops.epoch_shuffle([col], 3407, e, want_order=True)
        perms[e] = order.cpu().numpy()
        assert torch.equal(out.long(), order)
    assert np.array_equal(np.sort(perms, axis=1), np.broadcast_to(np.arange(n), (K, n)))
    assert np.array_equal(perms, E.permutations(n, 3407, np.arange(K)))
    tag = "device shuffle n=%d K=%d" % (n, K)
    _inside(tag + " bucket_chi2 G=64", E.bucket_chi2(perms, 64))
    for name, fn in (("successor_count", E.successor_count), ("same_as_previous", E.same_as_previous)):
        z, mean = fn(perms)
        _inside("%s %s" % (tag, name), z, "mean %.4f" % mean)
    for e in range(8):
        _inside("%s batch_composition B=2048 G=16 epoch %d" % (tag, e), E.batch_composition(perms[e], 2048, 16))


def test_epoch_shuffle_full_size_is_a_permutation():
    """C2 scale (100 M rows, BASELINE.json configs[1]): the order is a bijection (every row exactly once) and the three
    columns travel together; sampled positions equal the oracle's permutation."""
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    n = 100_000_000
    base = torch.arange(n, dtype=torch.int32, device=dev)
    outs, order = hip_ops.epoch_shuffle([base, base + 1, base * 2 % 1000003], 11, 3, want_order=True)
    assert int(order.min()) == 0 and int(order.max()) == n - 1
    seen = torch.zeros(n, dtype=torch.uint8, device=dev)
    seen[order] = 1
    assert int(seen.sum(dtype=torch.int64)) == n
    assert torch.equal(outs[0].long(), order) and torch.equal(outs[1].long(), order + 1)
    assert torch.equal(outs[2].long(), order * 2 % 1000003)
    # the network is evaluated per row: the oracle restates a sample of positions
    probe = np.array([0, 1, 2, 12345, 65536, n // 2, n - 2, n - 1])
    got = order.cpu().numpy()[probe]
    ref = oracle.epoch_permutation_at(probe, n, 11, 3)
    assert np.array_equal(got, ref)


def test_epoch_shuffle_rejects_bad_arguments():
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    a = torch.arange(10, device=dev)
    with pytest.raises(ValueError):
        hip_ops.epoch_shuffle([a, a[:5]], 1, 1)
    with pytest.raises(TypeError):
        hip_ops.epoch_shuffle([a.float()], 1, 1)
    with pytest.raises(ValueError):
        hip_ops.epoch_shuffle([], 1, 1)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_fused_range_preparation_equals_sampler_then_shuffle(dtype):
    """wr_epoch_prepare_range (shuffle + negatives fused, any range of output rows) = wr_sample_negatives followed by
    wr_epoch_shuffle, bit for bit, and — through the oracle restatements of both — the reference's rule
    (src/models/BaseModel.py:167-177, src/helpers/BaseRunner.py:188-193)"""
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(3)
    nU, nI, n = 300, 97, 20011
    users = rng.randint(0, nU, n)
    items = rng.randint(0, nI, n)
    sets = {}
    for a, b in zip(users, items):
        sets.setdefault(int(a), set()).add(int(b))
    sets[5] = set(range(1, nI - 2))                                  # a user who clicked almost everything: long redraw chains
    ptr, idx = _csr(sets, nU)
    tu, ti = torch.from_numpy(users).to(dev).to(dtype), torch.from_numpy(items).to(dev).to(dtype)
    tptr, tidx = torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)
    for epoch in (0, 3):
        neg, _ = hip_ops.sample_negatives(tu, nU, nI, tptr, tidx, 3407, epoch)
        (su, si, sn), order = hip_ops.epoch_shuffle([tu, ti, neg], 3407, epoch, want_order=True)
        prep = hip_ops.EpochPrep(tu, ti, nU, nI, tptr, tidx, 3407, epoch, want_order=True)
        for lo, hi in ((7000, 20011), (0, 1), (1, 7000)):           # ranges in any order, any cut
            prep.fill(lo, hi)
        # membership through the hash set of the pairs (wr_pairset_build) instead of the lists: the same columns
        pairs = hip_ops.pair_set(tptr, tidx, nU)
        neg_set, _ = hip_ops.sample_negatives(tu, nU, nI, None, None, 3407, epoch, pairs=pairs)
        prep_set = hip_ops.EpochPrep(tu, ti, nU, nI, None, None, 3407, epoch, want_order=True, pairs=pairs)
        prep_set.fill(0, n)
        # ... and with the source rows packed into one word each (wr_epoch_prepare_range_packed): the same columns again
        prep_pk = hip_ops.EpochPrep(tu, ti, nU, nI, None, None, 3407, epoch, want_order=True, pairs=pairs,
                                    packed=hip_ops.pack_rows(tu, ti))
        for lo, hi in ((100, n), (0, 100)):
            prep_pk.fill(lo, hi)
        torch.cuda.synchronize()
        assert torch.equal(neg_set, neg)
        assert all(torch.equal(a, b) for a, b in zip(prep_set.cols, prep.cols)) and torch.equal(prep_set.order, prep.order)
        assert prep_pk.packed is not None
        assert all(torch.equal(a, b) for a, b in zip(prep_pk.cols, prep.cols)) and torch.equal(prep_pk.order, prep.order)
        assert torch.equal(prep.cols[0], su) and torch.equal(prep.cols[1], si) and torch.equal(prep.cols[2], sn)
        assert torch.equal(prep.order, order)
        prep.check()
        ref_neg = oracle.sample_negatives_counter(users, nI, ptr, idx, 3407, epoch)
        perm = oracle.epoch_permutation(n, 3407, epoch)
        assert np.array_equal(prep.cols[2].cpu().numpy().astype(np.int64), ref_neg[perm])
        assert np.array_equal(prep.cols[0].cpu().numpy().astype(np.int64), users[perm])
    bad = tu.clone(); bad[17] = nU
    p2 = hip_ops.EpochPrep(bad, ti, nU, nI, tptr, tidx, 1, 0)
    p2.fill(0, n)
    with pytest.raises(IndexError):
        p2.check()


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_fused_preparation_draws_from_the_rule(dtype):
    """EpochPrep.fill end to end, packed source rows and the pair set, filled in two ranges: the negatives column against its
    expectation under the rule given the SHUFFLED users column beside it (not through equality with the other two kernels),
    on a frame ordered by user as the reference's is"""
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(7)
    nU, nI, n = 2000, 5000, 200_003
    sets = {u: set(rng.randint(0, nI, rng.randint(1, 60)).tolist()) for u in range(nU)}
    ptr, idx = _csr(sets, nU)
    users = np.sort(rng.randint(0, nU, n))
    items = idx[ptr[users] + rng.randint(0, 1 << 30, n) % (ptr[users + 1] - ptr[users])].astype(np.int64)   # a clicked item each
    tu, ti = torch.from_numpy(users).to(dev).to(dtype), torch.from_numpy(items).to(dev).to(dtype)
    tptr, tidx = torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)
    prep = hip_ops.EpochPrep(tu, ti, nU, nI, None, None, 3407, 2, want_order=True, pairs=hip_ops.pair_set(tptr, tidx, nU),
                             packed=hip_ops.pack_rows(tu, ti))
    assert prep.packed is not None
    for lo, hi in ((65536, n), (0, 65536)):
        prep.fill(lo, hi)
    torch.cuda.synchronize()
    prep.check()
    assert int(prep.err.item()) == 0
    su, si, sn = (c.cpu().numpy().astype(np.int64) for c in prep.cols)
    order = prep.order.cpu().numpy()
    assert np.array_equal(np.sort(order), np.arange(n))
    assert np.array_equal(su, users[order]) and np.array_equal(si, items[order])
    assert E.forbidden(sn, su, sets, nI) == 0
    _inside("device EpochPrep packed %s item_chi2" % str(dtype)[6:], E.item_chi2(sn, su, sets, nI))
    _inside("device EpochPrep packed %s batch_composition B=2048 G=16" % str(dtype)[6:], E.batch_composition(order, 2048, 16))


def test_pipelined_preparation_trains_the_same_epoch():
    """PipelinedSgd with an EpochPrep (rows of plan chunk c+1 produced beside the steps of chunk c) = the same epoch with the
    columns prepared up front: tables and losses bitwise equal"""
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(4)
    nU, nI, D, B, nb = 5000, 4000, 64, 2048, 13
    n = nb * B - 77
    users = rng.randint(0, nU, n).astype(np.int32); items = rng.randint(0, nI, n).astype(np.int32)
    ptr, idx = hip_ops.clicked_csr_from_pairs(torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev), nU, nI)
    U = (rng.standard_normal((nU, D)) * 0.1).astype(np.float32); I = (rng.standard_normal((nI, D)) * 0.1).astype(np.float32)
    tu, ti = torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev)
    outs = []
    for pipelined in (False, True):
        Ud, Id = torch.from_numpy(U).to(dev), torch.from_numpy(I).to(dev)
        prep = hip_ops.EpochPrep(tu, ti, nU, nI, ptr, idx, 11, 2)
        if not pipelined:
            prep.fill(0, n)
        pipe = hip_ops.PipelinedSgd(chunk=3, min_triplets=1)
        h = pipe.plan(Ud, [(Id, prep.cols[0], prep.cols[1], prep.cols[2])], B, prep=prep if pipelined else None)
        losses = torch.empty(nb, dtype=torch.float32, device=dev)
        pipe.run(h, 0, 0.05, losses)
        torch.cuda.synchronize()
        prep.check()
        assert prep.filled == n
        outs.append((Ud, Id, losses))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
