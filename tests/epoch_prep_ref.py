"""Distribution battery for the device epoch preparation (wr_sampler.hip, wr_shuffle.h): plain NumPy, float64, no GPU.

Three parts.  (1) The two generators restated over whole arrays (`sample_negatives_counter`, `permutations`): the same bits
as oracle.sample_negatives_counter / oracle.epoch_permutation (tests/test_epoch_prep_contract.py holds them equal), fast
enough for 200,000 rows and thousands of epochs.  (2) `wrong=`: deliberately wrong samplers for the power tests (the wrong
shuffles are oracle.epoch_permutation's own `rounds=`).  (3) The statistics.  Each returns a z-score, (chi2 - dof) /
sqrt(2 dof) or (x - mean) / sd, under the law the reference's rule implies (src/models/BaseModel.py:167-177: uniform over the
items of [1, n_items) the user has not clicked; src/helpers/BaseRunner.py:188-193: a uniform random order), so one bound
serves all of them."""
import math

import numpy as np

GOLD = np.uint64(0x9E3779B97F4A7C15)
ROW_MUL = np.uint64(0xD1B54A32D192ED03)
SHUFFLE_DOMAIN = np.uint64(0x5DEECE66D)
MAX_ATTEMPTS = 64
BOUND = 4.9                     # sigma per statistic (two-sided 1e-6), as in tests/test_contrarec_aug_contract.py
WRONG = ("collision_next", "last_item_missing", "zero_included", "epoch_ignored", "attempt_ignored")
_U = np.uint64


def mix64(x):
    """splitmix64 finaliser (wr_common.h)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
        return x ^ (x >> _U(31))


def csr(sets, n_users):
    """{user: set of items} -> (ptr int64 [n_users + 1], idx int32, ascending per user; one element at least)"""
    ptr = np.zeros(n_users + 1, np.int64)
    chunks = []
    for u in range(n_users):
        it = sorted(sets.get(u, ()))
        ptr[u + 1] = ptr[u] + len(it)
        chunks.append(np.asarray(it, np.int32))
    idx = np.concatenate(chunks) if chunks else np.zeros(0, np.int32)
    return ptr, (idx if len(idx) else np.zeros(1, np.int32))


def _pair_keys(ptr, idx, n_items):
    """the (user, item) pairs of the lists as ascending keys user * n_items + item"""
    ptr = np.asarray(ptr, np.int64)
    n_users = len(ptr) - 1
    owner = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(ptr))
    keys = np.sort(owner * n_items + np.asarray(idx, np.int64)[:ptr[-1]])
    return keys, keys // n_items


def _member(keys, q):
    if len(keys) == 0:
        return np.zeros(len(q), bool)
    pos = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    return keys[pos] == q


# ------------------------------------------------------------------------------------------------ the sampler, restated
def draw_item(seed, epoch, rows, attempt, n_items, wrong=None):
    """draw_item of wr_sampler.hip for an array of rows -> int64 items"""
    with np.errstate(over="ignore"):
        a = mix64(_U(seed)) if wrong == "epoch_ignored" else mix64(_U(seed) ^ (_U(epoch) * GOLD))
        b = mix64(np.asarray(rows, dtype=np.uint64) * ROW_MUL + _U(0 if wrong == "attempt_ignored" else attempt))
        hi = mix64(a ^ b) >> _U(32)
        if wrong == "last_item_missing":
            return (_U(1) + ((hi * _U(n_items - 2)) >> _U(32))).astype(np.int64)
        if wrong == "zero_included":
            return ((hi * _U(n_items - 1)) >> _U(32)).astype(np.int64)
        return (_U(1) + ((hi * _U(n_items - 1)) >> _U(32))).astype(np.int64)


def sample_negatives_counter(user_ids, n_items, clicked_ptr, clicked_idx, seed, epoch, wrong=None):
    """draw_negative of wr_sampler.hip over all rows at once; wrong=None gives oracle.sample_negatives_counter's bits"""
    assert wrong is None or wrong in WRONG
    users = np.asarray(user_ids, dtype=np.int64)
    keys, _ = _pair_keys(clicked_ptr, clicked_idx, n_items)
    cand = draw_item(seed, epoch, np.arange(len(users)), 0, n_items, wrong)
    pend = np.flatnonzero(_member(keys, users * n_items + cand))
    if wrong == "collision_next":
        cand[pend] += 1
        return cand
    attempt = 0
    while len(pend):
        attempt += 1
        if attempt < MAX_ATTEMPTS:
            cand[pend] = draw_item(seed, epoch, pend, attempt, n_items, wrong)
        else:                                               # the cyclic walk from the last draw
            c = cand[pend]
            cand[pend] = np.where(c + 1 >= n_items, 1, c + 1)
            if attempt >= MAX_ATTEMPTS + n_items:
                break
        pend = pend[_member(keys, users[pend] * n_items + cand[pend])]
    return cand


# ------------------------------------------------------------------------------------------------ the shuffle, restated
def permutations(n, seed, epochs, rounds=8):
    """shuffle_index of wr_shuffle.h for every row of every epoch asked for -> int32 [len(epochs), n]; row e equals
    oracle.epoch_permutation(n, seed, epochs[e], rounds)"""
    n = int(n)
    assert 0 < n < (1 << 31)
    epochs = np.asarray(epochs, dtype=np.uint64)
    bits = 2
    while (1 << bits) < n:
        bits += 1
    a = bits >> 1
    b = bits - a
    mask_a, mask_b = _U((1 << a) - 1), _U((1 << b) - 1)
    out = np.empty((len(epochs), n), np.int32)
    step = max(1, (1 << 21) // n)
    with np.errstate(over="ignore"):
        keys = mix64(mix64(_U(seed) ^ (epochs * GOLD)) ^ SHUFFLE_DOMAIN)
        for s in range(0, len(epochs), step):
            key = np.repeat(keys[s:s + step], n)
            x = np.tile(np.arange(n, dtype=np.uint64), len(keys[s:s + step]))
            todo = np.arange(len(x))
            while len(todo):
                v, k = x[todo], key[todo]
                hi, lo = v >> _U(b), v & mask_b
                for r in range(rounds):
                    if r % 2 == 0:
                        hi = hi ^ (mix64(k ^ (lo * ROW_MUL + _U(r))) & mask_a)
                    else:
                        lo = lo ^ (mix64(k ^ (hi * ROW_MUL + _U(r))) & mask_b)
                v = (hi << _U(b)) | lo
                x[todo] = v
                todo = todo[v >= _U(n)]
            out[s:s + step] = x.reshape(-1, n)
    return out


# ------------------------------------------------------------------------------------------------ statistics
def _z(chi2, dof):
    return (chi2 - dof) / math.sqrt(2.0 * dof) if dof > 0 else 0.0


def forbidden(neg, users, sets, n_items):
    """the number of rows whose negative is outside [1, n_items) or in the user's list: 0 under the reference's rule"""
    neg, users = np.asarray(neg, np.int64), np.asarray(users, np.int64)
    n_users = int(max(users.max(), max(sets) if sets else 0)) + 1
    ptr, idx = csr(sets, n_users)
    keys, _ = _pair_keys(ptr, idx, n_items)
    bad = (neg < 1) | (neg >= n_items)
    return int((bad | _member(keys, users * n_items + neg)).sum())


def item_chi2(neg, users, sets, n_items):
    """The item histogram of all rows against its expectation under the rule: item j expects the sum, over the rows whose user
    has not clicked j, of 1 / |allowed(user)|, allowed(u) = [1, n_items) minus u's list.  Needs no second generator.  Counts
    the draws in [1, n_items) only (forbidden() counts the others)."""
    neg, users = np.asarray(neg, np.int64), np.asarray(users, np.int64)
    n_users = int(max(users.max(), max(sets) if sets else 0)) + 1
    ptr, idx = csr(sets, n_users)
    keys, owner = _pair_keys(ptr, idx, n_items)
    item_of = keys - owner * n_items                                   # owner is ascending, as the keys are
    drawable = item_of >= 1
    rows_of = np.bincount(users, minlength=n_users).astype(np.float64)
    n_allowed = (n_items - 1) - np.bincount(owner[drawable], minlength=n_users)
    assert (n_allowed[rows_of > 0] > 0).all(), "a user with rows and no allowed item"
    w = np.where(rows_of > 0, rows_of / np.maximum(n_allowed, 1), 0.0)
    expected = np.full(n_items, w.sum()) - np.bincount(item_of, weights=w[owner], minlength=n_items)
    expected[0] = 0.0
    assert abs(expected.sum() - len(neg)) <= 1e-6 * len(neg)
    observed = np.bincount(neg[(neg >= 1) & (neg < n_items)], minlength=n_items).astype(np.float64)
    live = expected > 0
    return _z(float(((observed[live] - expected[live]) ** 2 / expected[live]).sum()), int(live.sum()) - 1)


def user_chi2(neg, allowed):
    """one user's rows against the uniform law on that user's allowed items (draws outside them show as a deficit)"""
    neg, allowed = np.asarray(neg, np.int64), np.sort(np.asarray(allowed, np.int64))
    pos = np.minimum(np.searchsorted(allowed, neg), len(allowed) - 1)
    observed = np.bincount(pos[allowed[pos] == neg], minlength=len(allowed)).astype(np.float64)
    expected = len(neg) / len(allowed)
    return _z(float(((observed - expected) ** 2 / expected).sum()), len(allowed) - 1)


def equal_rate(a, b, n_allowed):
    """the share of rows where two streams drew the same item, against 1 / n_allowed (both uniform on the same n_allowed
    items and independent)"""
    a, b = np.asarray(a), np.asarray(b)
    p = 1.0 / n_allowed
    if p >= 1.0:
        return 0.0 if (a == b).all() else math.inf
    return float(((a == b).mean() - p) / math.sqrt(p * (1.0 - p) / len(a)))


def _fixed_margin_chi2(table, rows, cols, n, K):
    """Pearson's statistic of a table whose two margins are fixed (K permutations of n rows, summed): n / (n - 1) times a
    chi-square on (R - 1)(C - 1) degrees of freedom, the factor being that of drawing without replacement"""
    expected = K * np.outer(rows, cols) / float(n)
    chi2 = float(((table - expected) ** 2 / expected).sum()) * (n - 1.0) / n
    return _z(chi2, (len(rows) - 1) * (len(cols) - 1))


def bucket_chi2(perms, G):
    """the G x G table of position bucket against source bucket (bucket of i: i * G // n) over a list of permutations"""
    perms = np.asarray(perms)
    K, n = perms.shape
    pos = np.arange(n, dtype=np.int64) * G // n
    table = np.zeros(G * G)
    for p in perms:
        table += np.bincount(pos * G + p.astype(np.int64) * G // n, minlength=G * G)
    size = np.bincount(pos, minlength=G).astype(np.float64)
    return _fixed_margin_chi2(table.reshape(G, G), size, size, n, K)


def batch_composition(perm, B, G):
    """the counts of source block g (block of j: j * G // n) in each batch of B consecutive output rows, the short last batch
    included, against the batch's size times the block's share of the rows: batches are uniform samples of an ordered epoch"""
    perm = np.asarray(perm, np.int64)
    n = len(perm)
    batch = np.arange(n, dtype=np.int64) // B
    nb = int(batch[-1]) + 1
    table = np.bincount(batch * G + perm * G // n, minlength=nb * G).reshape(nb, G).astype(np.float64)
    return _fixed_margin_chi2(table, np.bincount(batch, minlength=nb).astype(np.float64),
                              np.bincount(np.arange(n, dtype=np.int64) * G // n, minlength=G).astype(np.float64), n, 1)


def successor_count(perms):
    """the mean number of i with perm(i + 1) == perm(i) + 1 over K permutations, against (n - 1) / n (that is 1 to within
    1 / n) with sd 1 / sqrt(K) -> (z, mean)"""
    perms = np.asarray(perms)
    K, n = perms.shape
    mean = float((perms[:, 1:] == perms[:, :-1] + 1).sum(axis=1).mean())
    return (mean - (n - 1.0) / n) * math.sqrt(K), mean


def fixed_points(perms):
    """the mean number of i with perm(i) == i, against 1 with sd 1 / sqrt(K) -> (z, mean)"""
    perms = np.asarray(perms)
    K, n = perms.shape
    mean = float((perms == np.arange(n, dtype=perms.dtype)[None, :]).sum(axis=1).mean())
    return (mean - 1.0) * math.sqrt(K), mean


def same_as_previous(perms):
    """the mean number of i with perm_e(i) == perm_{e+1}(i) over consecutive permutations, against 1 with sd 1 / sqrt(K - 1):
    consecutive epochs are unrelated -> (z, mean)"""
    perms = np.asarray(perms)
    mean = float((perms[1:] == perms[:-1]).sum(axis=1).mean())
    return (mean - 1.0) * math.sqrt(len(perms) - 1), mean
