"""Exact-arithmetic reference for the ranking kernels (wr_rank_eval, wr_rank_eval_rows, wr_rank_eval_multi): NumPy only.

The rule.  rank = 1 + the number of items that are not masked for the row and whose score is STRICTLY above the target's.
The target's own column never counts, masked or not.  A row whose target score is NaN ranks behind everything:
rank = n_items + 1, whatever its mask.  A NaN score of another item never counts, a +inf target ranks 1, a -inf target ranks
1 + the number of unmasked items above -inf.

The tables.  grid_tables() draws multiples of 1/8 in [-1, 1]: a product is a multiple of 1/64 and a sum of D of them is at
most D in size, so every fp32 fmaf chain, in any order, is exact up to D = 252 (252 * 64 < 2^24), and the float64 score
IS the kernel's score.  No row has to be skipped and exact ties are frequent.

The cases (CASES: name -> constructor, case(name) builds and caches) are dicts of arrays:
    family, name, entry   "rank_eval" | "rank_eval_rows" | "rank_eval_multi": the entry the case is run through
    Q [rows, D], I [n_items, D] float32, target int64 [n], KQ
    query_row             int64 [n] or None (row e scores with Q[e]); with KQ > 1 row e owns Q[e KQ .. e KQ + KQ - 1]
    mask_row, ptr, idx    int64 [n], CSR int64 / int32 of the mask lists (ascending), or None x 3
    eval_user             entry "rank_eval" only: query_row = mask_row = eval_user
rank_wrong(case, variant) restates the kernel with one plausible defect; tests/test_rank_contract.py shows that every defect
moves a rank in some case, so a kernel that had it could not pass tests/test_hip_rank_exact.py.
"""
import functools

import numpy as np

CHUNK = 2048                      # kEvalChunk
F32_OVERFLOW = 2.0 ** 128 - 2.0 ** 103   # what rounds to +-inf in fp32 (round to nearest even)
REGA_D = (8, 16, 32, 64)          # register-operand scan, item tiles of 64; any other D: LDS-operand scan, tiles of 32
LDS_D = (4, 24, 128, 252)


def tile_of(D):
    return 64 if D in REGA_D else 32


def grid_tables(D, n_rows, n_items, seed):
    """multiples of 1/8 in [-1, 1] (tests/test_hip_topk.py, _tables(grid=True))"""
    rng = np.random.RandomState(seed)
    Q = rng.randint(-8, 9, (n_rows, D)) / 8.0
    I = rng.randint(-8, 9, (n_items, D)) / 8.0
    return Q.astype(np.float32), I.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ reference
def row_queries(c):
    """float32 [n KQ, D]: the query rows of every evaluation row, in order"""
    if c["KQ"] > 1 or c["query_row"] is None:
        return c["Q"][:len(c["target"]) * c["KQ"]]
    return c["Q"][c["query_row"]]


def scores64(Qr, I, KQ=1, combine="max"):
    """float64 [n, n_items]; KQ > 1: the maximum over the row's KQ queries.  A score outside the fp32 range is +-inf, as it is
    at the end of any fp32 chain whose partial sums are monotone (the non-finite cases are built that way)"""
    with np.errstate(invalid="ignore", over="ignore"):
        S = np.asarray(Qr, np.float64) @ np.asarray(I, np.float64).T
        S = np.where(np.abs(S) >= F32_OVERFLOW, np.sign(S) * np.inf, S)
        if KQ > 1:
            S = S.reshape(-1, KQ, S.shape[1])
            S = S.max(axis=1) if combine == "max" else S.sum(axis=1)
    return S


def mask_matrix(n, n_items, mask_row, ptr, idx):
    M = np.zeros((n, n_items), bool)
    if ptr is not None:
        for e in range(n):
            M[e, idx[ptr[mask_row[e]]:ptr[mask_row[e] + 1]]] = True
    return M


def _ranks(S, t, M, n_items, nan_last=True, ge=False):
    with np.errstate(invalid="ignore"):
        beat = (S >= t[:, None]) if ge else (S > t[:, None])
    rank = 1 + (beat & ~M).sum(axis=1).astype(np.int64)
    if nan_last:
        rank[np.isnan(t)] = n_items + 1
    return rank


def rank_ref(Q, I, target, mask_row, ptr, idx, KQ=1):
    """Q: the rows' own queries (row_queries).  Returns int64 [n]."""
    S = scores64(Q, I, KQ)
    n = len(target)
    return _ranks(S, S[np.arange(n), target], mask_matrix(n, len(I), mask_row, ptr, idx), len(I))


def case_ref(c):
    """(rank int64 [n], target score float64 [n], tied bool [n]: an unmasked item other than the target scores exactly the
    target's score)"""
    n, n_items = len(c["target"]), len(c["I"])
    S = scores64(row_queries(c), c["I"], c["KQ"])
    t = S[np.arange(n), c["target"]]
    M = mask_matrix(n, n_items, c["mask_row"], c["ptr"], c["idx"])
    eq = (S == t[:, None]) & ~M
    eq[np.arange(n), c["target"]] = False
    return _ranks(S, t, M, n_items), t, eq.any(axis=1)


def per_row_csr(c):
    """the mask with one list per evaluation row: (ptr int64 [n + 1], idx int32), or (None, None)"""
    if c["ptr"] is None:
        return None, None
    lists = [c["idx"][c["ptr"][r]:c["ptr"][r + 1]] for r in c["mask_row"]]
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(v) for v in lists])
    idx = np.concatenate(lists).astype(np.int32) if ptr[-1] else np.zeros(1, np.int32)
    return ptr, idx


def csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(v) for v in lists])
    idx = np.concatenate([np.asarray(v, np.int32) for v in lists]) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, np.concatenate([idx, np.zeros(1, np.int32)])      # never an empty device array


def with_mask(c, kind):
    """the same case without a mask ("none") or with every list full ("full")"""
    c = dict(c)
    if kind == "none":
        c["mask_row"] = c["ptr"] = c["idx"] = None
    else:
        n_items, n = len(c["I"]), len(c["target"])
        c["mask_row"] = np.arange(n, dtype=np.int64) % 3
        c["ptr"], c["idx"] = csr([np.arange(n_items)] * 3)
    if c["entry"] == "rank_eval":
        c["entry"] = "rank_eval_rows"
    return c


# ------------------------------------------------------------------------------------------------------------ the cases
N_LISTS = 50
FORCED = (0, 31, 32, 63, 64, 2047, 2048)


def edge_masks(rng, n, n_items):
    """50 lists shared among the rows, mask_row[e] != e.  List 7 holds every item, lists 9, 19, .. are empty, every other one
    is a random tenth of the items; the odd ones hold every column of FORCED and n_items - 1 that exists, the even ones none
    of them: a masked and an unmasked item on the first and last column of a tile and of a chunk.  Rows 0..15 of every odd
    slab of 32 rows take an empty list: there only the upper half of the slab is masked."""
    forced = np.asarray(sorted(set(j for j in FORCED + (n_items - 1,) if j < n_items)))
    lists = []
    for L in range(N_LISTS):
        if L == 7:
            lists.append(np.arange(n_items))
        elif L % 10 == 9:
            lists.append(np.zeros(0, np.int64))
        else:
            m = rng.random_sample(n_items) < 0.1
            m[forced] = L % 2 == 1
            lists.append(np.flatnonzero(m))
    e = np.arange(n)
    mask_row = (7 * e + 3) % N_LISTS
    low_half_of_odd_slab = ((e // 32) % 2 == 1) & (e % 32 < 16)
    mask_row = np.where(low_half_of_odd_slab, 9 + 10 * ((e // 2) % 5), mask_row).astype(np.int64)
    assert (mask_row != e).all()
    return lists, mask_row


def pick_targets(rng, n, n_items, lists, mask_row):
    """every fifth row has its own target masked (where its list is not empty), the others an unmasked one (where there is
    one)"""
    target = rng.randint(0, n_items, n).astype(np.int64)
    for e in range(n):
        own = lists[mask_row[e]]
        if e % 5 == 0 and len(own):
            target[e] = own[rng.randint(len(own))]
        elif e % 5 and len(own) < n_items:
            while target[e] in own:
                target[e] = rng.randint(n_items)
    return target


def _case(family, name, entry, Q, I, target, KQ=1, query_row=None, mask_row=None, lists=None, eval_user=None):
    ptr, idx = csr(lists) if lists is not None else (None, None)
    return dict(family=family, name=name, entry=entry, D=Q.shape[1], KQ=KQ, Q=Q, I=I, target=np.asarray(target, np.int64),
                query_row=query_row, mask_row=mask_row, ptr=ptr, idx=idx, eval_user=eval_user)


def edges_case(D, n_items, n):
    seed = 1000 * D + 7 * n_items + n
    rng = np.random.RandomState(seed)
    Q, I = grid_tables(D, n, n_items, seed + 1)
    lists, mask_row = edge_masks(rng, n, n_items)
    target = pick_targets(rng, n, n_items, lists, mask_row)
    return _case("edges", "edges-D%d-items%d-n%d" % (D, n_items, n), "rank_eval_rows", Q, I, target, mask_row=mask_row, lists=lists)


ONE_WINNER_ITEMS = CHUNK + 1 + 64
ONE_WINNER_TARGET = 100


def one_winner_case(D, row, winner):
    """every query the first unit vector, every item zero but the target (0.5) and one winner (1.0); row < 0: no mask at all,
    otherwise row `row` alone has a mask list and it holds the winner alone"""
    n = 128
    Q = np.zeros((n, D), np.float32); Q[:, 0] = 1.0
    I = np.zeros((ONE_WINNER_ITEMS, D), np.float32)
    I[ONE_WINNER_TARGET, 0], I[winner, 0] = 0.5, 1.0
    target = np.full(n, ONE_WINNER_TARGET)
    if row < 0:
        return _case("one_winner", "one_winner-D%d-nomask-w%d" % (D, winner), "rank_eval_rows", Q, I, target)
    mask_row = np.zeros(n, np.int64); mask_row[row] = 1
    return _case("one_winner", "one_winner-D%d-row%d-w%d" % (D, row, winner), "rank_eval_rows", Q, I, target, mask_row=mask_row,
                 lists=[[], [winner]])


def ties_case(D):
    """seven item classes (I[j] = I[j % 7]); every 16th query row is zero; the targets walk through the classes; list 1 hides
    the first 150 members of class 2, list 2 the first 150 of class 5 and the whole of class 0"""
    n, n_items = 129, CHUNK + 1
    Q, I = grid_tables(D, n, 7, 31 * D)
    I = I[np.arange(n_items) % 7]
    Q[::16] = 0.0
    e = np.arange(n)
    target = (e % 7 + 7 * ((37 * e) % 290)).astype(np.int64)
    cls = np.arange(n_items) % 7
    lists = [[], np.flatnonzero(cls == 2)[:150], np.flatnonzero((cls == 0) | ((cls == 5) & (np.arange(n_items) < 1050)))]
    return _case("ties", "ties-D%d" % D, "rank_eval_rows", Q, I, target, mask_row=(e % 3).astype(np.int64), lists=lists)


def roles_users_case(D):
    """rank_eval: 40 users, each evaluated several times, the mask list is the user's"""
    n, n_items, n_users = 257, CHUNK + 1, 40
    rng = np.random.RandomState(77 + D)
    Q, I = grid_tables(D, n_users, n_items, 78 + D)
    lists = [np.flatnonzero(rng.random_sample(n_items) < 0.1) if u % 8 else np.zeros(0, np.int64) for u in range(n_users)]
    eu = rng.randint(0, n_users, n).astype(np.int64)
    return _case("roles", "roles-users-D%d" % D, "rank_eval", Q, I, rng.randint(0, n_items, n), query_row=eu, mask_row=eu,
                 lists=lists, eval_user=eu)


def roles_rows_case(D):
    """rank_eval_rows: the queries stored in another order, rows 0 and 1 sharing one query row"""
    n, n_items = 129, CHUNK + 1
    rng = np.random.RandomState(91 + D)
    Q, I = grid_tables(D, n, n_items, 92 + D)
    lists, mask_row = edge_masks(rng, n, n_items)
    query_row = rng.permutation(n).astype(np.int64)
    query_row[1] = query_row[0]
    return _case("roles", "roles-rows-D%d" % D, "rank_eval_rows", Q, I, pick_targets(rng, n, n_items, lists, mask_row),
                 query_row=query_row, mask_row=mask_row, lists=lists)


def roles_multi_case(D, KQ, n):
    n_items = CHUNK + 1
    seed = 5000 + 100 * D + 10 * KQ + n
    rng = np.random.RandomState(seed)
    Q, I = grid_tables(D, n * KQ, n_items, seed + 1)
    lists, mask_row = edge_masks(rng, n, n_items)
    target = pick_targets(rng, n, n_items, lists, mask_row)
    for e in range(1, n, 2):              # odd rows: the interest that scores the target best is not interest 0
        own = Q[e * KQ:(e + 1) * KQ]
        if KQ > 1 and (own @ I[target[e]]).argmax() == 0:
            Q[e * KQ:(e + 1) * KQ] = np.roll(own, 1, axis=0)
    return _case("roles", "roles-multi-D%d-KQ%d-n%d" % (D, KQ, n), "rank_eval_multi", Q, I, target, KQ=KQ, mask_row=mask_row,
                 lists=lists)


# rows of a non-finite case
NF_NAN_QUERY = (3, 128)       # a NaN in (every one of) the row's queries: every score of the row is NaN
NF_NAN_TARGET = (20, 40, 85)  # the target's item row holds a NaN; row 20: another mask, row 40: no mask, row 85: target masked
NF_POS_INF, NF_NEG_INF = 70, 100
NF_NAN_ITEM, NF_POS_ITEM, NF_NEG_ITEM = 65, 2048, 2112


def nonfinite_case(D, KQ):
    """a grid case with non-finite scores.  Item NF_NAN_ITEM holds a NaN: its score is NaN for every row, so it never counts,
    and the rows NF_NAN_TARGET, which have it as their target, rank n_items + 1; the rows NF_NAN_QUERY hold a NaN in every one
    of their queries.  Items NF_POS_ITEM / NF_NEG_ITEM are +-2^127 in their first
    two components and zero elsewhere: their score is (q0 + q1) * 2^127 rounded once, the same in every order of the chain,
    and +-inf exactly where q0 = q1 = +-1 -- which rows NF_POS_INF and NF_NEG_INF have, with these items as their targets."""
    n, n_items = 129, ONE_WINNER_ITEMS
    seed = 9000 + 10 * D + KQ
    rng = np.random.RandomState(seed)
    Q, I = grid_tables(D, n * KQ, n_items, seed + 1)
    lists, mask_row = edge_masks(rng, n, n_items)
    target = pick_targets(rng, n, n_items, lists, mask_row)
    I[NF_NAN_ITEM, D // 2] = np.nan
    for item, sign in ((NF_POS_ITEM, 1.0), (NF_NEG_ITEM, -1.0)):
        I[item] = 0.0
        I[item, :2] = sign * 2.0 ** 127
    for e in NF_NAN_QUERY:
        Q[e * KQ:(e + 1) * KQ, 1] = np.nan
    for e in (NF_POS_INF, NF_NEG_INF):
        Q[e * KQ:(e + 1) * KQ, :2] = 1.0
    target[list(NF_NAN_TARGET)] = NF_NAN_ITEM
    target[NF_POS_INF], target[NF_NEG_INF] = NF_POS_ITEM, NF_NEG_ITEM
    lists = [np.asarray(v) for v in lists]
    other, none, own = (int(mask_row[e]) for e in NF_NAN_TARGET)
    assert len(lists[none]) == 0 and len({other, none, own, 7}) == 4
    lists[own] = np.union1d(lists[own], [NF_NAN_ITEM])
    lists[other] = np.setdiff1d(lists[other], [NF_NAN_ITEM])
    assert len(lists[other])
    return _case("nonfinite", "nonfinite-D%d-KQ%d" % (D, KQ), "rank_eval_multi" if KQ > 1 else "rank_eval_rows", Q, I, target,
                 KQ=KQ, mask_row=mask_row, lists=lists)


EDGE_ITEMS = (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4097)
EDGE_ROWS = (1, 127, 128, 129, 257)
ONE_WINNER_ROWS = (0, 31, 32, 63, 64, 95, 96, 127)
ONE_WINNER_COLS = (0, 63, 64, 2047, 2048, 2049 + 63)


def _build_cases():
    out = {}

    def add(fn, *a):
        out[_name(fn, a)] = functools.partial(fn, *a)

    for D in LDS_D + REGA_D:
        for n_items in EDGE_ITEMS:
            add(edges_case, D, n_items, 129)
        for n in EDGE_ROWS:
            if n != 129:
                add(edges_case, D, CHUNK + 1, n)
    for D in (8, 24):
        for w in ONE_WINNER_COLS:
            add(one_winner_case, D, -1, w)
            for r in ONE_WINNER_ROWS:
                add(one_winner_case, D, r, w)
    for D in (16, 24):
        add(ties_case, D)
    for D in (24, 64):
        add(roles_users_case, D)
        add(roles_rows_case, D)
        for KQ in (1, 2, 4):
            for n in (1, 31, 32, 33, 129):
                add(roles_multi_case, D, KQ, n)
    return out


def _name(fn, a):
    if fn is edges_case:
        return "edges-D%d-items%d-n%d" % a
    if fn is one_winner_case:
        return "one_winner-D%d-%s-w%d" % (a[0], "nomask" if a[1] < 0 else "row%d" % a[1], a[2])
    if fn is ties_case:
        return "ties-D%d" % a
    if fn is roles_users_case:
        return "roles-users-D%d" % a
    if fn is roles_rows_case:
        return "roles-rows-D%d" % a
    return "roles-multi-D%d-KQ%d-n%d" % a


CASES = _build_cases()
NONFINITE = {"nonfinite-D%d-KQ%d" % (D, KQ): functools.partial(nonfinite_case, D, KQ) for D in (24, 64) for KQ in (1, 2)}
FAMILIES = ("edges", "one_winner", "ties", "roles", "nonfinite")


@functools.lru_cache(maxsize=None)
def case(name):
    c = (CASES.get(name) or NONFINITE[name])()
    assert c["name"] == name
    return c


def family(name):
    return name.split("-")[0]


# ------------------------------------------------------------------------------------------------------- wrong variants
def _drop_first_of_chunk(M):
    M = M.copy()
    for c0 in range(0, M.shape[1], CHUNK):
        part = M[:, c0:c0 + CHUNK]
        rows = np.flatnonzero(part.any(axis=1))
        part[rows, part[rows].argmax(axis=1)] = False
    return M


def _drop_last_of_tile(M, T):
    M = M.copy()
    for j0 in range(0, M.shape[1], T):
        part = M[:, j0:j0 + T]
        rows = np.flatnonzero(part.any(axis=1))
        part[rows, part.shape[1] - 1 - part[rows, ::-1].argmax(axis=1)] = False
    return M


def _slab_upper_half_unseen(M, T):
    """a slab of 32 rows takes the unmasked shortcut in a tile whenever none of its rows 0..15 has a masked item there"""
    M = M.copy()
    for r0 in range(0, M.shape[0], 32):
        for j0 in range(0, M.shape[1], T):
            if not M[r0:r0 + 16, j0:j0 + T].any():
                M[r0:r0 + 32, j0:j0 + T] = False
    return M


SINGLE_VARIANTS = ("ge", "last_partial_tile_dropped", "zero_padding_counted", "items_from_2048_ignored",
                   "first_masked_of_chunk_lost", "last_masked_of_tile_lost", "mask_from_query_row", "query_from_mask_row",
                   "slab_upper_half_unseen", "own_column_counted")
MULTI_VARIANTS = ("sum_over_kq", "target_from_interest_0", "kq_group_shifted")
VARIANTS = SINGLE_VARIANTS + MULTI_VARIANTS + ("nan_target_ranks_first",)


def rank_wrong(c, variant):
    """the ranks a kernel with the named defect would return for the case"""
    assert variant in VARIANTS, variant
    n, n_items, KQ, D = len(c["target"]), len(c["I"]), c["KQ"], c["D"]
    T = tile_of(D)
    rows = np.arange(n)
    Qr = row_queries(c)
    mask_row = c["mask_row"]
    if variant == "mask_from_query_row" and c["ptr"] is not None:
        qrow = c["query_row"] if c["query_row"] is not None else rows
        mask_row = qrow % (len(c["ptr"]) - 1)
    if variant == "query_from_mask_row" and c["ptr"] is not None and KQ == 1:
        Qr = c["Q"][c["mask_row"] % len(c["Q"])]
    if variant == "kq_group_shifted":
        Qr = np.roll(Qr, -1, axis=0)
    S = scores64(Qr, c["I"], KQ, "sum" if variant == "sum_over_kq" else "max")
    t = S[rows, c["target"]]
    if variant == "target_from_interest_0":
        t = scores64(Qr[::KQ], c["I"])[rows, c["target"]]
    M = mask_matrix(n, n_items, mask_row, c["ptr"], c["idx"])
    if variant == "first_masked_of_chunk_lost":
        M = _drop_first_of_chunk(M)
    elif variant == "last_masked_of_tile_lost":
        M = _drop_last_of_tile(M, T)
    elif variant == "slab_upper_half_unseen":
        M = _slab_upper_half_unseen(M, T)
    elif variant == "last_partial_tile_dropped":
        M[:, n_items // T * T:] = True
    elif variant == "items_from_2048_ignored":
        M[:, CHUNK:] = True
    rank = _ranks(S, t, M, n_items, nan_last=variant != "nan_target_ranks_first", ge=variant == "ge")
    if variant == "zero_padding_counted":
        rank += (-n_items % T) * (t < 0)
    elif variant == "own_column_counted":
        rank += ~M[rows, c["target"]] & ~np.isnan(t)
    return rank


# a case named for every variant: the narrowest one in which the defect must show
NAMED_FOR = {
    "ge": "ties-D16",
    "last_partial_tile_dropped": "edges-D8-items65-n129",
    "zero_padding_counted": "edges-D24-items33-n129",
    "items_from_2048_ignored": "one_winner-D8-nomask-w2048",
    "first_masked_of_chunk_lost": "one_winner-D8-row32-w2048",
    "last_masked_of_tile_lost": "one_winner-D24-row64-w63",
    "mask_from_query_row": "roles-rows-D24",
    "query_from_mask_row": "edges-D16-items64-n129",
    "slab_upper_half_unseen": "one_winner-D8-row31-w64",
    "own_column_counted": "edges-D4-items1-n129",
    "sum_over_kq": "roles-multi-D24-KQ2-n33",
    "target_from_interest_0": "roles-multi-D64-KQ4-n32",
    "kq_group_shifted": "roles-multi-D64-KQ2-n31",
    "nan_target_ranks_first": "nonfinite-D24-KQ1",
}
