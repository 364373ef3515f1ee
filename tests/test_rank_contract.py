"""The exact cases of tests/rank_ref.py judged on the CPU: they are exact in fp32, the counting rule and the reference's sort
say the same thing on them, they hold the ties they are meant to hold, and every plausible defect of the ranking kernels moves
a rank in them.  No kernel runs here; tests/test_hip_rank_exact.py runs the kernels on the same cases."""
import numpy as np
import pytest

import oracle
import rank_ref as R

ALL = list(R.CASES)


def test_fp32_scores_are_the_float64_scores_bit_for_bit():
    """a case that fails this is not a case: |score| <= D <= 252 in multiples of 1/64, below 2^24 / 64"""
    for name in ALL:
        c = R.case(name)
        Q, I = R.row_queries(c), c["I"]
        assert Q.dtype == np.float32 and I.dtype == np.float32 and c["D"] <= 252, name
        assert np.array_equal(Q * 8, np.round(Q * 8)) and np.array_equal(I * 8, np.round(I * 8)) and \
            max(np.abs(Q).max(), np.abs(I).max()) <= 1.0, name
        S64 = Q.astype(np.float64) @ I.astype(np.float64).T
        S32 = Q @ I.T
        assert S32.dtype == np.float32 and np.array_equal(S32.astype(np.float64), S64), name
        assert np.array_equal(S64.astype(np.float32).astype(np.float64), S64), name


def _sort_ranks(c):
    """oracle.eval_ranks (the reference's argsort, stable, the target first) on the case: one user and one mask list per row"""
    n = len(c["target"])
    ptr, idx = R.per_row_csr(c)
    rank, _ = oracle.eval_ranks(R.row_queries(c), c["I"], np.arange(n), c["target"], ptr, idx, KQ=c["KQ"])
    return rank


def test_the_counting_rule_and_the_stable_sort_agree_on_every_row():
    """rank_ref counts strictly greater scores; oracle.eval_ranks sorts, stably, with the target's score first.  On every row
    of every case, ties and masked targets included, the two are one number."""
    rows = tied = 0
    for name in ALL:
        c = R.case(name)
        ref, _, t = R.case_ref(c)
        assert np.array_equal(ref, R.rank_ref(R.row_queries(c), c["I"], c["target"], c["mask_row"], c["ptr"], c["idx"], c["KQ"]))
        assert np.array_equal(ref, _sort_ranks(c)), name
        rows += len(ref); tied += int(t.sum())
    print("rank contract: %d cases, %d rows, %d with an exact tie at the target: counting rule == stable sort" %
          (len(ALL), rows, tied))


def test_the_cases_are_what_they_claim():
    for name in ALL:
        c = R.case(name)
        n, n_items = len(c["target"]), len(c["I"])
        assert c["target"].min() >= 0 and c["target"].max() < n_items, name
        if c["ptr"] is not None:
            assert c["mask_row"].min() >= 0 and c["mask_row"].max() < len(c["ptr"]) - 1, name
            for r in range(len(c["ptr"]) - 1):
                v = c["idx"][c["ptr"][r]:c["ptr"][r + 1]]
                assert (np.diff(v) > 0).all() and (len(v) == 0 or (v[0] >= 0 and v[-1] < n_items)), name
        if c["family"] == "edges":
            M = R.mask_matrix(n, n_items, c["mask_row"], c["ptr"], c["idx"])
            assert (c["mask_row"] != np.arange(n)).all() and len(c["ptr"]) - 1 == R.N_LISTS
            lens = np.diff(c["ptr"])
            assert (lens == 0).sum() >= 5 and (lens == n_items).sum() >= 1
            edge = [j for j in R.FORCED + (n_items - 1,) if j < n_items]
            for j in edge:                         # both a masked and an unmasked row on every edge column
                if n >= 127:
                    assert M[:, j].any() and not M[:, j].all(), (name, j)
            own = M[np.arange(n), c["target"]]
            has_list = lens[c["mask_row"]] > 0
            assert np.array_equal(own[::5], has_list[::5]), name               # every fifth row: its own target masked
            rest = np.arange(n) % 5 != 0
            assert not own[rest & (lens[c["mask_row"]] < n_items)].any(), name
        if c["family"] == "one_winner":
            ref = R.case_ref(c)[0]
            want = np.full(n, 2)
            if c["ptr"] is not None:
                row = int(np.flatnonzero(c["mask_row"])[0])
                want[row] = 1
            assert np.array_equal(ref, want), name
        if c["entry"] == "rank_eval_multi" and c["KQ"] > 1 and n > 1:
            per = (R.row_queries(c).astype(np.float64) @ c["I"].astype(np.float64).T).reshape(n, c["KQ"], n_items)
            win = per.argmax(axis=1)
            assert (win.min(axis=1) != win.max(axis=1)).all(), name            # the winning interest differs between items
            assert (win[np.arange(n), c["target"]] != 0).mean() >= 1 / 3, name  # the target's best interest is not interest 0
    c = R.case("ties-D16")
    ref = R.case_ref(c)[0]
    assert (ref[::16] == 1).all() and not R.row_queries(c)[::16].any()
    assert set((c["target"] % 7).tolist()) == set(range(7))
    c = R.case("roles-rows-D24")
    assert c["query_row"][0] == c["query_row"][1] and not np.array_equal(c["query_row"], np.arange(len(c["target"])))
    c = R.case("roles-users-D64")
    assert len(set(c["eval_user"].tolist())) < len(c["eval_user"])
    query_rows = set(len(R.case(n)["target"]) * R.case(n)["KQ"] for n in ALL if n.startswith("roles-multi"))
    assert {31, 32, 33, 124, 128, 132} <= query_rows                   # n KQ on either side of a slab and of a workgroup


def _tie_case_names():
    return [n for n in ALL if R.family(n) == "ties" or (R.family(n) == "edges" and R.case(n)["D"] >= 16 and
                                                         len(R.case(n)["I"]) >= 2047)]


def test_more_than_half_of_the_rows_hold_an_exact_tie_with_the_target():
    """A condition on the inputs, no kernel involved: in the `ties` cases and in the `edges` cases with D >= 16 and at least
    2,047 items (a table of 65 items or fewer cannot hold the ties; those cases are there for the tile edges) an unmasked
    item other than the target scores exactly the target's score in more than half of the rows.  Shares measured over the
    rows of the cases named, lowest and highest per group:
        ties   D = 16: 0.97            D = 24: 0.95
        edges  D = 16: 0.91 .. 0.96    D = 24: 0.87 .. 0.95    D = 32: 0.90 .. 0.97    D = 64: 0.84 .. 0.92
               D = 128: 0.71 .. 0.88   D = 252: 0.64 .. 0.84
    (a row whose list is full, one in fifty, can hold none)."""
    by = {}
    for name in _tie_case_names():
        c = R.case(name)
        share = R.case_ref(c)[2].mean() if len(c["target"]) > 1 else None
        if share is None:
            continue                                  # the one-row case has no share to speak of
        by.setdefault((c["family"], c["D"]), []).append(share)
        assert share > 0.5, (name, share)
    for key in sorted(by):
        print("tie share %s D=%d: %d cases, %.2f .. %.2f" % (key + (len(by[key]), min(by[key]), max(by[key]))))
    assert len(by) == 2 + 6


def _changed(name, variant):
    c = R.case(name)
    return int((R.rank_wrong(c, variant) != R.case_ref(c)[0]).sum())


def test_every_wrong_variant_changes_a_rank():
    """The power of the cases.  Every variant changes a rank in the case named for it.  Over the `edges` family as a whole,
    every variant that can differ from the kernel at one query per row changes at least 5 % of the rows (the three KQ
    variants are the identity at KQ = 1, and edges has no NaN: they are judged on `roles` and `nonfinite`).  In
    `one_winner`, losing the chunk's first or the tile's last masked item changes exactly the one masked row, and so does a
    slab that overlooks its upper half when that row is in one; with the row in a lower half it changes nothing."""
    names = ALL + list(R.NONFINITE)
    table = {v: dict.fromkeys(R.FAMILIES, 0) for v in R.VARIANTS}
    rows = dict.fromkeys(R.FAMILIES, 0)
    for name in names:
        c = R.case(name)
        ref = R.case_ref(c)[0]
        rows[c["family"]] += len(ref)
        for v in R.VARIANTS:
            diff = np.flatnonzero(R.rank_wrong(c, v) != ref)
            table[v][c["family"]] += len(diff)
            if c["family"] == "one_winner" and c["ptr"] is not None:
                row = int(np.flatnonzero(c["mask_row"])[0])
                if v in ("first_masked_of_chunk_lost", "last_masked_of_tile_lost") or \
                        (v == "slab_upper_half_unseen" and row % 32 >= 16):
                    assert diff.tolist() == [row], (name, v, diff)
                elif v == "slab_upper_half_unseen":
                    assert len(diff) == 0, (name, v, diff)
    print("\nrows whose rank a wrong variant changes (rows per family: %s)" % ", ".join("%s %d" % kv for kv in rows.items()))
    print("%-28s" % "variant" + "".join("%12s" % f for f in R.FAMILIES))
    for v in R.VARIANTS:
        print("%-28s" % v + "".join("%12d" % table[v][f] for f in R.FAMILIES))
    for v in R.VARIANTS:
        assert _changed(R.NAMED_FOR[v], v) >= 1, (v, R.NAMED_FOR[v])
        assert sum(table[v].values()) > 0, v
    for v in R.SINGLE_VARIANTS:
        assert table[v]["edges"] >= 0.05 * rows["edges"], (v, table[v]["edges"], rows["edges"])
    for v in R.MULTI_VARIANTS:
        assert table[v]["roles"] >= 0.05 * rows["roles"], (v, table[v]["roles"])


def test_rank_ref_carries_the_rule_for_non_finite_targets():
    """NaN target: n_items + 1 whatever the mask; a NaN score of another item never counts; +inf target: 1; -inf target:
    1 + the unmasked items above -inf"""
    for name in R.NONFINITE:
        c = R.case(name)
        n_items = len(c["I"])
        ref, t, _ = R.case_ref(c)
        S = R.scores64(R.row_queries(c), c["I"], c["KQ"])
        M = R.mask_matrix(len(ref), n_items, c["mask_row"], c["ptr"], c["idx"])
        for e in R.NF_NAN_QUERY:
            assert np.isnan(S[e]).all() and ref[e] == n_items + 1
        masked = [bool(M[e, R.NF_NAN_ITEM]) for e in R.NF_NAN_TARGET]
        assert masked == [False, False, True] and M[R.NF_NAN_TARGET[0]].any() and not M[R.NF_NAN_TARGET[1]].any()
        for e in R.NF_NAN_TARGET:
            assert np.isnan(t[e]) and np.isfinite(np.delete(S[e], R.NF_NAN_ITEM)).all() and ref[e] == n_items + 1
        assert t[R.NF_POS_INF] == np.inf and ref[R.NF_POS_INF] == 1
        e = R.NF_NEG_INF
        assert t[e] == -np.inf and not M[e].any() and ref[e] == n_items - 1      # all but itself and the NaN item
        finite = np.isfinite(t)
        assert np.isnan(S[finite][:, R.NF_NAN_ITEM]).all()
        S0 = np.where(np.isnan(S), -np.inf, S)                                    # a NaN item counted as a loser: same ranks
        assert np.array_equal(ref[finite], 1 + ((S0 > t[:, None]) & ~M).sum(axis=1)[finite])
        wrong = R.rank_wrong(c, "nan_target_ranks_first")
        nan_rows = sorted(R.NF_NAN_QUERY + R.NF_NAN_TARGET)
        assert np.flatnonzero(wrong != ref).tolist() == nan_rows and (wrong[nan_rows] == 1).all()
