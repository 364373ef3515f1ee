"""Top-K over several interests on the device (K23, wr_topk_recommend_multi): against the score chains of wr_rank_eval_rows bit
for bit, against the float64 restatement of tests/if4rec_topk_ref.py, on tables that make every item a candidate, in row blocks,
under permutations of the interests, and through HipRunner / the launcher for IF4Rec (--interest_topk_native 1)."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import if4rec_ref as R  # noqa: E402
import if4rec_topk_ref as T  # noqa: E402
from whisprrec_amd import hip_ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KS = (1, 20, 129, 256)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.int32)


def _call(c, k, with_interest=True, queries=None):
    masked = c.get("mask_row") is not None
    out = hip_ops.topk_recommend_multi(_t(c["queries"] if queries is None else queries), _t(c["items"]), k,
                                       _t(c["mask_row"]) if masked else None, _t(c["mask_ptr"]) if masked else None,
                                       _t(c["mask_idx"]) if masked else None, with_interest=with_interest)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


# ------------------------------------------------------------------------------------------------ 1. exact composition
def _chains(queries, items):
    """[n, KQ, n_items] fp32: every <query row, item> as wr_rank_eval_rows' target_score (the MFMA's chain bit for bit), the
    pairs enumerated through query_row / eval_target.  The item table goes in slices of 128 rows: a pair's target_score does not
    depend on the other items, and the ranks that come with it (not used) then cost 128 scores per pair instead of n_items."""
    n, KQ, D = queries.shape
    n_items, step = items.shape[0], 128
    Q, I = _t(queries.reshape(n * KQ, D)), _t(items)
    out = torch.empty((n * KQ, n_items), dtype=torch.float32, device=DEV)
    for j0 in range(0, n_items, step):
        w = min(step, n_items - j0)
        qr = torch.arange(n * KQ, device=DEV).repeat_interleave(w)
        et = torch.arange(w, device=DEV).repeat(n * KQ)
        _, ts = hip_ops.rank_eval_rows(Q, I[j0:j0 + w].contiguous(), et, query_row=qr)
        out[:, j0:j0 + w] = ts.view(n * KQ, w)
    return out.cpu().numpy().reshape(n, KQ, n_items)


def _exact_case(D, n_items, n, KQ):
    """make_rank_case with two more rows of interest: row 5 takes a new list that leaves 3 items, row 6 the empty list"""
    c = R.make_rank_case(D, n_items, n, KQ)
    rng = np.random.RandomState(D + n_items)
    few = np.sort(rng.choice(n_items, size=n_items - 3, replace=False)).astype(np.int32)
    c["mask_idx"] = np.concatenate([c["mask_idx"], few])
    c["mask_ptr"] = np.concatenate([c["mask_ptr"], [c["mask_ptr"][-1] + few.size]]).astype(np.int64)
    c["mask_row"] = c["mask_row"].copy()
    c["mask_row"][5], c["mask_row"][6] = len(c["mask_ptr"]) - 2, 0
    assert c["mask_ptr"][1] == 0 and (c["mask_row"] != np.arange(n)).all()
    return c


@pytest.mark.parametrize("KQ", [1, 2, 4])
@pytest.mark.parametrize("D,n_items,n", [(64, 2100, 257), (32, 333, 129), (24, 500, 130), (16, 8300, 130)])
def test_lists_are_the_sorted_maxima_of_the_rank_kernels_chains(D, n_items, n, KQ):
    c = _exact_case(D, n_items, n, KQ)
    per = _chains(c["queries"], c["items"])
    S = per.max(axis=1)                                             # fp32: the maximum of the chains, no arithmetic
    for e in range(n):
        r = c["mask_row"][e]
        S[e, c["mask_idx"][c["mask_ptr"][r]:c["mask_ptr"][r + 1]]] = -np.inf
    order = np.argsort(-S, axis=1, kind="stable")
    left = np.isfinite(S).sum(axis=1)
    assert left[5] == 3 and left[6] == n_items
    padded = 0
    for k in KS:
        items, scores, interest = _call(c, k)
        assert items.shape == scores.shape == interest.shape == (n, k) and items.dtype == interest.dtype == np.int64
        kk = min(k, n_items)
        want_items = np.full((n, k), -1, np.int64)
        want_sc = np.full((n, k), -np.inf, np.float32)
        want_sc[:, :kk] = np.take_along_axis(S, order[:, :kk], axis=1)
        want_items[:, :kk] = np.where(np.isfinite(want_sc[:, :kk]), order[:, :kk], -1)
        assert np.array_equal(items, want_items), k                 # EVERY row
        assert np.array_equal(_bits(scores), _bits(want_sc)), k     # -inf at the padding included
        pad = items < 0
        assert np.array_equal(pad, np.arange(k)[None, :] >= left[:, None])
        padded += int(pad.any(axis=1).sum())
        safe = np.where(pad, 0, items)
        hit = np.take_along_axis(per, np.broadcast_to(safe[:, None, :], (n, KQ, k)), axis=2) == scores[:, None, :]
        assert hit.any(axis=1)[~pad].all()
        assert np.array_equal(interest, np.where(pad, -1, hit.argmax(axis=1))), k        # the smallest such q
        if KQ == 1:
            it1, sc1 = hip_ops.topk_recommend_rows(_t(c["queries"][:, 0, :]), _t(c["items"]), k, _t(c["mask_row"]), _t(c["mask_ptr"]),
                                                   _t(c["mask_idx"]))
            assert np.array_equal(it1.cpu().numpy(), items) and np.array_equal(_bits(sc1), _bits(scores))
            assert (interest[~pad] == 0).all()
    assert padded >= (3 if n_items != 333 else 10)                  # rows 5 at every k > 3; 30 % lists of 333 items at k = 256


# ------------------------------------------------------------------------------------------------ 2. the float64 restatement
def _ref_case(D, n_items, n, KQ, grid, seed):
    from test_hip_topk import _tables
    Q, I = _tables(D, n * KQ, n_items, seed, grid=grid)
    rng = np.random.RandomState(seed + 1)
    lists = [np.flatnonzero(rng.random_sample(n_items) < 0.1).astype(np.int32) for _ in range(40)]
    return dict(queries=Q.reshape(n, KQ, D), items=I, mask_idx=np.concatenate(lists),
                mask_ptr=np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.int64),
                mask_row=rng.randint(0, 40, n).astype(np.int64))


@pytest.mark.parametrize("KQ", [2, 4])
@pytest.mark.parametrize("D,n_items,k", [(64, 2100, 100), (24, 500, 256), (32, 333, 256), (16, 8300, 100)])
def test_grid_tables_equal_the_float64_sort_ties_included(D, n_items, k, KQ):
    """multiples of 1/8 in [-1, 1]: every fp32 chain is exact, so every row, its ties and its first winning interest included,
    is the float64 restatement's"""
    n = 130
    c = _ref_case(D, n_items, n, KQ, True, 23 * D + n_items + KQ)
    items, scores, interest = _call(c, k)
    ref_items, ref_sc, ref_int, _ = T.topk_ref(c, k)
    ties = int((ref_sc[:, 1:] == ref_sc[:, :-1])[np.isfinite(ref_sc[:, 1:])].sum())
    print("parity if4rec topk grid D=%d n_items=%d k=%d KQ=%d: rows %d, tied neighbours %d, rows differing %d"
          % (D, n_items, k, KQ, n, ties, int((items != ref_items).any(axis=1).sum())))
    assert ties > n                                                 # the case does hold ties
    assert np.array_equal(items, ref_items)
    assert np.array_equal(scores.astype(np.float64), ref_sc)
    assert np.array_equal(interest, ref_int)


@pytest.mark.parametrize("KQ", [1, 2, 4])
@pytest.mark.parametrize("D,n_items,k", [(16, 777, 10), (24, 5000, 10), (64, 2100, 20), (32, 333, 20), (16, 8300, 20), (64, 2100, 1)])
def test_gaussian_tables_match_the_float64_restatement(D, n_items, k, KQ):
    """score standard deviation 10; a row is judged when its reference scores at positions 1..k+1 lie at least 1e-4 apart"""
    n = 200
    c = _ref_case(D, n_items, n, KQ, False, 31 * D + n_items + k + KQ)
    items, scores, interest = _call(c, k)
    ref_items, ref_sc, ref_int, judged = T.topk_ref(c, k)
    differing = int((items[judged] != ref_items[judged]).any(axis=1).sum())
    print("parity if4rec topk D=%d n_items=%d k=%d KQ=%d: judged share %.4f, judged rows differing %d"
          % (D, n_items, k, KQ, judged.mean(), differing))
    fin = np.isfinite(ref_sc)
    assert np.array_equal(np.isfinite(scores), fin)
    # an fp32 chain of D terms against float64: the bound test_hip_topk uses for the same chains
    np.testing.assert_allclose(scores[fin], ref_sc[fin], rtol=1e-5, atol=1e-5 * np.abs(ref_sc[fin]).max())
    assert judged.mean() >= 0.9, judged.mean()
    assert differing == 0


# ------------------------------------------------------------------------------------------------ 3. every item a candidate
@pytest.mark.parametrize("KQ", [2, 4])
@pytest.mark.parametrize("k", [20, 200])
@pytest.mark.parametrize("rising", [True, False])
def test_every_item_a_candidate_and_none(k, KQ, rising):
    """scores rise with the item id for every row: every tile fills the staging and the merges run as often as they can; the
    mirrored table makes every item after the first k lose at the threshold"""
    D, n_items, n = 8, 1500, 70
    items = np.zeros((n_items, D), np.float32)
    ids = np.arange(n_items)
    items[:, 0] = (ids if rising else n_items - 1 - ids) / 1024.0
    queries = np.zeros((n, KQ, D), np.float32)
    queries[:, :, 0] = 1.0 + np.arange(KQ)[None, :]
    rng = np.random.RandomState(k + KQ)
    lists = [np.flatnonzero(rng.random_sample(n_items) < 0.2).astype(np.int32) for _ in range(9)]
    c = dict(queries=queries, items=items, mask_idx=np.concatenate(lists),
             mask_ptr=np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.int64),
             mask_row=((np.arange(n) + 1) % 9).astype(np.int64))
    got, scores, interest = _call(c, k)
    for e in range(n):
        free = np.setdiff1d(ids, lists[c["mask_row"][e]])
        want = free[::-1][:k] if rising else free[:k]
        assert np.array_equal(got[e], want), e
    assert np.array_equal(scores, KQ * items[got, 0]) and (interest == KQ - 1).all()


# ------------------------------------------------------------------------------------------------ 4. row blocks
def test_row_blocks_under_the_workspace_cap_equal_the_whole_call(monkeypatch):
    n, KQ, D, n_items, k = 700, 2, 32, 900, 10
    c = R.make_rank_case(D, n_items, n, KQ)
    whole = _call(c, k)
    need = hip_ops.abi.lib().wr_topk_multi_workspace_bytes(n, n_items, D, KQ, k)
    assert need > hip_ops.abi.lib().wr_topk_multi_workspace_bytes(350, n_items, D, KQ, k)
    monkeypatch.setattr(hip_ops, "TOPK_WORKSPACE_CAP", need - 1)    # the rows are halved until a block fits: 2 blocks of 350
    blocked = _call(c, k)
    assert len(blocked) == 3
    for a, b in zip(whole, blocked):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ 5. invariances
@pytest.mark.parametrize("D,KQ", [(64, 4), (24, 2)])
def test_interest_order_repeat_and_full_mask(D, KQ):
    n, n_items, k = 130, 2100, 20
    c = R.make_rank_case(D, n_items, n, KQ)
    items, scores, interest = _call(c, k)
    again = _call(c, k)
    assert np.array_equal(items, again[0]) and np.array_equal(_bits(scores), _bits(again[1])) and np.array_equal(interest, again[2])
    rev = _call(c, k, queries=c["queries"][:, ::-1, :])
    assert np.array_equal(items, rev[0]) and np.array_equal(_bits(scores), _bits(rev[1]))
    two = _call(c, k, with_interest=False)
    assert len(two) == 2 and np.array_equal(items, two[0]) and np.array_equal(_bits(scores), _bits(two[1]))
    full = dict(c, mask_ptr=np.array([0, n_items], np.int64), mask_idx=np.arange(n_items, dtype=np.int32), mask_row=np.zeros(n, np.int64))
    items, scores, interest = _call(full, k)
    assert (items == -1).all() and np.isneginf(scores).all() and (interest == -1).all()


# ------------------------------------------------------------------------------------------------ 6. runner and launcher
def _argv(path, tmp, extra):
    return ["--model_name", "IF4Rec", "--runner_name", "HipRunner", "--dataset", "ml-100k", "--path", path, "--epoch", "1",
            "--batch_size", "1024", "--eval_batch_size", "2048", "--lr", "1e-3", "--l2", "0.0", "--emb_size", "32", "--history_max", "20",
            "--n_head", "4", "--encoder_dropout", "0.0", "--log_file", str(tmp / "log.txt"), "--model_path", str(tmp / "m.pt"),
            "--num_workers", "0", "--topk", "5,10", "--metric", "NDCG, HR", "--random_seed", "3407", "--seq_eval_native", "1",
            "--interest_native", "1", "--interest_topk_native", "1"] + extra


@pytest.fixture(scope="module")
def if4rec(tmp_path_factory):
    from test_reader import _write_inter
    from whisprrec_amd import main as launcher, runner
    tmp = tmp_path_factory.mktemp("if4rec_topk")
    g8 = np.load(os.path.join(GOLD, "g8_reader.npz"))
    path = _write_inter(g8, tmp)
    args, model_class, reader_class, runner_class = launcher.build_args(_argv(path, tmp, []))
    launcher.init_seed(args.random_seed)
    args.device = DEV
    corpus = reader_class(args).corpus()
    model = model_class(args, corpus).to(DEV)
    with torch.no_grad():
        model.i_embeddings.weight.mul_(30)                                      # scores spread: few near-ties
    ds = model_class.Dataset(model, corpus, "dev")
    pred = runner.BaseRunner(args).interface(ds).astype(np.float64)
    return dict(run=runner_class(args), ds=ds, model=model, corpus=corpus, S=pred[:, 1:], tmp=tmp, path=path)


def test_recommend_rows_equals_the_host_list(if4rec):
    run, ds, S, k = if4rec["run"], if4rec["ds"], if4rec["S"], 10
    items, scores, interest = run.recommend_rows(ds, k, with_interest=True)
    assert items.shape == (len(ds), k) and items.dtype == np.int64 and scores.dtype == np.float32 and interest.dtype == np.int64
    order = np.argsort(-S, axis=1, kind="stable")
    h_items = order[:, :k]
    top = np.take_along_axis(S, order[:, :k + 1], axis=1)
    gaps = -np.diff(np.where(np.isfinite(top), top, -1e30), axis=1)
    ok = gaps.min(axis=1) > 1e-5 * np.abs(S[np.isfinite(S)]).max()
    differing = int((items[ok] != h_items[ok]).any(axis=1).sum())
    print("parity if4rec topk runner: n_eval %d rows kept %.4f lists differing on kept rows %d" % (len(ds), ok.mean(), differing))
    assert ok.mean() >= 0.9 and differing == 0
    assert ((interest >= 0) & (interest < int(if4rec["model"].n_interests)))[items >= 0].all()
    two = run.recommend_rows(ds, k)
    assert len(two) == 2 and np.array_equal(two[0], items) and np.array_equal(_bits(two[1]), _bits(scores))


def test_rows_subset_exclude_and_recommend_next(if4rec):
    run, ds, model, corpus, k = if4rec["run"], if4rec["ds"], if4rec["model"], if4rec["corpus"], 10
    users, positions = np.asarray(ds.data["user_id"]), np.asarray(ds.data["position"])
    items, scores = run.recommend_rows(ds, k)
    sub = np.array([len(ds) - 1, 3, 3, 17, 0])
    sub_items, sub_scores = run.recommend_rows(ds, k, rows=sub)
    # the rows asked for, in that order.  The pooling shifts its scores by the maximum of the whole batch as the reference writes
    # it (IF4Rec.py:100), so a row's bits belong to its batch: the scores agree up to that rounding, the lists outright
    assert np.array_equal(sub_items, items[sub]) and np.array_equal(sub_items[1], sub_items[2])
    np.testing.assert_allclose(sub_scores, scores[sub], rtol=1e-4)
    sub_his = [[x[0] for x in corpus.user_his[users[r]][:positions[r]]] for r in sub]
    nx = run.recommend_next(model, corpus, sub_his, k, users=users[sub], with_interest=True)     # the same five rows, given directly
    rw = run.recommend_rows(ds, k, rows=sub, with_interest=True)
    assert np.array_equal(nx[0], rw[0]) and np.array_equal(nx[2], rw[2])
    np.testing.assert_allclose(nx[1], rw[1], rtol=1e-4)
    for r in range(0, len(ds), 7):                                              # a clicked item is never recommended
        clicked = corpus.train_clicked_set.get(users[r], set()) | corpus.residual_clicked_set.get(users[r], set())
        assert not (set(items[r].tolist()) & clicked)
    tr_items, _ = run.recommend_rows(ds, k, exclude="train")
    none_items, none_scores = run.recommend_rows(ds, k, exclude="none")
    assert all(not (set(tr_items[r].tolist()) & corpus.train_clicked_set[users[r]]) for r in range(len(ds)))
    assert (none_scores[:, 0] >= scores[:, 0]).all() and (none_items != items).any()
    histories = [[x[0] for x in corpus.user_his[u][:p]] for u, p in zip(users.tolist(), positions.tolist())]
    free_items, free_scores = run.recommend_next(model, corpus, histories, k)    # no users: no mask
    assert np.array_equal(free_items, none_items)
    np.testing.assert_allclose(free_scores, none_scores, rtol=1e-4)
    with pytest.raises(ValueError):
        run.recommend_rows(ds, k, exclude="bogus")
    with pytest.raises(NotImplementedError, match="recommend_rows"):
        run.recommend(model, corpus, users[:4], k)
    with pytest.raises(NotImplementedError, match="k=300"):
        run.recommend_rows(ds, 300)


def test_save_rec_results_writes_recommend_rows_items(if4rec):
    run, ds, k = if4rec["run"], if4rec["ds"], 10
    items, _ = run.recommend_rows(ds, k)
    path = run.save_rec_results(ds, k, str(if4rec["tmp"] / "rec-IF4Rec.csv"), sep="\t")
    with open(path, newline="") as f:
        rows = list(csv.reader(f, delimiter="\t"))
    users = np.asarray(ds.data["user_id"])
    assert rows[0] == ["user_id", "rec_items"] and len(rows) == 1 + len(ds)
    for r, (row, u) in enumerate(zip(rows[1:], users)):
        assert int(row[0]) == u and eval(row[1]) == items[r].tolist()


def test_launcher_run_ends_with_the_recommendation_file(tmp_path):
    from test_reader import _write_inter
    from whisprrec_amd import main as launcher
    g8 = np.load(os.path.join(GOLD, "g8_reader.npz"))
    path = _write_inter(g8, tmp_path)
    launcher.main(_argv(path, tmp_path, ["--save_rec", "10"]))
    rec = os.path.join(path, "ml-100k", "rec-IF4Rec.csv")
    assert os.path.exists(rec)
    with open(rec, newline="") as f:
        rows = list(csv.reader(f, delimiter="\t"))
    # one line per dev row of the sequential dataset (the rows that have a history), with that row's user
    args, model_class, reader_class, _ = launcher.build_args(_argv(path, tmp_path, []))
    args.device = DEV
    corpus = reader_class(args).corpus()
    ds = model_class.Dataset(model_class(args, corpus).to(DEV), corpus, "dev")
    assert rows[0] == ["user_id", "rec_items"] and len(rows) == 1 + len(ds)
    assert [int(row[0]) for row in rows[1:]] == np.asarray(ds.data["user_id"]).tolist()
    assert all(len(eval(row[1])) == 10 for row in rows[1:])
