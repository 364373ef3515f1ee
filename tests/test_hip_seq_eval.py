"""Ranking evaluation and top-K with one query per row (K14: wr_rank_eval_rows / wr_topk_recommend_rows) — bit for bit
against the per-user entries they generalise, against the oracle with the query role and the mask role apart, and through
HipRunner (--seq_eval_native 1, recommend_rows, recommend_next, save_rec_results) against the host path for SASRec.
Run with -rP for the `seq eval` lines."""
import csv
import os

import numpy as np
import pytest
import torch

import oracle
from whisprrec_amd import hip_ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mask_csr(rng, n_rows, n_items, max_len):
    """the rule of tests/test_hip_eval.py::_mask_csr: per row, randint(0, max_len) distinct items, ascending"""
    ptr = np.zeros(n_rows + 1, np.int64)
    chunks = []
    for r in range(n_rows):
        k = rng.randint(0, max_len)
        chunks.append(np.sort(rng.choice(n_items, k, replace=False)).astype(np.int32))
        ptr[r + 1] = ptr[r] + k
    return ptr, np.concatenate(chunks)


def _bits(x):
    return x.cpu().numpy().view(np.int32)


# ------------------------------------------------------------------------------------------------ 1. the existing entries
@pytest.mark.parametrize("D,n_items,n", [(64, 2100, 257), (32, 333, 129), (24, 500, 129), (252, 600, 140)])
def test_bitwise_equal_to_the_per_user_entries(D, n_items, n):
    """Q = U[eu], mask_row = eu: ranks, target scores, top-K items and scores of the per-row entries are those of rank_eval /
    topk_recommend, with the queries in order (query_row None) and stored permuted (query_row = perm).  No tolerance."""
    rng = np.random.RandomState(D + n_items)
    n_users = 400
    U = rng.standard_normal((n_users, D)).astype(np.float32)
    I = rng.standard_normal((n_items, D)).astype(np.float32)
    ptr, idx = _mask_csr(rng, n_users, n_items, min(60, n_items // 2))
    eu, et = rng.randint(0, n_users, n), rng.randint(0, n_items, n)
    perm = rng.permutation(n)
    Q = U[eu]
    Qp = np.empty_like(Q)
    Qp[perm] = Q                                          # row e's query sits in row perm[e]
    Ud, Id, eud, etd, ptrd, idxd = _t(U), _t(I), _t(eu), _t(et), _t(ptr), _t(idx)
    rank, tsc = hip_ops.rank_eval(Ud, Id, eud, etd, ptrd, idxd)
    rank0, tsc0 = hip_ops.rank_eval(Ud, Id, eud, etd)
    for name, qmat, qrow in (("in order", _t(Q), None), ("permuted", _t(Qp), _t(perm))):
        r, s = hip_ops.rank_eval_rows(qmat, Id, etd, eud, ptrd, idxd, query_row=qrow)
        assert torch.equal(r, rank) and np.array_equal(_bits(s), _bits(tsc)), name
        r, s = hip_ops.rank_eval_rows(qmat, Id, etd, query_row=qrow)
        assert torch.equal(r, rank0) and np.array_equal(_bits(s), _bits(tsc0)), name + ", no mask"
    for k in (1, 20, 256):
        items, scores = hip_ops.topk_recommend(Ud, Id, eud, k, ptrd, idxd)
        items0, scores0 = hip_ops.topk_recommend(Ud, Id, eud, k)
        for name, qmat, qrow in (("in order", _t(Q), None), ("permuted", _t(Qp), _t(perm))):
            it, sc = hip_ops.topk_recommend_rows(qmat, Id, k, eud, ptrd, idxd, query_row=qrow)
            assert torch.equal(it, items) and np.array_equal(_bits(sc), _bits(scores)), (name, k)
            it, sc = hip_ops.topk_recommend_rows(qmat, Id, k, query_row=qrow)
            assert torch.equal(it, items0) and np.array_equal(_bits(sc), _bits(scores0)), (name, k, "no mask")
    # a returned score is the target_score of that (row, item) pair
    it, sc = hip_ops.topk_recommend_rows(_t(Q), Id, 20, eud, ptrd, idxd)
    valid = (it >= 0).cpu().numpy()
    rows = np.repeat(np.arange(n), 20).reshape(n, 20)[valid]
    _, ts = hip_ops.rank_eval_rows(_t(Q), Id, it[torch.from_numpy(valid).to(DEV)], query_row=_t(rows))
    assert np.array_equal(_bits(ts), _bits(sc)[valid])


def test_topk_blocks_rows_under_the_workspace_cap(monkeypatch):
    """several blocks (the cap lowered): a block without query_row scores with ITS rows of query_mat and ITS mask rows"""
    rng = np.random.RandomState(5)
    n, n_items, D, k = 700, 900, 32, 10
    Q = rng.standard_normal((n, D)).astype(np.float32)
    I = rng.standard_normal((n_items, D)).astype(np.float32)
    ptr, idx = _mask_csr(rng, 50, n_items, 60)
    mrow = rng.randint(0, 50, n)
    perm = rng.permutation(n)
    Qp = np.empty_like(Q)
    Qp[perm] = Q
    whole = hip_ops.topk_recommend_rows(_t(Q), _t(I), k, _t(mrow), _t(ptr), _t(idx))
    need = hip_ops.abi.lib().wr_topk_workspace_bytes(n, n_items, D, k)
    monkeypatch.setattr(hip_ops, "TOPK_WORKSPACE_CAP", need - 1)     # the rows are halved until a block fits: 2 blocks of 350
    for qmat, qrow in ((_t(Q), None), (_t(Qp), _t(perm))):
        it, sc = hip_ops.topk_recommend_rows(qmat, _t(I), k, _t(mrow), _t(ptr), _t(idx), query_row=qrow)
        assert torch.equal(it, whole[0]) and np.array_equal(_bits(sc), _bits(whole[1]))


# ------------------------------------------------------------------------------------------------ 2. the oracle, roles apart
@pytest.mark.parametrize("D,n_items,n", [(64, 2100, 257), (32, 333, 129), (8, 777, 130), (16, 4133, 300), (24, 500, 129),
                                         (252, 600, 140)])
def test_ranks_match_oracle_with_query_and_mask_rows_apart(D, n_items, n):
    """every row its own query, 50 mask rows shared among the rows and mask_row[e] != e: a kernel that reads the mask of the
    query's row, or the query of the mask's row, gets most ranks wrong (the mask changes the rank of most rows)"""
    rng = np.random.RandomState(D + n_items)
    n_mask = 50
    Q = rng.standard_normal((n, D)).astype(np.float32)
    I = rng.standard_normal((n_items, D)).astype(np.float32)
    ptr, idx = _mask_csr(rng, n_mask, n_items, min(60, n_items // 2))
    mrow = rng.randint(0, n_mask, n)
    same = mrow == np.arange(n)
    mrow[same] = (mrow[same] + 1) % n_mask
    et = rng.randint(0, n_items, n)
    # the CSR expanded per evaluation row: the oracle keeps one index for both roles
    lens = (ptr[1:] - ptr[:-1])[mrow]
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    row_idx = np.concatenate([idx[ptr[m]:ptr[m + 1]] for m in mrow]).astype(np.int32)
    ref, margin = oracle.eval_ranks(Q, I, np.arange(n), et, row_ptr, row_idx)
    ref_nomask, margin_nomask = oracle.eval_ranks(Q, I, np.arange(n), et)
    ok = margin > 1e-4                                   # rows with a near-tie are decided by rounding, skip them
    print("seq eval oracle D=%d n_items=%d n=%d: kept %.3f, rank moved by the mask on %.3f of the rows"
          % (D, n_items, n, ok.mean(), (ref != ref_nomask).mean()))
    assert ok.mean() > 0.9
    rank, tsc = hip_ops.rank_eval_rows(_t(Q), _t(I), _t(et), _t(mrow), _t(ptr), _t(idx))
    assert np.array_equal(rank.cpu().numpy()[ok], ref[ok])
    assert np.allclose(tsc.cpu().numpy(), (Q * I[et]).sum(1), rtol=1e-5, atol=1e-5)
    # the same with the queries stored in another order
    perm = rng.permutation(n)
    Qp = np.empty_like(Q)
    Qp[perm] = Q
    rank_p, _ = hip_ops.rank_eval_rows(_t(Qp), _t(I), _t(et), _t(mrow), _t(ptr), _t(idx), query_row=_t(perm))
    assert torch.equal(rank_p, rank)
    # no mask
    rank2, _ = hip_ops.rank_eval_rows(_t(Q), _t(I), _t(et))
    ok2 = margin_nomask > 1e-4
    assert np.array_equal(rank2.cpu().numpy()[ok2], ref_nomask[ok2])
    # every item masked: nothing beats the target, all ranks are 1
    full_ptr = np.arange(0, (n_mask + 1) * n_items, n_items, dtype=np.int64)
    full_idx = np.tile(np.arange(n_items, dtype=np.int32), n_mask)
    rank3, _ = hip_ops.rank_eval_rows(_t(Q), _t(I), _t(et), _t(mrow), _t(full_ptr), _t(full_idx))
    assert int(rank3.min()) == 1 and int(rank3.max()) == 1
    it, sc = hip_ops.topk_recommend_rows(_t(Q), _t(I), 5, _t(mrow), _t(full_ptr), _t(full_idx))
    assert bool((it == -1).all()) and bool(torch.isneginf(sc).all())


# ------------------------------------------------------------------------------------------------ 3./4. the runner
def _launch_argv(path, tmp, extra):
    return ["--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--dropout", "0.0", "--history_max", "20",
            "--model_name", "SASRec", "--runner_name", "HipRunner", "--dataset", "ml-100k", "--path", path, "--epoch", "1",
            "--batch_size", "1024", "--eval_batch_size", "512", "--optimizer", "Adam", "--lr", "1e-3", "--l2", "0.0",
            "--log_file", str(tmp / "log.txt"), "--model_path", str(tmp / "m.pt"), "--num_workers", "0", "--topk", "5,10,20",
            "--metric", "NDCG, HR", "--random_seed", "3407"] + extra


@pytest.fixture(scope="module", params=[0, 1], ids=["block_native0", "block_native1"])
def sasrec(request, tmp_path_factory):
    """SASRec on the ml-100k reader fixture, embeddings scaled up so that scores spread; the host path's score matrix of the
    dev and test rows (BaseRunner.interface: full_predict, clicked items at -inf) is computed once"""
    from test_reader import _write_inter
    from whisprrec_amd import main as launcher, runner
    tmp = tmp_path_factory.mktemp("seq_eval")
    g8 = np.load(os.path.join(os.path.dirname(__file__), "golden", "g8_reader.npz"))
    path = _write_inter(g8, tmp)
    args, model_class, reader_class, runner_class = launcher.build_args(
        _launch_argv(path, tmp, ["--block_native", str(request.param), "--seq_eval_native", "1"]))
    launcher.init_seed(args.random_seed)
    args.device = torch.device("cuda")
    corpus = reader_class(args).corpus()
    model = model_class(args, corpus).to(args.device)
    with torch.no_grad():
        model.item_embedding.weight.mul_(30)
        model.position_embedding.weight.mul_(30)
    data = {ph: model_class.Dataset(model, corpus, ph) for ph in ("dev", "test")}
    host = runner.BaseRunner(args)
    pred = {ph: host.interface(data[ph]).astype(np.float64) for ph in data}
    if request.param:
        assert model._block_native_ok and all(model._block_native_ok.values()), "the block kernels refused the test's shape"
    return {"args": args, "corpus": corpus, "model": model, "data": data, "host": host, "pred": pred, "run": runner_class(args),
            "tmp": tmp}


@pytest.mark.parametrize("phase", ["dev", "test"])
def test_runner_ranks_and_metrics_match_the_host_path(sasrec, phase, monkeypatch):
    from whisprrec_amd import runner
    ds, pred, run = sasrec["data"][phase], sasrec["pred"][phase], sasrec["run"]
    n_eval = len(ds)
    order = (-pred).argsort(axis=1)
    host_rank = np.argwhere(order == 0)[:, 1] + 1                      # evaluate_method
    target, S = pred[:, 0], pred[:, 1:].copy()
    S[np.arange(n_eval), np.asarray(ds.data["item_id"])] = np.nan      # the target's own column
    fin = np.isfinite(S)
    margin = np.where(fin, np.abs(S - target[:, None]), np.inf).min(axis=1)
    ok = margin > 1e-5 * np.abs(S[fin]).max()
    monkeypatch.setattr(runner.BaseRunner, "interface", lambda *a: pytest.fail("the host path ran"))
    assert run._seq_eval_ok(ds)
    before = torch.get_rng_state()
    rank = run.rank_rows(ds)
    after = torch.get_rng_state()
    torch.set_rng_state(before)
    runner.consume_loader_seed()                                       # exactly the draw of one DataLoader iterator
    assert torch.equal(torch.get_rng_state(), after)
    assert rank.dtype == np.int64 and rank.shape == (n_eval,)
    print("seq eval runner %s: n_eval %d, rows kept %.4f, ranks differing on kept rows %d, on all rows %d"
          % (phase, n_eval, ok.mean(), int((rank[ok] != host_rank[ok]).sum()), int((rank != host_rank).sum())))
    assert ok.mean() >= 0.9
    assert np.array_equal(rank[ok], host_rank[ok])
    topk, metrics = [5, 10, 20], ["NDCG", "HR"]
    dev_res = run.evaluate(ds, topk, metrics)
    host_res = runner.BaseRunner.metrics_from_ranks(host_rank, topk, metrics)
    bound = (~ok).sum() / n_eval                                       # one moved rank moves HR@k or NDCG@k by at most 1 / n_eval
    for key in host_res:
        assert abs(host_res[key] - dev_res[key]) <= bound, (key, host_res[key], dev_res[key], bound)
    # train, dev and test keep their own history arrays
    assert len(run._hist_cache) >= 1 and run._history_columns(ds, DEV)[0].shape[0] == n_eval


def test_recommend_rows_next_and_rec_file_match_the_host_topk(sasrec):
    k = 20
    ds, run, model, corpus = sasrec["data"]["dev"], sasrec["run"], sasrec["model"], sasrec["corpus"]
    S = sasrec["pred"]["dev"][:, 1:]
    items, scores = run.recommend_rows(ds, k)
    assert items.dtype == np.int64 and scores.dtype == np.float32 and items.shape == (len(ds), k)
    h_items = np.argsort(-S, axis=1, kind="stable")[:, :k]
    h_sc = np.take_along_axis(S, h_items, axis=1)
    tol = 1e-5 * np.abs(h_sc).max()
    np.testing.assert_allclose(scores, h_sc, rtol=1e-5, atol=tol)
    # every row: the returned items are a top-k of the host scores (up to the rounding of the two GEMMs)
    np.testing.assert_allclose(np.take_along_axis(S, items, axis=1), h_sc, rtol=1e-5, atol=tol)
    # rows outside near-ties (consecutive scores at positions 1..k+1 at least 2 tol apart): the same list
    top = -np.sort(-S, axis=1)[:, :k + 1]
    ok = (-np.diff(top, axis=1)).min(axis=1) >= 2 * tol
    print("seq eval recommend_rows: rows kept %.4f" % ok.mean())
    assert ok.mean() >= 0.5, ok.mean()
    assert np.array_equal(items[ok], h_items[ok])
    users = np.asarray(ds.data["user_id"])
    for r in range(0, len(ds), 97):                                     # a clicked item is never recommended
        clicked = corpus.train_clicked_set.get(users[r], set()) | corpus.residual_clicked_set.get(users[r], set())
        assert not (set(items[r].tolist()) & clicked)
    # a subset of the rows, in the order asked for
    sub = np.array([len(ds) - 1, 3, 3, 700, 0])
    sub_items, sub_scores = run.recommend_rows(ds, k, rows=sub)
    positions = np.asarray(ds.data["position"])
    sub_his = [[x[0] for x in corpus.user_his[users[r]][:positions[r]]] for r in sub]
    nx_items, nx_scores = run.recommend_next(model, corpus, sub_his, k, users=users[sub])   # the same five rows, given directly
    assert np.array_equal(sub_items, nx_items) and np.array_equal(sub_scores.view(np.int32), nx_scores.view(np.int32))
    if not model.block_native:
        # On torch ops a query does not depend on the batch it is computed in.  The block kernels shift the attention scores
        # by the maximum of the whole batch as the reference writes it (layers.py:54), and with embeddings scaled by 30 a
        # row far below another batch's maximum underflows there: its bits belong to its batch.
        assert np.array_equal(sub_items, items[sub]) and np.array_equal(sub_scores.view(np.int32), scores[sub].view(np.int32))
    none_items, _ = run.recommend_rows(ds, 5, rows=[0, 1], exclude="none")
    tr_items, _ = run.recommend_rows(ds, 5, rows=[0, 1], exclude="train")
    assert none_items.shape == (2, 5) and not (set(tr_items[0].tolist()) & corpus.train_clicked_set[users[0]])
    with pytest.raises(ValueError):
        run.recommend_rows(ds, 5, exclude="bogus")
    with pytest.raises(IndexError):
        run.recommend_rows(ds, 5, rows=[len(ds)])
    # the same histories given directly (uncut: recommend_next keeps the last history_max items)
    histories = [[x[0] for x in corpus.user_his[u][:p]] for u, p in zip(users.tolist(), np.asarray(ds.data["position"]).tolist())]
    nx_items, nx_scores = run.recommend_next(model, corpus, histories, k, users=users)
    assert np.array_equal(nx_items, items)
    free_items, _ = run.recommend_next(model, corpus, histories, k)                      # no users: no mask
    assert np.array_equal(free_items, run.recommend_rows(ds, k, exclude="none")[0])
    with pytest.raises(ValueError):
        run.recommend_next(model, corpus, [[]], k)
    with pytest.raises(IndexError):
        run.recommend_next(model, corpus, [[1, model.item_num]], k)
    # recommend() is per user: for a model with one query per row it names the method to use
    with pytest.raises(NotImplementedError, match="recommend_rows"):
        run.recommend(model, corpus, users[:4], k)
    # save_rec_results: one line per dev row, in order, that parses back to those lists
    path = run.save_rec_results(ds, k, str(sasrec["tmp"] / "rec-SASRec.csv"), sep="\t")
    with open(path, newline="") as f:
        rows = list(csv.reader(f, delimiter="\t"))
    assert rows[0] == ["user_id", "rec_items"] and len(rows) == 1 + len(ds)
    for r, (row, u) in enumerate(zip(rows[1:], users)):
        assert int(row[0]) == u and eval(row[1]) == items[r].tolist()


def test_flag_on_a_factor_model_warns_once_and_changes_nothing(g2, caplog):
    import argparse
    import logging
    from test_host_contract import ml100k_corpus, seed_all
    from whisprrec_amd import runner
    from whisprrec_amd.bprmf import BPRMF
    base = dict(device=DEV, model_path="/tmp/wr_seq_eval_model.pt", buffer=1, num_neg=1, test_all=1, embedding_size=64, fused=1,
                epoch=1, check_epoch=1, test_epoch=-1, early_stop=10, lr=1e-3, l2=0.0, batch_size=2048, eval_batch_size=512,
                optimizer="SGD", num_workers=0, pin_memory=0, topk="5,10,20", metric="NDCG, HR", device_epoch_prep=0,
                random_seed=3407)
    seed_all(7)
    corpus = ml100k_corpus(g2)
    rng = np.random.RandomState(3)
    dev_u, dev_i = rng.randint(0, 943, 300), rng.randint(0, 1574, 300)
    corpus.data_df["dev"] = {"user_id": dev_u, "item_id": dev_i}
    for a, b in zip(dev_u.tolist(), dev_i.tolist()):
        corpus.residual_clicked_set[a].add(b)
    model = BPRMF(argparse.Namespace(**base), corpus).to(DEV)
    ds = BPRMF.Dataset(model, corpus, "dev")
    plain = runner.HipRunner(argparse.Namespace(**base)).evaluate(ds, [10], ["NDCG", "HR"])
    flagged = runner.HipRunner(argparse.Namespace(seq_eval_native=1, **base))
    with caplog.at_level(logging.WARNING):
        a = flagged.evaluate(ds, [10], ["NDCG", "HR"])
        b = flagged.evaluate(ds, [10], ["NDCG", "HR"])
    assert a == plain and b == plain
    assert sum("seq_eval_native" in r.getMessage() for r in caplog.records) == 1


# ------------------------------------------------------------------------------------------------ 5. end to end
def test_end_to_end_run_with_device_evaluation_matches_the_reference(tmp_path, monkeypatch):
    """the ("sasrec", "HipRunner") case of tests/test_reader.py::test_end_to_end_run_matches_the_reference_train_loop with
    --seq_eval_native 1, under that test's bounds.  The losses of epochs >= 2 match only if every evaluation leaves torch's
    global generator where the reference's evaluation DataLoader leaves it."""
    from test_reader import _write_inter
    from whisprrec_amd import main as launcher, runner
    gold = os.path.join(os.path.dirname(__file__), "golden")
    g8, g9 = np.load(os.path.join(gold, "g8_reader.npz")), np.load(os.path.join(gold, "g9_end_to_end.npz"))
    path = _write_inter(g8, tmp_path)
    tag = "sasrec"
    lr, l2, epochs = g9[tag + "_hp"]
    argv = ["--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--dropout", "0.0", "--history_max", "20",
            "--seq_eval_native", "1", "--model_name", "SASRec", "--runner_name", "HipRunner", "--dataset", "ml-100k", "--path", path,
            "--epoch", str(int(epochs)), "--batch_size", "1024", "--eval_batch_size", "2048", "--optimizer", "Adam",
            "--lr", repr(float(lr)), "--l2", repr(float(l2)), "--log_file", str(tmp_path / "log.txt"),
            "--model_path", str(tmp_path / "m.pt"), "--num_workers", "0", "--topk", "10,20", "--metric", "NDCG, HR",
            "--random_seed", "3407"]
    args, model_class, reader_class, runner_class = launcher.build_args(argv)
    assert args.seq_eval_native == 1
    launcher.init_seed(args.random_seed)
    args.device = torch.device("cuda")
    corpus = reader_class(args).corpus()
    model = model_class(args, corpus).to(args.device)
    data = {ph: model_class.Dataset(model, corpus, ph) for ph in ("train", "dev", "test")}
    run = runner_class(args)
    monkeypatch.setattr(runner.BaseRunner, "interface", lambda *a: pytest.fail("the host evaluation ran"))
    losses, devs = [], []
    for epoch in range(args.epoch):
        losses.append(run.fit(data["train"], epoch=epoch + 1))
        devs.append(run.evaluate(data["dev"], run.topk[:1], run.metrics))
    test = run.evaluate(data["test"], run.topk, run.metrics)
    assert len(run._hist_cache) == 3                                   # train, dev and test: nobody evicted anybody
    print("seq eval g9: loss rel %.2e" % np.max(np.abs(np.asarray(losses) / g9[tag + "_loss"] - 1.0)))
    assert np.allclose(losses, g9[tag + "_loss"], rtol=5e-5, atol=0)
    n_eval = len(data["dev"])
    flips = 6.0 / n_eval                              # a handful of near-tied ranks may fall on the other side of the cut
    dev = np.asarray([[d[k] for k in g9[tag + "_dev_keys"]] for d in devs])
    assert np.abs(dev - g9[tag + "_dev"]).max() <= flips, np.abs(dev - g9[tag + "_dev"]).max()
    tst = np.asarray([test[k] for k in g9[tag + "_test_keys"]])
    assert np.abs(tst - g9[tag + "_test"]).max() <= flips
