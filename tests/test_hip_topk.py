"""Top-K recommendation on the device (K11, wr_topk_recommend) against a float64 NumPy restatement of the reference's
sort of full_predict with -inf masking (src/main.py:83-102), against wr_rank_eval bit for bit, and through HipRunner /
the launcher."""
import argparse
import csv
import os

import numpy as np
import pytest
import torch

from whisprrec_amd import hip_ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _tables(D, n_users, n_items, seed, grid=False, std=10.0):
    """Gaussian tables whose scores have standard deviation `std`; grid=True: multiples of 1/8 in [-1, 1], so every fp32
    score is exact (and exact ties are frequent)"""
    rng = np.random.RandomState(seed)
    if grid:
        U = rng.randint(-8, 9, (n_users, D)) / 8.0
        I = rng.randint(-8, 9, (n_items, D)) / 8.0
    else:
        s = np.sqrt(std / np.sqrt(D))
        U, I = rng.standard_normal((n_users, D)) * s, rng.standard_normal((n_items, D)) * s
    return U.astype(np.float32), I.astype(np.float32)


def _random_mask(rng, n_users, n_items, frac):
    sets = {u: set(np.flatnonzero(rng.random_sample(n_items) < frac).tolist()) for u in range(n_users)}
    return sets, hip_ops.clicked_csr(sets, n_users, DEV)


def _reference(U, I, users, k, sets=None):
    """float64 scores, masked items at -inf, stable descending sort (ties by ascending item id); masked slots -> -1"""
    S = U[users].astype(np.float64) @ I.astype(np.float64).T
    if sets is not None:
        for r, u in enumerate(users):
            if sets[u]:
                S[r, list(sets[u])] = -np.inf
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
    sc = np.take_along_axis(S, order, axis=1)
    items = np.where(np.isfinite(sc), order, -1)
    if k > S.shape[1]:
        pad = k - S.shape[1]
        items = np.concatenate([items, -np.ones((len(users), pad), np.int64)], axis=1)
        sc = np.concatenate([sc, np.full((len(users), pad), -np.inf)], axis=1)
    return items, sc, S


def _run(U, I, users, k, mask=None):
    Ud, Id = torch.from_numpy(U).to(DEV), torch.from_numpy(I).to(DEV)
    q = torch.from_numpy(np.asarray(users, np.int64)).to(DEV)
    ptr, idx = mask if mask is not None else (None, None)
    items, scores = hip_ops.topk_recommend(Ud, Id, q, k, ptr, idx)
    torch.cuda.synchronize()
    return items.cpu().numpy(), scores.cpu().numpy()


def _check_padding_and_mask(items, scores, users, sets, n_items):
    assert items.dtype == np.int64 and scores.dtype == np.float32
    pad = items == -1
    assert np.all(np.isneginf(scores[pad])) and np.all(np.isfinite(scores[~pad]))
    assert np.all((items[~pad] >= 0) & (items[~pad] < n_items))
    # pads only at the end, no repeated item in a row
    for r in range(items.shape[0]):
        p = np.flatnonzero(pad[r])
        assert p.size == 0 or p[0] == items.shape[1] - p.size
        real = items[r][~pad[r]]
        assert len(set(real.tolist())) == real.size
        if sets is not None:
            assert not (set(real.tolist()) & sets[users[r]]), "a masked item was returned"


CASES = [  # D, n_items, k, masked, grid
    (8, 40, 100, False, False), (8, 40, 10, True, False), (16, 777, 10, True, False), (32, 5000, 100, False, True), (32, 777, 100, False, False),
    (64, 70000, 10, True, False), (64, 70000, 1, False, False), (64, 5000, 100, True, True), (64, 777, 100, True, False), (64, 777, 256, True, True),
    (64, 70000, 100, True, True), (64, 5000, 256, False, True), (24, 70000, 1, False, False), (24, 777, 256, True, True),
    (24, 5000, 10, True, False), (128, 5000, 10, True, False), (128, 70000, 10, False, False), (252, 5000, 100, False, True), (252, 777, 100, False, False),
    (252, 777, 256, True, True), (252, 40, 1, True, False), (16, 70000, 256, True, True), (32, 777, 1, True, False),
]


@pytest.mark.parametrize("D,n_items,k,masked,grid", CASES)
def test_matches_float64_restatement(D, n_items, k, masked, grid):
    n_users = 300
    U, I = _tables(D, n_users, n_items, seed=D * 7 + n_items + k, grid=grid)
    rng = np.random.RandomState(k + 1)
    users = rng.randint(0, n_users, 200)
    sets, mask = _random_mask(rng, n_users, n_items, 0.1) if masked else (None, None)
    items, scores = _run(U, I, users, k, mask)
    ref_items, ref_sc, _ = _reference(U, I, users, k, sets)
    _check_padding_and_mask(items, scores, users, sets, n_items)
    fin = np.isfinite(ref_sc)
    assert np.array_equal(np.isfinite(scores), fin)
    np.testing.assert_allclose(scores[fin], ref_sc[fin], rtol=1e-5, atol=1e-5 * np.abs(ref_sc[fin]).max())
    if grid:                 # exact fp32 scores: every row, ties included, equals the stable sort
        assert np.array_equal(items, ref_items)
        return
    # rows whose reference scores at positions 1..k+1 are at least 1e-4 apart must match exactly
    _, _, S = _reference(U, I, users, min(k + 1, n_items), sets)
    top = -np.sort(-S, axis=1)[:, :k + 1]
    gaps = -np.diff(np.where(np.isfinite(top), top, -1e30), axis=1)
    ok = gaps.min(axis=1) >= 1e-4 if top.shape[1] > 1 else np.ones(len(users), bool)
    assert ok.mean() >= 0.9, ok.mean()
    assert np.array_equal(items[ok], ref_items[ok])


@pytest.mark.parametrize("D,n_items,k", [(64, 5000, 100), (64, 70000, 20), (24, 3000, 50), (128, 2000, 256)])
def test_scores_and_ranks_agree_with_rank_eval(D, n_items, k):
    """no tolerance: rank_eval on (user, returned item) gives the returned score bit for bit, and the rank the full
    score set implies"""
    n_users = 200
    U, I = _tables(D, n_users, n_items, seed=11 + D)
    rng = np.random.RandomState(5)
    users = rng.randint(0, n_users, 150)
    sets, (ptr, idx) = _random_mask(rng, n_users, n_items, 0.05)
    items, scores = _run(U, I, users, k, (ptr, idx))
    Ud, Id = torch.from_numpy(U).to(DEV), torch.from_numpy(I).to(DEV)
    valid = items >= 0
    eu = np.repeat(users, k).reshape(len(users), k)[valid]
    et = items[valid]
    rank, tsc = hip_ops.rank_eval(Ud, Id, torch.from_numpy(eu).to(DEV), torch.from_numpy(et).to(DEV), ptr, idx)
    rank, tsc = rank.cpu().numpy(), tsc.cpu().numpy()
    assert np.array_equal(tsc.view(np.int32), scores[valid].view(np.int32)), "scores differ from rank_eval's target_score"
    # rank = 1 + #{unmasked s in the row : s > score}, from the row's full fp32 score set (rank_eval over all items)
    n_all = len(users) * n_items
    au = np.repeat(users, n_items)
    ai = np.tile(np.arange(n_items), len(users))
    _, full = hip_ops.rank_eval(Ud, Id, torch.from_numpy(au).to(DEV), torch.from_numpy(ai).to(DEV), ptr, idx)
    full = full.cpu().numpy().reshape(len(users), n_items).astype(np.float64)
    for r, u in enumerate(users):
        full[r, list(sets[u])] = -np.inf
    expect = np.stack([1 + (full[r][None, :] > scores[r][:, None].astype(np.float64)).sum(axis=1)
                       for r in range(len(users))])
    assert np.array_equal(rank, expect[valid])
    assert n_all == full.size
    # untied rows: the r-th item has rank r + 1
    ties = np.array([len(np.unique(full[r][np.isfinite(full[r])])) < np.isfinite(full[r]).sum() for r in range(len(users))])
    pos = np.tile(np.arange(1, k + 1), (len(users), 1))
    assert np.array_equal(rank[(~ties[:, None] & valid)[valid]], pos[~ties[:, None] & valid])
    # evaluation rows: #recommended scores strictly above the target's = min(rank - 1, k)
    targets = rng.randint(0, n_items, len(users))
    rk, ts = hip_ops.rank_eval(Ud, Id, torch.from_numpy(users).to(DEV), torch.from_numpy(targets).to(DEV), ptr, idx)
    rk, ts = rk.cpu().numpy(), ts.cpu().numpy()
    above = (scores > ts[:, None]).sum(axis=1)
    assert np.array_equal(above, np.minimum(rk - 1, k))


def test_ties_order_by_item_id():
    D, n_items, k = 64, 3000, 100
    rng = np.random.RandomState(2)
    base = (rng.standard_normal((7, D)) * 0.3).astype(np.float32)
    I = base[np.arange(n_items) % 7]                                  # I[j] = I[j % 7]: every score ties bitwise
    U = (rng.standard_normal((50, D)) * 0.3).astype(np.float32)
    users = np.arange(50)
    items, scores = _run(U, I, users, k)
    for r in range(len(users)):
        s = scores[r]
        assert np.all(s[:-1] >= s[1:])
        same = s[:-1] == s[1:]
        assert np.all(items[r][:-1][same] < items[r][1:][same])
    ref_items, _, _ = _reference(U, I, users, k)
    assert np.array_equal(items, ref_items)


def test_zero_user_row_returns_first_unmasked_ids():
    D, n_items, k = 32, 1000, 20
    U, I = _tables(D, 4, n_items, seed=3)
    U[1] = 0.0
    sets = {0: set(), 1: {0, 2, 5, 6}, 2: set(), 3: set()}
    mask = hip_ops.clicked_csr(sets, 4, DEV)
    items, scores = _run(U, I, [1, 1], k, mask)
    expect = [j for j in range(n_items) if j not in sets[1]][:k]
    assert items[0].tolist() == expect and items[1].tolist() == expect
    assert np.all(scores == 0.0)


@pytest.mark.parametrize("D", [64, 24])
def test_masking_and_padding(D):
    n_items, k = 500, 10
    U, I = _tables(D, 3, n_items, seed=4)
    keep = [17, 250, 499]
    sets = {0: set(range(n_items)), 1: set(range(n_items)) - set(keep), 2: set()}
    mask = hip_ops.clicked_csr(sets, 3, DEV)
    items, scores = _run(U, I, [0, 1, 2], k, mask)
    assert np.all(items[0] == -1) and np.all(np.isneginf(scores[0]))
    assert sorted(items[1][:3].tolist()) == keep and np.all(items[1][3:] == -1) and np.all(np.isneginf(scores[1][3:]))
    S = U[1].astype(np.float64) @ I[keep].astype(np.float64).T
    assert items[1][:3].tolist() == [keep[i] for i in np.argsort(-S, kind="stable")]
    assert np.all(items[2] >= 0)


def test_deterministic_and_repeated_users_agree():
    D, n_items, k = 64, 70000, 100
    U, I = _tables(D, 100, n_items, seed=9)
    rng = np.random.RandomState(1)
    sets, mask = _random_mask(rng, 100, n_items, 0.02)
    users = np.concatenate([np.arange(100), np.arange(100)[::-1], [5] * 40])
    a_items, a_sc = _run(U, I, users, k, mask)
    b_items, b_sc = _run(U, I, users, k, mask)
    assert np.array_equal(a_items, b_items) and np.array_equal(a_sc.view(np.int32), b_sc.view(np.int32))
    for r, u in enumerate(users):
        assert np.array_equal(a_items[r], a_items[u]) and np.array_equal(a_sc[r].view(np.int32), a_sc[u].view(np.int32))


# ------------------------------------------------------------------------------------------------ runner and launcher
def _runner_args(dev, **kw):
    base = dict(device=dev, model_path="/tmp/wr_topk_model.pt", buffer=1, num_neg=1, test_all=1, embedding_size=64, fused=1,
                epoch=1, check_epoch=1, test_epoch=-1, early_stop=10, lr=1e-3, l2=0.0, batch_size=2048, eval_batch_size=512,
                optimizer="SGD", num_workers=0, pin_memory=0, topk="5,10,20", metric="NDCG, HR", device_epoch_prep=0,
                random_seed=3407, n_layers=2, gcn_layers=2, emb_size=64)
    base.update(kw)
    return argparse.Namespace(**base)


def _host_topk(model, corpus, users, k):
    """full_predict, the user's train + dev + test items at -inf, stable descending argsort"""
    with torch.no_grad():
        s = model.full_predict({"user_id": torch.from_numpy(users).to(DEV),
                                "pos_item": torch.zeros(len(users), dtype=torch.int64, device=DEV)})
    S = s.double().cpu().numpy()
    for r, u in enumerate(users):
        clicked = corpus.train_clicked_set.get(u, set()) | corpus.residual_clicked_set.get(u, set())
        S[r, list(clicked)] = -np.inf
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
    return order, np.take_along_axis(S, order, axis=1), S


def _corpus(g2):
    from test_host_contract import ml100k_corpus, seed_all
    seed_all(7)
    corpus = ml100k_corpus(g2)
    rng = np.random.RandomState(3)
    dev_u = rng.randint(0, 943, 1500)
    dev_i = rng.randint(0, 1574, 1500)
    corpus.data_df["dev"] = {"user_id": dev_u, "item_id": dev_i}
    for a, b in zip(dev_u.tolist(), dev_i.tolist()):
        corpus.residual_clicked_set[a].add(b)
    return corpus


def _compare_with_host(model, corpus, rn, k=20):
    users = np.arange(corpus.n_users)
    items, scores = rn.recommend(model, corpus, users, k)
    h_items, h_sc, S = _host_topk(model, corpus, users, k)
    tol = 1e-5 * np.abs(h_sc).max()
    np.testing.assert_allclose(scores, h_sc, rtol=1e-5, atol=tol)
    # every row: the returned items are a top-k of the host scores (up to the rounding of the two GEMMs)
    np.testing.assert_allclose(np.take_along_axis(S, items, axis=1), h_sc, rtol=1e-5, atol=tol)
    # rows outside near-ties (consecutive scores at positions 1..k+1 at least 2 tol apart): the same list
    top = -np.sort(-S, axis=1)[:, :k + 1]
    ok = (-np.diff(top, axis=1)).min(axis=1) >= 2 * tol
    assert ok.mean() >= 0.5, ok.mean()
    assert np.array_equal(items[ok], h_items[ok])
    return items


def test_runner_recommend_bprmf_matches_host_path(g2, tmp_path):
    from whisprrec_amd import runner
    from whisprrec_amd.bprmf import BPRMF
    corpus = _corpus(g2)
    model = BPRMF(_runner_args(DEV), corpus).to(DEV)
    with torch.no_grad():
        model.user_embeddings.weight.mul_(30); model.item_embeddings.weight.mul_(30)
    rn = runner.HipRunner(_runner_args(DEV))
    items = _compare_with_host(model, corpus, rn)
    # exclude="none" / "train": the masks the docstring names
    none_items, _ = rn.recommend(model, corpus, [0, 1], 5, exclude="none")
    tr_items, _ = rn.recommend(model, corpus, [0, 1], 5, exclude="train")
    assert not (set(tr_items[0].tolist()) & corpus.train_clicked_set[0])
    assert none_items.shape == (2, 5)
    with pytest.raises(ValueError):
        rn.recommend(model, corpus, [0], 5, exclude="bogus")
    # save_rec_results: one line per dev row, in order, that parses back to those lists
    ds = BPRMF.Dataset(model, corpus, "dev")
    path = rn.save_rec_results(ds, 20, str(tmp_path / "rec-BPRMF.csv"), sep="\t")
    with open(path, newline="") as f:
        rows = list(csv.reader(f, delimiter="\t"))
    assert rows[0] == ["user_id", "rec_items"] and len(rows) == 1 + len(ds.data["user_id"])
    for row, u in zip(rows[1:], ds.data["user_id"]):
        assert int(row[0]) == u and eval(row[1]) == items[u].tolist()


def test_runner_recommend_lightgcn_matches_host_path(g2):
    from whisprrec_amd import runner
    from whisprrec_amd.lightgcn import LightGCN
    corpus = _corpus(g2)
    p = argparse.ArgumentParser()
    LightGCN.parse_model_args(p)
    margs = p.parse_args([])
    for k_, v in vars(_runner_args(DEV)).items():
        if not hasattr(margs, k_):
            setattr(margs, k_, v)
    margs.device = DEV
    model = LightGCN(margs, corpus).to(DEV)
    with torch.no_grad():
        for prm in model.parameters():
            prm.mul_(30)
    _compare_with_host(model, corpus, runner.HipRunner(_runner_args(DEV)))


def test_runner_refuses_models_without_factors():
    from whisprrec_amd import runner

    class NoFactors(torch.nn.Module):
        test_all = 1
    with pytest.raises(NotImplementedError, match="NoFactors"):
        runner.HipRunner(_runner_args(DEV)).recommend(NoFactors(), None, [0], 5)


def test_launcher_writes_rec_file(tmp_path):
    from test_reader import _write_inter
    from whisprrec_amd import main as launcher
    g8 = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "g8_reader.npz")))
    path = _write_inter(g8, tmp_path)
    argv = ["--model_name", "BPRMF", "--dataset", "ml-100k", "--path", path, "--epoch", "1", "--batch_size", "1024",
            "--log_file", str(tmp_path / "log.txt"), "--model_path", str(tmp_path / "m.pt"), "--num_workers", "0",
            "--runner_name", "HipRunner", "--save_rec", "10"]
    launcher.main(argv)
    rec = os.path.join(path, "ml-100k", "rec-BPRMF.csv")
    assert os.path.exists(rec)
    with open(rec, newline="") as f:
        rows = list(csv.reader(f, delimiter="\t"))
    from whisprrec_amd.reader import BaseReader
    r = BaseReader(argparse.Namespace(sep="\t", path=path, dataset="ml-100k", sample="random"))
    assert rows[0] == ["user_id", "rec_items"] and len(rows) == 1 + len(r.data_df["dev"]["user_id"])
    assert all(len(eval(row[1])) == 10 for row in rows[1:])
