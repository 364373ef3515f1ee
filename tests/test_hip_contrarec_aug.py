"""GPU checks of ContraRec's device view builder (--aug_native 1): wr_seq_augment is bit-equal to its NumPy restatement
(contrarec_aug_ref) over lengths 1..T, unsorted row ids with repeats, four Beta parameter pairs, two epochs and two seeds; a row's
views do not depend on the call they are drawn in; bad lengths and row ids are flagged and contained; and ContraRec trains through
HipRunner.fit's batch loop with the views of exactly its batches' dataset rows."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrarec_aug_ref as A  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TOKEN, N_TABLE = 900, 1000
BETAS = ((3, 3), (1, 1), (1, 5), (8, 8))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _table(T, seed=0):
    """1,000 histories whose lengths cycle through 1..T"""
    rng = np.random.RandomState(100 + T + seed)
    lens = (np.arange(N_TABLE) % T + 1).astype(np.int64)
    hist = np.where(np.arange(T)[None, :] < lens[:, None], rng.randint(1, TOKEN, size=(N_TABLE, T)), 0).astype(np.int64)
    return hist, lens


def _views(hist, lens, rows, a, b, seed, epoch, err=None):
    from whisprrec_amd import hip_ops
    va, vb = hip_ops.seq_augment(_t(hist), _t(lens), _t(rows), TOKEN, a, b, seed, epoch, err_word=err)
    return va.cpu().numpy(), vb.cpu().numpy()


@pytest.mark.parametrize("T,B", [(1, 1), (2, 5), (20, 257), (50, 64), (64, 3)])
def test_kernel_is_bit_equal_to_the_restatement(T, B):
    hist, lens = _table(T)
    rows = np.random.RandomState(B).randint(0, N_TABLE, size=B).astype(np.int64)
    if B > 1:
        rows[-1] = rows[0]                                                       # a repeat, whatever the draw
    if B >= 8 * T:
        assert set(lens[rows].tolist()) == set(range(1, T + 1))                  # the batch itself meets every length
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    for a, b in BETAS:
        for epoch in (1, 2):
            for seed in (3407, 2 ** 63 + 5):
                got = _views(hist, lens, rows, a, b, seed, epoch, err)
                want = A.seq_augment(hist, lens, rows, TOKEN, a, b, seed, epoch)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (a, b, epoch, seed)
                if B > 1:
                    assert np.array_equal(got[0][-1], got[0][0]) and np.array_equal(got[1][-1], got[1][0])
    assert int(err.item()) == 0


def test_calls_repeat_their_bits_and_split_batches_concatenate():
    hist, lens = _table(20)
    rows = np.random.RandomState(1).randint(0, N_TABLE, size=257).astype(np.int64)
    one = _views(hist, lens, rows, 3, 3, 3407, 1)
    again = _views(hist, lens, rows, 3, 3, 3407, 1)
    head, tail = _views(hist, lens, rows[:200], 3, 3, 3407, 1), _views(hist, lens, rows[200:], 3, 3, 3407, 1)
    for v in (0, 1):
        assert np.array_equal(one[v], again[v])
        assert np.array_equal(one[v], np.concatenate([head[v], tail[v]]))
    assert not np.array_equal(one[0], _views(hist, lens, rows, 3, 3, 3407, 2)[0])
    assert not np.array_equal(one[0], _views(hist, lens, rows, 3, 3, 3408, 1)[0])
    assert not np.array_equal(one[0], one[1])


def test_bad_lengths_and_row_ids_set_their_bits_and_stay_contained():
    T = 20
    hist, lens = _table(T)
    rows = np.arange(40, 70, dtype=np.int64)
    clean = _views(hist, lens, rows, 3, 3, 3407, 1)
    for bad_len, bad_row, bit in ((0, None, 1), (T + 1, None, 1), (None, N_TABLE, 2), (None, -1, 2)):
        lens2, rows2 = lens.copy(), rows.copy()
        if bad_len is not None:
            lens2[rows[7]] = bad_len
        else:
            rows2[7] = bad_row
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = _views(hist, lens2, rows2, 3, 3, 3407, 1, err)
        want = A.seq_augment(hist, lens2, rows2, TOKEN, 3, 3, 3407, 1)
        assert int(err.item()) == bit == want[2]
        keep = np.arange(rows.size) != 7
        for v in (0, 1):
            assert np.array_equal(got[v], want[v])
            assert np.array_equal(got[v][keep], clean[v][keep])                   # no other row changes
            if bad_row is not None:
                assert not got[v][7].any()
            elif bad_len == 0:
                assert not got[v][7][1:].any()                                    # clamped to one item
    from whisprrec_amd import hip_ops
    assert hip_ops.seq_augment_supports(64, 8, 8) and not hip_ops.seq_augment_supports(65, 3, 3)
    with pytest.raises(Exception):
        hip_ops.seq_augment(_t(np.zeros((4, 65), np.int64)), _t(np.ones(4, np.int64)), _t(np.arange(4)), TOKEN, 3, 3, 1, 1)


# ------------------------------------------------------------------------------------------------ end to end
def _corpus():
    """a few hundred training rows: 48 users with 2 .. 30 items each in time order (every position > 0 is a training row)"""
    from whisprrec_amd import host
    rng = np.random.RandomState(11)
    n_users, n_items = 49, 200
    his, frame, clicked = {}, {"user_id": [], "item_id": [], "position": []}, {}
    for u in range(1, n_users):
        items = (rng.permutation(n_items - 1)[:rng.randint(2, 31)] + 1).tolist()
        his[u] = [(it, t) for t, it in enumerate(items)]
        clicked[u] = set(items)
        for q, it in enumerate(items):
            frame["user_id"].append(u); frame["item_id"].append(it); frame["position"].append(q)
    train = {k: np.asarray(v, np.int64) for k, v in frame.items()}
    empty = {k: np.zeros(0, np.int64) for k in frame}
    corpus = host.Corpus(n_users, n_items, {"train": train, "dev": empty, "test": empty}, clicked, {u: set() for u in clicked})
    corpus.user_his = his
    return corpus


def _setup(extra):
    from whisprrec_amd import main as launcher
    argv = ["--model_name", "ContraRec", "--runner_name", "HipRunner", "--batch_size", "64", "--lr", "1e-3", "--l2", "0.0",
            "--emb_size", "64", "--history_max", "20", "--num_workers", "0", "--random_seed", "2024", "--block_native", "1",
            "--ccc_native", "1", "--model_path", "/tmp/wr_contrarec_aug_gpu.pt", "--log_file", "/tmp/wr_contrarec_aug_gpu.txt"] + extra
    args, model_class, _, runner_class = launcher.build_args(argv)
    launcher.init_seed(args.random_seed)
    args.device = DEV
    corpus = _corpus()
    model = model_class(args, corpus).to(DEV)
    return args, model, model_class.Dataset(model, corpus, "train"), runner_class(args)


@pytest.mark.parametrize("prep", [0, 1])
def test_contrarec_trains_through_the_batch_loop_with_the_views_of_its_rows(prep, monkeypatch):
    from whisprrec_amd import runner
    args, model, data, run = _setup(["--aug_native", "1", "--device_epoch_prep", str(prep)])
    assert model.per_sample_feed is False

    def loader_loop(self, dataset, epoch=-1):
        raise AssertionError("the DataLoader loop was entered")

    monkeypatch.setattr(runner.BaseRunner, "fit", loader_loop)
    seen = []
    predict = model.predict

    def spy(batch):
        seen.append({k: v.clone() for k, v in batch.items() if isinstance(v, torch.Tensor)})
        return predict(batch)

    model.predict = spy
    hist_all, len_all = (t.cpu().numpy() for t in run._history_columns(data, DEV))
    data.actions_before_epoch()                                                   # a training feed dict reads its negative
    for i in (0, 17, len(data) - 1):                                              # the table is the per-sample feed's history
        fd = data[i]
        assert fd["lengths"] == len_all[i] and np.array_equal(fd["history_items"], hist_all[i, :len_all[i]])
    assert 200 <= len(data) <= 1000 and len_all.min() == 1 and len_all.max() == 20 and hist_all.shape[1] == 20
    losses, B = [], 64
    for epoch in (1, 2):
        del seen[:]
        losses.append(run.fit(data, epoch=epoch))
        order = run._last_order.cpu().numpy()
        assert np.array_equal(np.sort(order), np.arange(len(data))) and len(seen) == -(-len(data) // B)
        for k, batch in enumerate(seen):
            rows = order[k * B:(k + 1) * B]
            got = {name: t.cpu().numpy() for name, t in batch.items()}
            want_a, want_b, err = A.seq_augment(hist_all, len_all, rows, model.mask_token, 3, 3, 2024, epoch)
            assert err == 0
            assert np.array_equal(got["history_items_a"], want_a) and np.array_equal(got["history_items_b"], want_b), (epoch, k)
            assert np.array_equal(got["history_items"], hist_all[rows]) and np.array_equal(got["lengths"], len_all[rows])
            assert np.array_equal(got["pos_item"], data.data["item_id"][rows])
            assert np.array_equal(got["user_id"], data.data["user_id"][rows])
            neg = got["neg_items"].reshape(-1)
            if prep == 0:                                                         # the dataset's own draw, sliced by the shuffle
                assert np.array_equal(neg, np.asarray(data.data["neg_items"]).reshape(-1)[rows])
            else:
                assert np.array_equal(neg, run._epoch_prep.cols[2].cpu().numpy()[k * B:(k + 1) * B])
                assert all(1 <= x < 200 and x not in data.corpus.train_clicked_set[u] for x, u in zip(neg.tolist(), got["user_id"].tolist()))
        assert (np.concatenate([b["history_items_a"].cpu().numpy() for b in seen]) == model.mask_token).any()
    model.check_key_lengths()
    model.check_train_extras()
    assert all(model._block_native_ok.values()) and all(model._ccc_native_ok.values())
    assert np.isfinite(losses).all() and losses[0] != losses[1]


def test_flag_off_keeps_the_loader_loop(monkeypatch):
    from whisprrec_amd import runner
    args, model, data, run = _setup([])
    assert model.per_sample_feed is True
    monkeypatch.setattr(runner.BaseRunner, "fit", lambda self, dataset, epoch=-1: "loader loop")
    assert run.fit(data, epoch=1) == "loader loop"


def test_error_word_of_the_hook_is_read_once_per_epoch():
    args, model, data, run = _setup(["--aug_native", "1"])
    hist_all, len_all = run._history_columns(data, DEV)
    model.set_history_table(hist_all, len_all)
    model.train_batch_extras({}, torch.tensor([0, len(data)], device=DEV), 1)
    with pytest.raises(IndexError, match="row id outside"):
        model.check_train_extras()
    model.check_train_extras()                                                    # cleared by the read
