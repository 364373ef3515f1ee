"""GPU checks of IF4Rec's native paths: the interest pooling kernels (wr_interest_pool_fwd / _bwd, K18) and the multi-interest
ranking (wr_rank_eval_multi, K19) against the float64 restatements of tests/if4rec_ref.py under its tolerance; then the model
with its flags against its own torch path, on the reference's batch (g14) and over a 2-epoch launcher run on the committed ml-100k
file with the device evaluation.  Figures are printed as `parity ...` lines."""
import gzip
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import if4rec_ref as R  # noqa: E402
import sasblock_ref as S  # noqa: E402
from test_if4rec_contract import _args  # noqa: E402
from whisprrec_amd import host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POOL_KEYS = ("item", "pos", "hist", "W1", "b1", "W2", "b2")


@pytest.fixture(scope="module")
def g14():
    return np.load(os.path.join(GOLD, "g14_if4rec.npz"))


@pytest.fixture(scope="module")
def pool_cases():
    """every case with its float64 reference, computed once"""
    cases = [R.make_case(i) for i in range(len(R.CASES))]
    return [(c, R.pool_ref(c, g_out=c["g_out"])) for c in cases]


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _pool(c, hist=None, err=None):
    """forward + backward of the raw pair -> dict of numpy arrays named as if4rec_ref.FIGURES (g_item by scatter_add_rows)"""
    from whisprrec_amd import hip_ops
    a = [_t(c[k]) for k in POOL_KEYS]
    if hist is not None:
        a[2] = _t(hist)
    out = hip_ops.interest_pool_fwd(*a, err_word=err)
    g_hp, gW1, gb1, gW2, gb2, gpos = hip_ops.interest_pool_bwd(*a, _t(c["g_out"]), err_word=err)
    g_item = torch.zeros_like(a[0])
    hip_ops.scatter_add_rows(g_item, a[2].reshape(-1).clamp(0, a[0].shape[0] - 1), g_hp.view(-1, g_hp.shape[2]), padding_idx=0)
    torch.cuda.synchronize()
    got = dict(out=out, g_hp=g_hp, g_item=g_item, g_pos=gpos, gW1=gW1, gb1=gb1, gW2=gW2, gb2=gb2)
    return {k: v.cpu().numpy() for k, v in got.items()}


# ------------------------------------------------------------------------------------------------ K18: the pooling
@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_pool_matches_float64_and_repeats_its_bits(pool_cases, i):
    c, ref = pool_cases[i]
    got = _pool(c)
    fig = R.figures(got, ref)
    print("parity if4rec pool case %s: %s (tol %.0e)" % (R.CASES[i], " ".join("%s=%.2e" % kv for kv in fig.items()), R.TOL))
    again = _pool(c)
    for k in got:
        assert np.array_equal(got[k], again[k]), k                              # same inputs, same bits
        assert np.isfinite(got[k]).all(), k
    valid = c["hist"] > 0
    assert (got["g_hp"][~valid] == 0).all()                                      # exactly zero at masked positions
    zero_rows = ~valid.any(axis=1)
    assert (got["out"][zero_rows] == 0).all() and (got["g_hp"][zero_rows] == 0).all()
    assert (got["g_pos"][c["hist"].shape[1]:] == 0).all()                        # position rows past T
    for k, v in fig.items():
        assert v <= R.TOL, (k, v)


# ------------------------------------------------------------------------------------------------ several visits per workgroup
_WALK = {}


def _walk_case(i):
    if i not in _WALK:
        c = R.make_case(i, R.WALK_CASES, R.WALK_SEED)
        _WALK[i] = (c, R.pool_ref(c, g_out=c["g_out"]))
    return _WALK[i]


@pytest.mark.parametrize("i", range(len(R.WALK_CASES)), ids=["x".join(map(str, s)) for s in R.WALK_CASES])
def test_pool_walk_parity_with_float64(i):
    """B above kIpBwdWg (and, at B = 4099, above kIpFwdWg): a workgroup meets several sequences, each under its own history mask
    (a row of length 1 and all-zero rows among the later ones), and carries the partials of the parameter gradients across them"""
    c, ref = _walk_case(i)
    got = _pool(c)
    fig = R.figures(got, ref)
    print("parity if4rec pool walk case %s: %s (tol %.0e)" % (R.WALK_CASES[i], " ".join("%s=%.2e" % kv for kv in fig.items()), R.WALK_TOL))
    print("parity if4rec pool walk case %s visits (b < %d | later): %s" % (R.WALK_CASES[i], R.BWD_WG,
                                                                         R.visit_fmt(R.visit_figures(got, ref, R.BWD_WG))))
    valid = c["hist"] > 0
    zero_rows = ~valid.any(axis=1)
    assert zero_rows[R.BWD_WG:].any() and (valid[R.BWD_WG:].sum(axis=1) == 1).any()
    for k in got:
        assert np.isfinite(got[k]).all(), k
    assert (got["g_hp"][~valid] == 0).all()                                      # exactly zero at masked positions
    assert (got["out"][zero_rows] == 0).all() and (got["g_hp"][zero_rows] == 0).all()
    assert (got["g_pos"][c["hist"].shape[1]:] == 0).all()                        # position rows past T
    for k, v in fig.items():
        assert v <= R.WALK_TOL, (k, v)


def test_pool_walk_two_identical_calls_give_equal_bits():
    """the case with the most visits: 8 - 9 per workgroup of the backward, 2 for three of the forward"""
    c, _ = _walk_case(R.WALK_CASES.index((4099, 2, 64, 8, 1)))
    got, again = _pool(c), _pool(c)
    for k in got:
        assert np.array_equal(got[k], again[k]), k


def test_pool_without_a_position_table(pool_cases):
    from whisprrec_amd import hip_ops
    c, _ = pool_cases[2]
    c0 = dict(c, pos=np.zeros_like(c["pos"]))
    ref = R.pool_ref(c0, g_out=c["g_out"])
    a = [_t(c[k]) for k in POOL_KEYS]
    a[1] = None
    out = hip_ops.interest_pool_fwd(*a)
    res = hip_ops.interest_pool_bwd(*a, _t(c["g_out"]))
    assert res[5] is None
    got = dict(out=out.cpu().numpy(), g_hp=res[0].cpu().numpy(), gW1=res[1].cpu().numpy(), gW2=res[3].cpu().numpy())
    for k, v in R.figures(got, ref).items():
        assert v <= R.TOL, (k, v)


def test_pool_clamps_ids_outside_the_table_and_reports_them(pool_cases):
    c, _ = pool_cases[0]
    n_items = c["item"].shape[0]
    bad, clamped = c["hist"].copy(), c["hist"].copy()
    bad[3, 0], clamped[3, 0] = -1, 0
    bad[4, 1], clamped[4, 1] = n_items, n_items - 1
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    want = _pool(c, hist=clamped, err=err)
    assert int(err.item()) == 0
    got = _pool(c, hist=bad, err=err)
    assert int(err.item()) == 1
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_autograd_function_hands_back_the_kernel_gradients(pool_cases):
    from whisprrec_amd import hip_ops
    c, _ = pool_cases[0]
    want = _pool(c)
    params = [_t(c[k]).requires_grad_(True) for k in ("item", "pos", "W1", "b1", "W2", "b2")]
    out = hip_ops.interest_pool(params[0], params[1], _t(c["hist"]), *params[2:])
    out.backward(_t(c["g_out"]))
    assert np.array_equal(out.detach().cpu().numpy(), want["out"])
    for p, k in zip(params, ("g_item", "g_pos", "gW1", "gb1", "gW2", "gb2")):
        assert np.array_equal(p.grad.cpu().numpy(), want[k]), k


# ------------------------------------------------------------------------------------------------ K19: ranks of K interests
RANK_SHAPES = [(64, 2100, 257), (32, 333, 129), (24, 500, 130)]      # (D, n_items, n): register-operand and LDS-operand scans


def _rank(c, queries=None, full_mask=False):
    from whisprrec_amd import hip_ops
    q = _t(c["queries"] if queries is None else queries)
    ptr, idx = c["mask_ptr"], c["mask_idx"]
    if full_mask:
        n_items, n_lists = c["items"].shape[0], len(c["mask_ptr"]) - 1
        ptr = np.arange(n_lists + 1, dtype=np.int64) * n_items
        idx = np.tile(np.arange(n_items, dtype=np.int32), n_lists)
    rank, tsc = hip_ops.rank_eval_multi(q, _t(c["items"]), _t(c["target"]), _t(c["mask_row"]), _t(ptr), _t(idx))
    return rank.cpu().numpy().astype(np.int64), tsc.cpu().numpy()


@pytest.mark.parametrize("shape", RANK_SHAPES)
@pytest.mark.parametrize("KQ", [1, 2, 4])
def test_rank_eval_multi_equals_the_float64_oracle(shape, KQ):
    from whisprrec_amd import hip_ops
    D, n_items, n = shape
    c = R.make_rank_case(D, n_items, n, KQ)
    assert (c["mask_row"] != np.arange(n)).all()
    want, margin = R.rank_ref(c)
    ok = margin > R.RANK_MARGIN
    rank, tsc = _rank(c)
    print("parity if4rec rank KQ=%d D=%d items=%d n=%d: kept %.3f differing on kept rows %d" %
          (KQ, D, n_items, n, ok.mean(), int((rank[ok] != want[ok]).sum())))
    assert ok.mean() > 0.9
    assert np.array_equal(rank[ok], want[ok])
    per = np.einsum("ekd,jd->ekj", c["queries"].astype(np.float64), c["items"].astype(np.float64)).max(axis=1)
    assert np.abs(tsc - per[np.arange(n), c["target"]]).max() <= 1e-5 * np.abs(per).max()
    for w in R.WRONG_RANK if KQ > 1 else ():
        assert (R.rank_ref(c, variant=w)[0][ok] != rank[ok]).any(), w
    # the interests of a row in another order: the same ranks and target scores
    perm = c["queries"][:, ::-1, :].copy()
    rank_p, tsc_p = _rank(c, queries=perm)
    assert np.array_equal(rank_p, rank) and np.array_equal(tsc_p, tsc)
    # every item masked: nothing counts
    assert (_rank(c, full_mask=True)[0] == 1).all()
    if KQ == 1:                                                   # one query per row: the bits of wr_rank_eval_rows
        r1, t1 = hip_ops.rank_eval_rows(_t(c["queries"][:, 0, :]), _t(c["items"]), _t(c["target"]), _t(c["mask_row"]),
                                        _t(c["mask_ptr"]), _t(c["mask_idx"]))
        assert np.array_equal(r1.cpu().numpy(), rank) and np.array_equal(t1.cpu().numpy(), tsc)


def test_rank_eval_multi_without_a_mask():
    c = R.make_rank_case(64, 2100, 257, 2)
    c0 = dict(c, mask_ptr=np.zeros_like(c["mask_ptr"]), mask_idx=np.zeros(0, np.int32))
    want, margin = R.rank_ref(c0)
    from whisprrec_amd import hip_ops
    rank, _ = hip_ops.rank_eval_multi(_t(c["queries"]), _t(c["items"]), _t(c["target"]))
    ok = margin > R.RANK_MARGIN
    assert np.array_equal(rank.cpu().numpy()[ok], want[ok])


# ------------------------------------------------------------------------------------------------ the model
def _model(g14, **kw):
    from whisprrec_amd.if4rec import IF4Rec
    m = IF4Rec(_args(device=DEV, **kw), host.Corpus(40, 300, {}))
    sd = {str(n): torch.from_numpy(g14["sd__" + str(n)]) for n in g14["names"]}
    m.load_state_dict(sd)
    return m.to(DEV)


def _feed(g14, rows):
    return {"history_items": _t(g14["history"][rows]), "lengths": _t(g14["lengths"][rows]), "pos_item": _t(g14["item_id"][rows, 0]),
            "neg_items": _t(g14["item_id"][rows, 1:]), "phase": "train", "batch_size": int(len(rows))}


def _judged_rows(g14, **kw):
    """rows of g14's batch whose train-time choice of an interest is not a near-tie (gap > 1e-4 relative), on the torch path"""
    m = _model(g14, **kw)
    m.eval()
    with torch.no_grad():
        interests = m.forward(_feed(g14, np.arange(96)))
        tp = (interests * m.i_embeddings.weight[_t(g14["item_id"][:, 0])][:, None, :]).sum(-1)
    top = tp.topk(2, dim=1)[0]
    gap = ((top[:, 0] - top[:, 1]) / tp.abs().max()).cpu().numpy()
    return np.nonzero(gap > 1e-4)[0]


def _loss_and_grads(g14, rows, **kw):
    m = _model(g14, **kw)
    m.train()
    loss = m.predict(_feed(g14, rows))
    loss.backward()
    if m.interest_native:
        m.check_history_ids()
    return m, float(loss.detach()), {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()}


def _report(tag, fig):
    print("parity if4rec g14 %s gradients: %s" % (tag, " ".join("%s=%.2e" % (n.replace("transformer_block.0.", "tb0."), v)
                                                              for n, v in fig.items())))


def test_interest_native_model_matches_its_torch_path_on_g14(g14):
    """loss and every gradient under if4rec_ref.TOL; the four gradients of the blocks' score path under MODEL_QK_TOL, because
    the stock path itself misses TOL on them (if4rec_ref.py)"""
    rows = _judged_rows(g14)
    print("parity if4rec g14: rows above the selection gap %.3f" % (len(rows) / 96.0))
    assert len(rows) / 96.0 > 0.9
    _, loss_t, grads_t = _loss_and_grads(g14, rows)
    m, loss_n, grads_n = _loss_and_grads(g14, rows, interest_native=1)
    assert m._interest_native_ok == {20: True}, "the kernels refused the golden shape"
    fig = R.model_grad_figures(grads_n, grads_t)
    print("parity if4rec g14 interest_native: loss native %.7f torch %.7f (tol %.0e, score path %.0e)" %
          (loss_n, loss_t, R.TOL, R.MODEL_QK_TOL))
    _report("interest_native", fig)
    assert abs(loss_n - loss_t) <= R.TOL * abs(loss_t)
    for n, v in fig.items():
        assert v <= R.model_tol(n), (n, v)


def test_block_native_model_matches_its_torch_path_at_four_heads(g14):
    """--block_native 1 at n_head 4: the blocks over the K interest tokens on the key-length kernels (every token a key).  The
    loss under the block's `out` tolerance and the gradients under its `gparam` tolerance (tests/sasblock_ref.py); the score-path
    gradients under MODEL_QK_TOL as above"""
    rows = _judged_rows(g14, n_head=4)
    _, loss_t, grads_t = _loss_and_grads(g14, rows, n_head=4)
    m, loss_n, grads_n = _loss_and_grads(g14, rows, n_head=4, block_native=1)
    assert m._block_native_ok is True
    fig = R.model_grad_figures(grads_n, grads_t)
    print("parity if4rec g14 block_native: loss native %.7f torch %.7f" % (loss_n, loss_t))
    _report("block_native", fig)
    assert abs(loss_n - loss_t) <= S.TOL["out"] * abs(loss_t)
    for n, v in fig.items():
        assert v <= (R.MODEL_QK_TOL if n.endswith(R.SCORE_PATH) else S.TOL["gparam"]), (n, v)


def test_eight_heads_keep_the_torch_blocks_with_one_warning(g14, caplog):
    import logging
    m = _model(g14, block_native=1)
    with caplog.at_level(logging.WARNING):
        for _ in range(2):
            m.predict(_feed(g14, np.arange(8)))
    assert m._block_native_ok is False
    assert sum("block_native" in r.getMessage() for r in caplog.records) == 1


def test_dropout_on_the_native_blocks_repeats_its_bits_for_a_seed(g14):
    rows = np.arange(96)
    kw = dict(n_head=4, block_native=1, interest_native=1, encoder_dropout=0.3, random_seed=11)
    _, loss_a, grads_a = _loss_and_grads(g14, rows, **kw)
    _, loss_b, grads_b = _loss_and_grads(g14, rows, **kw)
    _, loss_0, _ = _loss_and_grads(g14, rows, **dict(kw, encoder_dropout=0.0))
    _, loss_s, _ = _loss_and_grads(g14, rows, **dict(kw, random_seed=12))
    assert loss_a == loss_b and all(np.array_equal(grads_a[n], grads_b[n]) for n in grads_a)
    assert loss_a != loss_0 and loss_a != loss_s                 # the dropout is applied, and keyed by the seed


# ------------------------------------------------------------------------------------------------ the launcher
def _write_ml100k(tmp):
    (tmp / "ml-100k").mkdir()
    with gzip.open(os.path.join(GOLD, "ml-100k.inter.gz"), "rb") as src, open(tmp / "ml-100k" / "ml-100k.inter", "wb") as dst:
        shutil.copyfileobj(src, dst)
    return str(tmp) + "/"


def _argv(path, tmp, extra):
    return ["--model_name", "IF4Rec", "--runner_name", "HipRunner", "--dataset", "ml-100k", "--path", path, "--epoch", "2",
            "--batch_size", "1024", "--eval_batch_size", "2048", "--lr", "1e-3", "--l2", "0.0", "--emb_size", "64", "--history_max", "20",
            "--n_head", "4", "--encoder_dropout", "0.0", "--log_file", str(tmp / "log.txt"), "--model_path", str(tmp / "m.pt"),
            "--num_workers", "0", "--topk", "5,10", "--metric", "NDCG, HR", "--random_seed", "3407"] + extra


EPOCH_MARGIN = 4e-6


def test_two_epoch_launcher_run_native_against_torch_path(tmp_path, monkeypatch):
    """`main`'s training for two epochs on tests/golden/ml-100k.inter.gz, --interest_native 1 --block_native 1 --seq_eval_native 1
    against the flag-off run, same seed: the epoch losses agree within EPOCH_MARGIN (relative), the dev metrics up to a handful
    of near-tied ranks (the allowance of tests/test_hip_seq_eval.py).  The file numbers its items from 0, so some histories hold
    only item 0 and are all-masked rows: both paths pass them no gradient.

    The margin comes from the torch path alone, as in tests/test_hip_contrarec.py: the flag-off command run again with its sums
    in another order.  Measured on an MI355X, relative to the plain torch run (epoch losses 0.4303705, 0.2293486), epoch 1 /
    epoch 2:
        the same command again                                                              0 / 0
        every batch with its rows reversed (the sums over the batch run backwards)          0 / 4.5e-7
        the GEMMs on the other BLAS libraries (torch.backends.cuda.preferred_blas_library)  0 / 0
    The largest, 4.5e-7, is the floor; by DESIGN section 2's rule EPOCH_MARGIN = 8 x floor rounded up to one digit.  The native
    run measured 0 / 0 in the same session: at lr 1e-3 the two trajectories stay within an ulp of the fp32 epoch means."""
    from whisprrec_amd import main as launcher, runner
    path = _write_ml100k(tmp_path)
    curves, metrics, n_eval = {}, {}, 0
    host_eval = runner.BaseRunner.interface
    for tag, extra in (("torch", []), ("native", ["--interest_native", "1", "--block_native", "1", "--seq_eval_native", "1"])):
        args, model_class, reader_class, runner_class = launcher.build_args(_argv(path, tmp_path, extra))
        launcher.init_seed(args.random_seed)
        args.device = DEV
        corpus = reader_class(args).corpus()
        model = model_class(args, corpus).to(DEV)
        data = {ph: model_class.Dataset(model, corpus, ph) for ph in ("train", "dev")}
        run = runner_class(args)
        if tag == "native":
            monkeypatch.setattr(runner.BaseRunner, "interface", lambda *a: pytest.fail("the host evaluation ran"))
        curves[tag] = [run.fit(data["train"], epoch=e + 1) for e in range(2)]
        metrics[tag] = run.evaluate(data["dev"], [5, 10], ["NDCG", "HR"])
        n_eval = len(data["dev"])
        if tag == "native":
            monkeypatch.setattr(runner.BaseRunner, "interface", host_eval)
            model.check_history_ids()
            assert all(model._interest_native_ok.values()) and model._block_native_ok is True and run._seq_eval_ok(data["dev"])
    rel = np.abs(np.asarray(curves["native"]) / np.asarray(curves["torch"]) - 1.0)
    print("parity if4rec ml-100k epochs: torch %s native %s rel %s (margin %.0e)" % (curves["torch"], curves["native"], rel, EPOCH_MARGIN))
    print("parity if4rec ml-100k dev metrics: torch %s native %s" % (metrics["torch"], metrics["native"]))
    assert curves["torch"][1] < curves["torch"][0]
    assert rel.max() <= EPOCH_MARGIN
    flips = 6.0 / n_eval                              # a handful of near-tied ranks may fall on the other side of the cut
    for key in metrics["torch"]:
        assert abs(metrics["torch"][key] - metrics["native"][key]) <= flips, key


def test_device_evaluation_equals_the_host_loop(tmp_path):
    """--seq_eval_native 1 on the small corpus: the ranks of wr_rank_eval_multi equal the host loop's over full_predict, on rows
    whose target is not nearly tied with another item"""
    from test_reader import _write_inter
    from whisprrec_amd import main as launcher, runner
    g8 = np.load(os.path.join(GOLD, "g8_reader.npz"))
    path = _write_inter(g8, tmp_path)
    argv = _argv(path, tmp_path, ["--seq_eval_native", "1", "--interest_native", "1", "--emb_size", "32"])
    args, model_class, reader_class, runner_class = launcher.build_args(argv)
    launcher.init_seed(args.random_seed)
    args.device = DEV
    corpus = reader_class(args).corpus()
    model = model_class(args, corpus).to(DEV)
    with torch.no_grad():
        model.i_embeddings.weight.mul_(30)                                      # scores spread: few near-ties
    ds = model_class.Dataset(model, corpus, "dev")
    run = runner_class(args)
    assert run._seq_eval_ok(ds)
    pred = runner.BaseRunner(args).interface(ds).astype(np.float64)
    host_rank = np.argwhere((-pred).argsort(axis=1) == 0)[:, 1] + 1
    rank = run.rank_rows(ds)
    target, Sc = pred[:, 0], pred[:, 1:].copy()
    Sc[np.arange(len(ds)), np.asarray(ds.data["item_id"])] = np.nan
    fin = np.isfinite(Sc)
    ok = np.where(fin, np.abs(Sc - target[:, None]), np.inf).min(axis=1) > 1e-5 * np.abs(Sc[fin]).max()
    print("parity if4rec seq eval: n_eval %d rows kept %.4f ranks differing on kept rows %d" %
          (len(ds), ok.mean(), int((rank[ok] != host_rank[ok]).sum())))
    assert ok.mean() >= 0.9 and np.array_equal(rank[ok], host_rank[ok])
    with pytest.raises(NotImplementedError, match="top-K over several interests"):
        run.recommend_rows(ds, 5)
