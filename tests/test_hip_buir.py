"""GPU checks of BUIR's native paths: the fused bootstrap loss and gradient (wr_buir_loss_grad, K16) against the float64
restatement of tests/buir_ref.py under its tolerance, with the same bits on a second call; the dense table gradients of the
autograd function and the error word; the momentum update (wr_ema_update, K17) bit for bit against torch's expression on the same
device; then the model with --buir_native 1 against its own torch path and the reference's numbers (g13), over a 2-epoch launcher
run on the committed ml-100k file, and through the device evaluation and top-K.  Figures are printed as `parity ...` lines."""
import argparse
import gzip
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buir_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(GOLD, "g13_buir.npz"))


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _call(case, **kw):
    from whisprrec_amd import hip_ops
    t = {k: _t(v) for k, v in case.items()}
    return hip_ops.buir_loss_grad(t["Uo"], t["Io"], t["Ut"], t["It"], t["W"], t["b"], t["users"], t["items"], **kw)


def _np(out):
    loss, gU, gI, gW, gb = out
    return {"loss": float(loss.item()), "gU": gU.cpu().numpy(), "gI": gI.cpu().numpy(), "gW": gW.cpu().numpy(), "gb": gb.cpu().numpy()}


# ------------------------------------------------------------------------------------------------ K16
@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_loss_grad_matches_float64_and_repeats_its_bits(i):
    case = R.make_case(i)
    ref = R.buir_f64(case)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _call(case, err_word=err)
    got = _np(a)
    fig = R.figures(got, ref)
    print(R.fmt("%s B=%d D=%d" % R.CASES[i][:3], fig))
    assert int(err.item()) == 0
    assert all(np.isfinite(v).all() for v in got.values())
    assert max(fig.values()) <= R.TOL, fig
    b = _call(case)
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                           # no float atomics, a fixed order: the same bits
    only = _call(case, grads=False)
    assert torch.equal(only[0], a[0]) and all(v is None for v in only[1:])
    if R.CASES[i][3] == "zero_target":
        assert np.abs(got["gU"][0]).max() == 0.0 and np.abs(got["gI"][1]).max() == 0.0


def test_autograd_function_builds_dense_gradients_and_backward_is_idempotent():
    from whisprrec_amd import hip_ops
    i = [c[0] for c in R.CASES].index("few_ids")
    case = R.make_case(i)
    ref = R.buir_f64(case)
    t = {k: _t(v) for k, v in case.items()}
    for k in ("Uo", "Io", "W", "b"):
        t[k].requires_grad_(True)
    loss = hip_ops.buir_loss(t["Uo"], t["Io"], t["Ut"], t["It"], t["W"], t["b"], t["users"], t["items"])
    (3.0 * loss).backward(retain_graph=True)
    first = {k: t[k].grad.clone() for k in ("Uo", "Io", "W", "b")}
    fig = {"dU": R.rel_err(first["Uo"].cpu().numpy(), 3.0 * ref["dU"]), "dI": R.rel_err(first["Io"].cpu().numpy(), 3.0 * ref["dI"]),
           "gW": R.rel_err(first["W"].cpu().numpy(), 3.0 * ref["gW"]), "gb": R.rel_err(first["b"].cpu().numpy(), 3.0 * ref["gb"])}
    print("parity buir dense gradients: " + " ".join("%s %.2e" % kv for kv in fig.items()) + " (tol %.0e)" % R.TOL)
    assert max(fig.values()) <= R.TOL, fig
    untouched = np.setdiff1d(np.arange(R.N_USERS), case["users"])
    assert float(first["Uo"][_t(untouched)].abs().max()) == 0.0
    for k in first:
        t[k].grad = None
    (3.0 * loss).backward(retain_graph=True)                               # a second backward: the same gradients, not doubled
    for k in first:
        assert torch.equal(t[k].grad, first[k]), k
    with torch.no_grad():
        quiet = hip_ops.buir_loss(t["Uo"], t["Io"], t["Ut"], t["It"], t["W"], t["b"], t["users"], t["items"])
    assert not quiet.requires_grad and torch.equal(quiet, loss.detach())


def test_unsafe_id_sets_the_error_word_and_faults_nothing(g13):
    case = R.make_case(2)
    case["users"] = case["users"].copy()
    case["users"][5] = R.N_USERS                                           # one past the table
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = _np(_call(case, err_word=err))
    assert int(err.item()) == 1
    assert all(np.isfinite(v).all() for v in got.values())
    m = _model(g13, buir_native=1)
    users = g13["users"].copy()
    users[0] = R.N_USERS
    loss = m.predict({"user_id": _t(users), "pos_item": _t(g13["items"])})
    loss.backward()                                                        # the scatter takes the clamped id too
    torch.cuda.synchronize()
    assert torch.isfinite(m.user_online.weight.grad).all()
    with pytest.raises(IndexError):
        m.check_ids()
    m.check_ids()                                                          # the word was cleared


# ------------------------------------------------------------------------------------------------ K17
@pytest.mark.parametrize("shape", [(1, 4), (257, 36), (1000, 64)])
def test_ema_update_is_bitwise_torchs_expression(shape):
    from whisprrec_amd import hip_ops
    rng = np.random.RandomState(shape[0])
    t0, o = _t(rng.standard_normal(shape).astype(np.float32)), _t(rng.standard_normal(shape).astype(np.float32))
    for m in (0.995, 0.9, 0.0, 1.0):
        for online in (o, None):
            t = t0.clone()
            src = t.clone() if online is None else online                  # o equal to t: still rewritten, t m + t (1 - m) != t
            want = t * m + src * (1. - m)
            out = hip_ops.ema_update_(t, src, m)
            assert out is t and torch.equal(t, want), (shape, m, online is None)


# ------------------------------------------------------------------------------------------------ the model on g13
def _args(**kw):
    base = dict(device=DEV, model_path="/tmp/wr_buir.pt", buffer=1, num_neg=1, test_all=1, embedding_size=64, momentum=0.995,
                buir_native=0)
    base.update(kw)
    return argparse.Namespace(**base)


def _model(g13, **kw):
    from whisprrec_amd import host
    from whisprrec_amd.buir import BUIR
    m = BUIR(_args(**kw), host.Corpus(R.N_USERS, R.N_ITEMS, {}))
    m.load_state_dict({str(n): torch.from_numpy(g13["sd__" + str(n)]) for n in g13["names"]})
    return m.to(DEV).train()


def _feed(g13):
    return {"user_id": _t(g13["users"]), "pos_item": _t(g13["items"]), "neg_items": torch.ones(96, 1, dtype=torch.int64, device=DEV),
            "batch_size": 96, "phase": "train"}


def test_native_model_matches_its_torch_path_and_the_reference_on_g13(g13):
    grads, losses = {}, {}
    for tag, native in (("torch", 0), ("native", 1)):
        m = _model(g13, buir_native=native)
        loss = m.predict(_feed(g13))
        loss.backward()
        losses[tag] = float(loss.detach())
        grads[tag] = {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters() if p.requires_grad}
        if native:
            m.check_ids()
            assert m._buir_native_ok is True, "the kernels refused the golden shape"
    ref = float(g13["loss"][0])
    print("parity buir g13 loss: native %.7f torch %.7f reference %.7f (tol %.0e)" % (losses["native"], losses["torch"], ref, R.LOSS_TOL))
    assert abs(losses["native"] - losses["torch"]) <= R.LOSS_TOL * abs(ref) and abs(losses["native"] - ref) <= R.LOSS_TOL * abs(ref)
    worst = 0.0
    for n, g in grads["native"].items():
        for other in (grads["torch"][n], g13["g__" + n]):
            e = R.rel_err(g, other)
            worst = max(worst, e)
            assert e <= R.TOL, (n, e)
    print("parity buir g13 gradients: worst %.2e (tol %.0e)" % (worst, R.TOL))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_native_adam_runs_reproduce_the_reference(g13, tag):
    momentum, lr = R.RUNS[tag]
    m = _model(g13, buir_native=1, momentum=momentum)
    m.optimizer = torch.optim.Adam(m.parameters(), lr=lr)
    curve = []
    for _ in range(5):
        m.optimizer.zero_grad()
        loss = m.predict(_feed(g13))
        loss.backward()
        m.optimizer.step()
        curve.append(float(loss.detach()))
    m.check_ids()
    assert m._buir_native_ok is True
    sd = {str(n): g13["sd__" + str(n)] for n in g13["names"]}
    tables = {k: v.cpu().numpy() for k, v in m.state_dict().items() if k in R.TABLES}
    gt = {k: g13[tag + "_sd__" + k] for k in R.TABLES}
    fig = R.run_figures(np.asarray(curve), tables, sd, g13[tag + "_losses"].astype(np.float64), gt)
    print(R.run_fmt("native " + tag, fig))
    assert fig["losses"] <= R.RUN_TOL["losses"] and fig["online_update"] <= R.RUN_TOL["online_update"], fig
    if tag == "b":                                       # run (a)'s target move is below what fp32 can judge (buir_ref)
        assert fig["target_update"] <= R.RUN_TOL["target_update"], fig
    untouched = np.setdiff1d(np.arange(R.N_USERS), g13["users"])
    assert np.array_equal(tables["user_target.weight"][untouched], gt["user_target.weight"][untouched])


# ------------------------------------------------------------------------------------------------ the launcher
def _write_ml100k(tmp):
    (tmp / "ml-100k").mkdir()
    with gzip.open(os.path.join(GOLD, "ml-100k.inter.gz"), "rb") as src, open(tmp / "ml-100k" / "ml-100k.inter", "wb") as dst:
        shutil.copyfileobj(src, dst)
    return str(tmp) + "/"


def _argv(path, tmp, extra):
    return ["--model_name", "BUIR", "--runner_name", "HipRunner", "--dataset", "ml-100k", "--path", path, "--epoch", "2",
            "--batch_size", "1024", "--eval_batch_size", "2048", "--lr", "1e-3", "--l2", "0.0", "--embedding_size", "64",
            "--log_file", str(tmp / "log.txt"), "--model_path", str(tmp / "m.pt"), "--num_workers", "0", "--topk", "5,10",
            "--metric", "NDCG, HR", "--random_seed", "3407"] + extra


def launcher_epochs(path, tmp, extra, reverse_rows=False, epochs=2):
    """`main`'s training loop for `epochs` epochs -> (epoch losses, model).  reverse_rows: every batch reaches predict with its rows
    in reverse order (the sums over the batch run backwards; the result on paper is the same)."""
    from whisprrec_amd import main as launcher
    args, model_class, reader_class, runner_class = launcher.build_args(_argv(path, tmp, extra))
    launcher.init_seed(args.random_seed)
    args.device = DEV
    corpus = reader_class(args).corpus()
    model = model_class(args, corpus).to(DEV)
    if reverse_rows:
        plain = model.predict
        model.predict = lambda fd: plain({k: (v.flip(0) if isinstance(v, torch.Tensor) else v) for k, v in fd.items()})
    data = model_class.Dataset(model, corpus, "train")
    run = runner_class(args)
    return [run.fit(data, epoch=e + 1) for e in range(epochs)], model


EPOCH_MARGIN = 5e-7


def test_two_epoch_launcher_run_native_against_torch_path(tmp_path):
    """`main`'s training for two epochs on tests/golden/ml-100k.inter.gz, --buir_native 1 against the torch path, same seed,
    --batch_size 1024: the epoch losses agree within EPOCH_MARGIN (relative).

    The margin comes from the torch path alone: this command run again with its sums in another order.  Measured on an MI355X,
    relative to the plain torch run (epoch losses 3.996968031, 3.987514019), epoch 1 / epoch 2:
        the same command again                                                              0 / 0
        the GEMMs on the other BLAS library (torch.backends.cuda.preferred_blas_library)   0 / 0
        every batch with its rows reversed (the sums over the batch run backwards)          0 / 0
    The epoch loss is the fp32 mean of about 80 batch losses near 4, and a batch loss moves by about 1e-7 of itself under such a
    reordering: the mean moves by less than one unit in the last place of the fp32 number `fit` returns, 2^-22 = 6.0e-8 of 3.99,
    and no smaller figure can be observed.  That unit is therefore taken as the floor; by DESIGN section 2's rule EPOCH_MARGIN =
    8 x floor rounded up to one digit.  The native run measured 0 / 0 in the same session."""
    path = _write_ml100k(tmp_path)
    torch_curve, _ = launcher_epochs(path, tmp_path, [])
    native_curve, model = launcher_epochs(path, tmp_path, ["--buir_native", "1"])
    model.check_ids()
    assert model._buir_native_ok is True
    rel = np.abs(np.asarray(native_curve) / np.asarray(torch_curve) - 1.0)
    print("parity buir ml-100k epochs: torch %s native %s rel %s (margin %.0e)" % (torch_curve, native_curve, rel, EPOCH_MARGIN))
    assert torch_curve[1] < torch_curve[0]
    assert rel.max() <= EPOCH_MARGIN


# ------------------------------------------------------------------------------------------------ evaluation and top-K
def test_device_evaluation_and_topk_equal_the_host_loop(tmp_path):
    """HipRunner.evaluate and recommend through eval_factors() (width 2 D = 64) on the small corpus against BaseRunner.interface:
    the same rank wherever the target is separated from every unmasked item by more than 1e-5 max|score| in float64"""
    from test_reader import _write_inter
    from whisprrec_amd import hip_ops, main as launcher, runner
    g8 = np.load(os.path.join(GOLD, "g8_reader.npz"))
    path = _write_inter(g8, tmp_path)
    args, model_class, reader_class, runner_class = launcher.build_args(
        _argv(path, tmp_path, ["--embedding_size", "32", "--buir_native", "1"]))
    launcher.init_seed(args.random_seed)
    args.device = DEV
    corpus = reader_class(args).corpus()
    model = model_class(args, corpus).to(DEV)
    with torch.no_grad():
        model.item_online.weight.mul_(30)
    assert hip_ops.rank_eval_supports(64) and model.eval_factors()[0].shape[1] == 64
    data = model_class.Dataset(model, corpus, "dev")
    rn = runner_class(args)
    assert isinstance(rn, runner.HipRunner)
    topks, metrics = [5, 10], ["NDCG", "HR"]

    pred = runner.BaseRunner.interface(rn, data).astype(np.float64)           # [n, 1 + n_items], masked items at -inf
    target, S = pred[:, 0], pred[:, 1:]
    host_rank = 1 + (S > target[:, None]).sum(axis=1)
    finite = np.isfinite(S)
    gap = np.where(finite, np.abs(S - target[:, None]), np.inf).min(axis=1)
    keep = gap > 1e-5 * np.abs(S[finite]).max()
    n = len(target)
    print("parity buir eval: %d rows, %.4f kept" % (n, keep.mean()))
    assert keep.mean() >= 0.9

    user_mat, item_mat = model.eval_factors()
    ptr, idx = rn._clicked_mask(corpus, True, user_mat.shape[0], DEV)
    rank, _ = hip_ops.rank_eval(user_mat, item_mat, _t(data.data["user_id"]), _t(data.data["item_id"]), ptr, idx)
    rank = rank.cpu().numpy().astype(np.int64)
    assert np.array_equal(rank[keep], host_rank[keep])
    dev_metrics = rn.evaluate(data, topks, metrics)
    host_metrics = runner.BaseRunner.metrics_from_ranks(host_rank, topks, metrics)
    left_out = (n - keep.sum()) / n
    for k in host_metrics:
        assert abs(dev_metrics[k] - host_metrics[k]) <= left_out + 1e-12, (k, dev_metrics[k], host_metrics[k])

    # recommend: the k best unmasked items; of those, min(rank - 1, k) score above the (masked) target
    k = 20
    users = np.asarray(data.data["user_id"])
    items, _ = rn.recommend(model, corpus, users, k)
    above = (np.take_along_axis(S, items, axis=1) > target[:, None]).sum(axis=1)
    assert np.array_equal(above[keep], np.minimum(host_rank - 1, k)[keep])
