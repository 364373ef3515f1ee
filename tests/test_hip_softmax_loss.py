"""GPU checks for the full-catalogue softmax loss (K26, wr_softmax.hip): parity with the float64 restatement of
tests/softmax_ref.py, bit-reproducibility, the excluded padding row, bad targets, memory, autograd, and SASRec / TiSASRec under
--train_loss softmax with --softmax_native 1 against 0."""
import argparse
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sasblock_ref as K13  # noqa: E402
import softmax_ref as R  # noqa: E402
import tisas_ref as K25  # noqa: E402
from whisprrec_amd import hip_ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = R.cases()
_REF = {}


def _case(tag):
    """inputs and the float64 triple of a parity case, computed once and never written to"""
    if tag not in _REF:
        _, i, v, seed = next(c for c in CASES if c[0] == tag)
        Q, E, t = R.make_case(*R.SHAPES[i], seed, v)
        _REF[tag] = (Q, E, t, R.softmax_ce_f64(Q, E, t))
    return _REF[tag]


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _np(triple):
    return float(triple[0].cpu()[0]), triple[1].cpu().numpy(), triple[2].cpu().numpy()


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_parity_with_float64(tag):
    Q, E, t, ref = _case(tag)
    got = _np(hip_ops.softmax_ce_loss_grad(_t(Q), _t(E), _t(t)))
    assert np.isfinite(got[0]) and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    fig = R.figures(got, ref, t)
    print(R.fmt(tag, fig))
    for k in R.FIGURES:
        assert fig[k] < R.TOL[k], (tag, k, fig[k])
    assert not got[2][0].any()                                              # the padding row is written as zeros


@pytest.mark.parametrize("tag", ["3706x200x64-dup", "20000x520x64-large", "4099x257x128-random", "70x1x64-random"])
def test_same_inputs_same_bits(tag):
    Q, E, t, _ = _case(tag)
    q, e, tt = _t(Q), _t(E), _t(t)
    a = hip_ops.softmax_ce_loss_grad(q, e, tt)
    b = hip_ops.softmax_ce_loss_grad(q, e, tt)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    only, gq, ge = hip_ops.softmax_ce_loss_grad(q, e, tt, grads=False)
    assert gq is None and ge is None and torch.equal(only, a[0])
    base = torch.full((1,), 3.5, dtype=torch.float32, device=DEV)
    acc = hip_ops.softmax_ce_loss_grad(q, e, tt, loss=base, grads=False)[0]
    assert acc is base and torch.equal(acc, torch.full_like(acc, 3.5) + a[0])
    out = (torch.full_like(a[1], np.nan), torch.full_like(a[2], np.nan))
    c = hip_ops.softmax_ce_loss_grad(q, e, tt, out=out)
    assert c[1] is out[0] and torch.equal(c[1], a[1]) and torch.equal(c[2], a[2])     # every row is written


def test_excluded_rows_are_exact_zeros_and_weight_scales():
    Q, E, t, ref = _case("3706x200x64-random")
    q, e = _t(Q), _t(E)
    _, _, ge = hip_ops.softmax_ce_loss_grad(q, e, _t(t))
    assert not ge[0].any() and ge[1:].abs().sum(dim=1).min() > 0
    t3 = np.maximum(t, 3)
    got = _np(hip_ops.softmax_ce_loss_grad(q, e, _t(t3), first_class=3, weight=1.0))
    assert not got[2][:3].any()
    fig = R.figures(got, R.softmax_ce_f64(Q, E, t3, first_class=3, weight=1.0), t3)
    print(R.fmt("first_class 3, sum", fig))
    assert all(fig[k] < R.TOL[k] for k in R.FIGURES), fig


def test_rows_and_columns_without_mass_are_finite():
    """a zero query (uniform softmax), a zero item, an item whose probability underflows to 0 for every query, and a query
    whose target holds all the mass"""
    rng = np.random.RandomState(3)
    n, B, D = 300, 130, 64
    Q = rng.standard_normal((B, D)).astype(np.float32)
    E = (rng.standard_normal((n, D)) * 0.1).astype(np.float32)
    Q[0] = 0
    E[5] = 0
    E[7] = -40 * np.abs(E[7])
    Q[1:] = np.abs(Q[1:])                                                   # <Q[b], E[7]> << 0: exp underflows
    t = rng.randint(1, n, B).astype(np.int64)
    t[t == 7] = 8
    E[9] = 3.0
    t[2] = 9                                                                # <Q[2], E[9]> ~ 150: p_target = 1
    got = _np(hip_ops.softmax_ce_loss_grad(_t(Q), _t(E), _t(t)))
    assert np.isfinite(got[0]) and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    ref = R.softmax_ce_f64(Q, E, t)
    assert abs(got[0] - ref[0]) / abs(ref[0]) < R.TOL["loss"]
    assert R.rel_err(got[1], ref[1]) < R.TOL["gQ"] and R.rel_err(got[2], ref[2]) < R.TOL["gE_in"]
    assert np.abs(got[2][7]).max() <= 1e-30


def test_bad_targets_raise_and_are_clamped():
    Q, E, t, _ = _case("5000x130x32-random")
    n = E.shape[0]
    q, e = _t(Q), _t(E)
    for b, bad, clamp in ((3, 0, 1), (50, -1, 1), (129, n, n - 1)):
        tb, tc = t.copy(), t.copy()
        tb[b], tc[b] = bad, clamp
        with pytest.raises(IndexError, match="outside"):
            hip_ops.softmax_ce_loss_grad(q, e, _t(tb))
        a = hip_ops.softmax_ce_loss_grad(q, e, _t(tb), validate=False)       # never dereferenced out of range: the clamp's result
        c = hip_ops.softmax_ce_loss_grad(q, e, _t(tc))
        assert all(torch.equal(x, y) for x, y in zip(a, c))
        good = hip_ops.softmax_ce_loss_grad(q, e, _t(t))
        keep = np.arange(len(t)) != b
        assert torch.equal(a[1][_t(keep)], good[1][_t(keep)])                 # the valid rows' gradients are unaffected
    hip_ops.softmax_ce_loss_grad(q, e, _t(t))                               # the error word is cleared by the next call


def test_no_score_matrix_at_two_hundred_thousand_items():
    n, B, D = 200_003, 2048, 64
    g = torch.Generator(device="cpu").manual_seed(5)
    q = torch.randn(B, D, generator=g).to(DEV)
    e = (torch.randn(n, D, generator=g) * 0.1).to(DEV)
    t = torch.randint(1, n, (B,), generator=g).to(DEV)
    hip_ops.softmax_ce_release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    loss, gq, ge = hip_ops.softmax_ce_loss_grad(q, e, t)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated(DEV) - base
    print("peak memory growth of one call at n=%d B=%d: %.1f MB (a score matrix: %.1f MB)" % (n, B, growth / 1e6, B * n * 4 / 1e6))
    assert growth < B * n * 4 // 8, growth
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(gq).all()) and bool(torch.isfinite(ge).all())
    # uniform-ish scores: the loss is near log(n - 1) + sigma^2 / 2 of the scores (sd 0.8)
    assert abs(float(loss) - (np.log(n - 1) + 0.32)) < 0.1
    hip_ops.softmax_ce_release_workspaces()


def test_autograd_against_the_stock_lines():
    Q, E, t, _ = _case("3706x200x64-dup")
    tt = _t(t)
    q0, e0 = _t(Q).requires_grad_(True), _t(E).requires_grad_(True)
    stock = R.stock_lines(q0, e0, tt)
    sq, se = torch.autograd.grad(stock, [q0, e0])
    q, e = _t(Q).requires_grad_(True), _t(E).requires_grad_(True)
    loss = hip_ops.softmax_ce_loss(q, e, tt)
    assert loss.dim() == 0 and loss.requires_grad
    loss.backward(retain_graph=True)
    fig = R.figures((float(loss.detach()), q.grad.cpu().numpy(), e.grad.cpu().numpy()),
                    (float(stock.detach()), sq.cpu().numpy().astype(np.float64), se.cpu().numpy().astype(np.float64)), t)
    print(R.fmt("autograd against the stock lines on the device", fig))
    assert all(fig[k] < R.TOL[k] for k in R.FIGURES), fig
    once_q, once_e = q.grad.clone(), e.grad.clone()
    loss.backward(retain_graph=True)                                        # a second backward accumulates the SAME gradient
    assert torch.equal(q.grad, once_q + once_q) and torch.equal(e.grad, once_e + once_e)
    (3.0 * loss).backward()
    assert torch.equal(q.grad, once_q + once_q + 3.0 * once_q)
    with torch.no_grad():
        assert torch.equal(hip_ops.softmax_ce_loss(q, e, tt), loss.detach())
    assert not hip_ops.softmax_ce_loss(q.detach(), e.detach(), tt).requires_grad
    only_q = hip_ops.softmax_ce_loss(q, e.detach(), tt)
    gq, = torch.autograd.grad(only_q, [q])
    assert torch.equal(gq, once_q)


# ------------------------------------------------------------------------------------------------ the models
class _Corpus:
    """what the two models read from a reader: sizes and user_his"""

    def __init__(self, n_users, n_items, user_his):
        self.n_users, self.n_items, self.user_his = n_users, n_items, user_his


N_USERS, N_ITEMS = 50, 300


def _model(name, native, D=64, heads=4, seed=11):
    from whisprrec_amd.sasrec import SASRec
    from whisprrec_amd.tisasrec import TiSASRec
    args = argparse.Namespace(device=DEV, model_path="", buffer=1, num_neg=1, test_all=1, history_max=20, emb_size=D,
                              num_layers=1, num_heads=heads, dropout=0.0, time_max=32, ti_native=0, block_native=0, emb_lazy=0,
                              random_seed=3407, train_loss="softmax", softmax_native=native)
    rng = np.random.RandomState(seed)
    his = {u: [(1, int(x)) for x in np.cumsum(rng.randint(0, 50, 6))] for u in range(N_USERS)}
    torch.manual_seed(seed)
    model = {"SASRec": SASRec, "TiSASRec": TiSASRec}[name](args, _Corpus(N_USERS, N_ITEMS, his)).to(DEV)
    with torch.no_grad():
        # parameters away from their initial 0 / 1, tables at a scale where neither the attention nor the softmax is flat
        for n, p in model.named_parameters():
            if n.endswith("bias") or "layer_norm" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "embedding" in n:
                p.mul_(8)
    return model


def _batch(B, T, seed):
    rng = np.random.RandomState(seed)
    lengths = rng.randint(1, T + 1, B)
    lengths[:2] = [T, 1]
    valid = np.arange(T)[None, :] < lengths[:, None]
    hist = rng.randint(1, N_ITEMS, (B, T)) * valid
    times = (1_000_000 + np.cumsum(rng.randint(0, 400, (B, T)), axis=1)) * valid
    pos = rng.randint(1, N_ITEMS, B)
    pos[:B // 4] = pos[0]
    return {"history_items": _t(hist), "history_times": _t(times), "lengths": _t(lengths), "user_id": _t(rng.randint(0, N_USERS, B)),
            "pos_item": _t(pos), "neg_items": _t(rng.randint(1, N_ITEMS, (B, 1))), "batch_size": B, "phase": "train"}


def _other_tol(name, param):
    """the bound the block's own tests hold the parameter to (the same torch blocks run under both settings)"""
    if name == "SASRec":
        return K13.TOL["gqk" if ("q_linear" in param or "k_linear" in param) else "gparam"]
    qk = any(s in param for s in ("q_linear", "k_linear", "time_k_embedding", "position_k_embedding"))
    return K25.TOL["gqk" if qk else "gv"]


@pytest.mark.parametrize("name", ["SASRec", "TiSASRec"])
def test_model_native_loss_agrees_with_the_stock_path(name):
    off, on = _model(name, 0), _model(name, 1)
    on.load_state_dict(off.state_dict())
    batch = _batch(40, 20, 3)
    res = {}
    for tag, m in (("off", off), ("on", on)):
        m.train()
        m.zero_grad()
        loss = m.predict(batch)
        loss.backward()
        res[tag] = (float(loss.detach()), {n: p.grad.detach().cpu().numpy().astype(np.float64) for n, p in m.named_parameters()})
    assert on._softmax_native_ok is True and off._softmax_native_ok is None
    named = np.zeros(N_ITEMS, bool)
    named[batch["pos_item"].cpu().numpy()] = True
    fig = {"loss": abs(res["on"][0] - res["off"][0]) / abs(res["off"][0])}
    kb, kw = "transformer_block.0.masked_attn_head.k_linear.bias", "transformer_block.0.masked_attn_head.k_linear.weight"
    tol = {"loss": R.TOL["loss"]}
    for n, g in res["off"][1].items():
        got = res["on"][1][n]
        if n == "item_embedding.weight":
            fig["gE_in"], fig["gE_out"] = R.rel_err(got[named], g[named]), R.rel_err(got[~named], g[~named])
            tol["gE_in"], tol["gE_out"] = R.TOL["gE_in"], R.TOL["gE_out"]
            assert not got[0].any()
        elif n == kb:                   # mathematically zero: absolutely, against the weight's (tests/sasblock_ref.py)
            fig[n] = float(np.max(np.abs(got - g))) / float(np.max(np.abs(res["off"][1][kw])))
            tol[n] = K13.TOL["gkb"] if name == "SASRec" else K25.TOL["gqk"]
        else:
            fig[n], tol[n] = R.rel_err(got, g), _other_tol(name, n)
    print("%s softmax_native 1 against 0: " % name + " ".join("%s %.1e" % (n.replace("transformer_block.0.", ""), v) for n, v in fig.items()))
    for n in fig:
        assert fig[n] < tol[n], (n, fig[n], tol[n])


def test_unsupported_embedding_size_warns_once_and_trains_on_the_stock_path(caplog):
    model = _model("SASRec", 1, D=48, heads=4)
    stock = _model("SASRec", 0, D=48, heads=4)
    stock.load_state_dict(model.state_dict())
    batch = _batch(16, 20, 4)
    model.train()
    stock.train()
    with caplog.at_level(logging.WARNING):
        first = model.predict(batch)
        first.backward()
        model.predict(batch)
    assert [r.getMessage() for r in caplog.records if "softmax_native" in r.getMessage()] == [
        "--softmax_native 1: the loss kernel does not take emb_size=48; keeping the torch path"]
    assert model._softmax_native_ok is False
    assert torch.equal(first.detach(), stock.predict(batch).detach())
    assert model.item_embedding.weight.grad is not None and bool(torch.isfinite(model.item_embedding.weight.grad).all())


def test_a_positive_that_is_no_class_raises_at_once_or_when_training_ends():
    model = _model("SASRec", 1).train()
    batch = _batch(16, 20, 5)
    batch["pos_item"][3] = 0
    with pytest.raises(IndexError, match="outside"):
        model.predict(batch)
    model._trusted_indices = True             # as inside HipRunner.fit: no read-back per step
    try:
        assert bool(torch.isfinite(model.predict(batch)))
    finally:
        model._trusted_indices = False
    with pytest.raises(IndexError, match="item 0 is padding"):
        model.eval()
    assert not model.training                 # the mode changed although the check raised
    model.train()
    model.eval()                              # the word was cleared
    stock = _model("SASRec", 0).train()
    assert bool(torch.isinf(stock.predict(batch)))


def _argv(model, path, tmp, extra=()):
    return ["--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--dropout", "0.0", "--history_max", "20",
            "--time_max", "64", "--model_name", model, "--runner_name", "HipRunner", "--dataset", "ml-100k", "--path", path,
            "--epoch", "1", "--batch_size", "256", "--eval_batch_size", "512", "--optimizer", "Adam", "--lr", "1e-3", "--l2", "0.0",
            "--log_file", str(tmp / "log.txt"), "--model_path", str(tmp / "m.pt"), "--num_workers", "0", "--topk", "5,10",
            "--metric", "NDCG, HR", "--random_seed", "3407", "--train_loss", "softmax", "--seq_eval_native", "1"] + list(extra)


@pytest.fixture(scope="module")
def ml100k(tmp_path_factory):
    from test_reader import _write_inter
    tmp = tmp_path_factory.mktemp("softmax_loss")
    return {"path": _write_inter(np.load(os.path.join(GOLD, "g8_reader.npz")), tmp), "tmp": tmp, "corpus": {}}


def _fit_three_steps(ml100k, name, native):
    """one HipRunner.fit over the first three batches of the training frame -> (mean loss, model, runner, its parts)"""
    from whisprrec_amd import main as launcher
    args, model_class, reader_class, runner_class = launcher.build_args(
        _argv(name, ml100k["path"], ml100k["tmp"], ["--softmax_native", str(native)]))
    args.device = torch.device("cuda")
    if name not in ml100k["corpus"]:
        ml100k["corpus"][name] = reader_class(args).corpus()
    corpus = ml100k["corpus"][name]
    launcher.init_seed(args.random_seed)
    model = model_class(args, corpus).to(args.device)
    ds = model_class.Dataset(model, corpus, "train")
    rows = np.flatnonzero(np.asarray(ds.data["item_id"]) != 0)[:3 * 256]     # the reader numbers items from 0; item 0 is no class
    ds.data = {k: np.asarray(v)[rows] for k, v in ds.data.items()}
    launcher.init_seed(7)
    run = runner_class(args)
    return run.fit(ds, epoch=1), model, run, (args, model_class, corpus)


@pytest.mark.parametrize("name", ["SASRec", "TiSASRec"])
def test_three_fit_steps_agree_and_the_device_evaluation_runs(ml100k, name):
    """Bound: step k's loss inherits, to first order, lr * |g|_1 * (the gradient tolerances) from the k steps before it, far
    below the loss tolerance itself; the mean of three steps is held to 3 x TOL["loss"]."""
    stock, _, _, _ = _fit_three_steps(ml100k, name, 0)
    native, model, run, (args, model_class, corpus) = _fit_three_steps(ml100k, name, 1)
    assert model._softmax_native_ok is True
    print("%s three fit steps: stock %.7f native %.7f" % (name, stock, native))
    assert np.isfinite(native) and abs(native - stock) / abs(stock) < 3 * R.TOL["loss"]
    assert abs(native - np.log(model.item_num - 1)) < 0.5                    # an untrained model: near log(classes)
    dev = model_class.Dataset(model, corpus, "dev")
    dev.data = {k: np.asarray(v)[:200] for k, v in dev.data.items()}
    assert run._seq_eval_ok(dev)
    res = run.evaluate(dev, [5, 10], ["NDCG", "HR"])
    assert set(res) == {"NDCG@5", "HR@5", "NDCG@10", "HR@10"} and all(0.0 <= v <= 1.0 for v in res.values())
    items, _ = run.recommend_rows(dev, 5, rows=[0, 7])
    assert items.shape == (2, 5)
