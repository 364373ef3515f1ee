"""The whole-sequence GRU (K27: wr_gru_seq_fwd / _bwd) and NARM's attention pooling (K28: wr_narm_pool_fwd / _bwd) on the device
against the float64 restatements of tests/narm_ref.py under the tolerances measured there, bit for bit against themselves and
against gru_last, and through NARM, GRU4Rec --num_layers 2, HipRunner and the launcher.
Run with -rP for the `parity narm` lines."""
import copy
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_ref as G  # noqa: E402
import narm_ref as R  # noqa: E402
from whisprrec_amd import hip_ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRU = ("wih", "whh", "bih", "bhh")
POOL = ("hs", "hg", "A1", "A2", "v")
_SEQ, _POOL = {}, {}


def _seq(key):
    """(inputs, {with g_last: float64 result}) of a gru_seq case, computed once"""
    if key not in _SEQ:
        c = R.make_seq_case(*key)
        _SEQ[key] = (c, {wl: R.seq_case_f64(c, wl) for wl in (False, True)})
    return _SEQ[key]


def _pool(key):
    if key not in _POOL:
        c = R.make_pool_case(*key)
        _POOL[key] = (c, R.pool_case_f64(c))
    return _POOL[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _pad(c, T):
    return np.arange(T)[None, :] >= np.clip(c["lengths"], 0, T)[:, None]


def _run_seq(c, with_last=False):
    """gru_seq_fwd and gru_seq_bwd -> dict(hs, gx, gwih, gwhh, gbih, gbhh) of numpy arrays"""
    args = [_t(c["x"]), _t(c["lengths"])] + [_t(c[n]) for n in GRU]
    hs = hip_ops.gru_seq_fwd(*args)
    grads = hip_ops.gru_seq_bwd(*args, hs, _t(c["ghs"]), _t(c["glast"]) if with_last else None)
    res = {"hs": hs.cpu().numpy()}
    res.update({n: g.cpu().numpy() for n, g in zip(("gx", "gwih", "gwhh", "gbih", "gbhh"), grads)})
    return res


def _run_last(c):
    """gru_fwd(save_hs=True) and gru_bwd -> dict(h, hs, gx, ...)"""
    args = [_t(c["x"]), _t(c["lengths"])] + [_t(c[n]) for n in GRU]
    h, hs = hip_ops.gru_fwd(*args, save_hs=True)
    grads = hip_ops.gru_bwd(*args, hs, _t(c["glast"]))
    res = {"h": h.cpu().numpy(), "hs": hs.cpu().numpy()}
    res.update({n: g.cpu().numpy() for n, g in zip(("gx", "gwih", "gwhh", "gbih", "gbhh"), grads)})
    return res


def _run_pool(c):
    """narm_pool under autograd -> dict(c, ghs, ghg, gA1, gA2, gv)"""
    leaves = {n: _t(c[n]).requires_grad_(True) for n in POOL}
    out = hip_ops.narm_pool(leaves["hs"], leaves["hg"], _t(c["lengths"]), leaves["A1"], leaves["A2"], leaves["v"])
    out.backward(_t(c["gc"]))
    res = {"c": out.detach().cpu().numpy()}
    res.update({"g" + n: leaves[n].grad.cpu().numpy() for n in POOL})
    return res


# ------------------------------------------------------------------------------------------------ gru_seq
@pytest.mark.parametrize("key", R.SEQ_CASES, ids=[R.seq_id(k) for k in R.SEQ_CASES])
def test_gru_seq_parity_with_float64(key):
    c, ref = _seq(key)
    B, T, E = c["x"].shape
    assert hip_ops.gru_supports(E, c["whh"].shape[1], T)
    pad = _pad(c, T)
    if key[1] == "mixed" and B > 1:
        assert pad.any()
    for with_last in (False, True):
        got = _run_seq(c, with_last)
        fig = R.seq_figures(got, ref[with_last])
        print(R.seq_fmt("%s%s" % (R.seq_id(key), " + g_last" if with_last else ""), fig))
        w = R.seq_worst(fig)
        for g in R.SEQ_GROUPS:
            assert w[g] < R.SEQ_TOL[g], (g, with_last, w[g], fig)
        assert not got["hs"][pad].any() and not got["gx"][pad].any()          # exactly zero past every row's length


@pytest.mark.parametrize("key", [(2, "mixed", False), (5, "mixed", False), (0, "mixed", True)], ids=lambda k: R.seq_id(k))
def test_gru_seq_two_identical_calls_give_equal_bits(key):
    c, _ = _seq(key)
    a, b = _run_seq(c, True), _run_seq(c, True)
    for n in a:
        assert _same_bits(a[n], b[n]), n


@pytest.mark.parametrize("key", [(2, "mixed", False), (4, "mixed", False), (3, "full", False), (0, "mixed", True)],
                         ids=lambda k: R.seq_id(k))
def test_gru_seq_ties_to_gru_last_bit_for_bit(key):
    c, _ = _seq(key)
    B, T, _ = c["x"].shape
    live, rows = ~_pad(c, T), np.arange(B)
    last = _run_last(c)
    zero = _run_seq(dict(c, ghs=np.zeros_like(c["ghs"])), with_last=True)          # g_hs = 0, g_last = g
    assert _same_bits(zero["hs"][live], last["hs"][live])
    assert _same_bits(zero["hs"][rows, c["lengths"] - 1], last["h"])
    only = np.zeros_like(c["ghs"])
    only[rows, c["lengths"] - 1] = c["glast"]
    at_last = _run_seq(dict(c, ghs=only))                                          # g_hs = g at [b, len_b - 1] alone, no g_last
    for n in ("gx", "gwih", "gwhh", "gbih", "gbhh"):
        assert _same_bits(zero[n], last[n]), n
        assert _same_bits(at_last[n], last[n]), n


@pytest.mark.parametrize("key", [(2, "mixed", False), (3, "mixed", False), (4, "mixed", False)], ids=lambda k: R.seq_id(k))
def test_gru_seq_never_reads_the_padding(key):
    """NaN in x and in g_hs at t >= lengths[b]: bitwise the results without"""
    c, _ = _seq(key)
    pad = _pad(c, c["x"].shape[1])
    assert pad.any()
    d = dict(c, x=c["x"].copy(), ghs=c["ghs"].copy())
    d["x"][pad] = np.nan
    d["ghs"][pad] = np.nan
    a, b = _run_seq(c, True), _run_seq(d, True)
    for n in a:
        assert np.isfinite(b[n]).all(), n
        assert _same_bits(a[n], b[n]), n


def test_gru_seq_lengths_are_clamped():
    c, _ = _seq((2, "mixed", False))                 # B = 17, T = 20
    d = dict(c, lengths=c["lengths"].copy())
    d["lengths"][[2, 16]] = 0                        # one row inside the full tile, and the only row of the last tile
    d["lengths"][1] = 10_000                         # row 1 is T long already
    d["lengths"][3] = -4
    e = dict(d, lengths=np.clip(d["lengths"], 0, 20))
    got, same = _run_seq(d, True), _run_seq(e, True)
    for n in got:
        assert _same_bits(got[n], same[n]), n
    w = R.seq_worst(R.seq_figures(got, R.seq_case_f64(e, True)))
    for g in R.SEQ_GROUPS:
        assert w[g] < R.SEQ_TOL[g], (g, w[g])
    for row in (2, 3, 16):
        assert not got["hs"][row].any() and not got["gx"][row].any()
    d["lengths"][:] = 0                              # every row at length 0: nothing at all
    got = _run_seq(d, True)
    for n in got:
        assert not got[n].any(), n


def test_gru_seq_under_autograd_is_the_direct_call():
    c, _ = _seq((4, "mixed", False))
    leaves = {n: _t(c[n]).requires_grad_(True) for n in ("x",) + GRU}
    hs = hip_ops.gru_seq(leaves["x"], _t(c["lengths"]).to(torch.int32), *(leaves[n] for n in GRU))
    hs.backward(_t(c["ghs"]))
    direct = _run_seq(c)
    assert _same_bits(hs.detach().cpu().numpy(), direct["hs"])
    for n in ("x",) + GRU:
        assert _same_bits(leaves[n].grad.cpu().numpy(), direct["g" + n]), n


# ------------------------------------------------------------------------------------------------ the pooling
@pytest.mark.parametrize("key", R.POOL_CASES, ids=[R.pool_id(k) for k in R.POOL_CASES])
def test_pool_parity_with_float64(key):
    c, ref = _pool(key)
    B, T, H, A = R.POOL_SHAPES[key[0]]
    assert hip_ops.narm_pool_supports(H, A, T)
    pad = _pad(c, T)
    if key[1] == "mixed" and B > 1:
        assert pad.any()
    got = _run_pool(c)
    fig = R.pool_figures(got, ref)
    print(R.pool_fmt(R.pool_id(key), fig))
    w = R.pool_worst(fig)
    for g in R.POOL_GROUPS:
        assert w[g] < R.POOL_TOL[g], (g, w[g], fig)
    assert not got["ghs"][pad].any()                                          # exactly zero past every row's length


@pytest.mark.parametrize("key", [(2, "mixed"), (3, "full"), (4, "mixed"), (5, "mixed")], ids=lambda k: R.pool_id(k))
def test_pool_two_identical_calls_give_equal_bits(key):
    c, _ = _pool(key)
    a, b = _run_pool(c), _run_pool(c)
    for n in a:
        assert _same_bits(a[n], b[n]), n


@pytest.mark.parametrize("key", [(2, "mixed"), (3, "mixed"), (4, "mixed"), (5, "mixed")], ids=lambda k: R.pool_id(k))
def test_pool_never_reads_the_padding(key):
    c, _ = _pool(key)
    pad = _pad(c, c["hs"].shape[1])
    assert pad.any()
    d = dict(c, hs=c["hs"].copy())
    d["hs"][pad] = np.nan
    z = dict(c, hs=np.where(pad[:, :, None], 0.0, c["hs"]).astype(np.float32))
    a, b, e = _run_pool(c), _run_pool(d), _run_pool(z)
    for n in a:
        if n == "ghs":
            continue
        assert np.isfinite(b[n]).all(), n
        assert _same_bits(a[n], b[n]) and _same_bits(a[n], e[n]), n
    assert _same_bits(a["ghs"], e["ghs"]) and _same_bits(a["ghs"], b["ghs"]) and not b["ghs"][pad].any()


def test_pool_lengths_are_clamped():
    c, _ = _pool((2, "mixed"))                       # B = 17, T = 20: four full groups of 4 rows and one row more
    d = dict(c, lengths=c["lengths"].copy())
    d["lengths"][[2, 16]] = 0
    d["lengths"][1] = 10_000
    d["lengths"][3] = -4
    e = dict(d, lengths=np.clip(d["lengths"], 0, 20))
    got, same = _run_pool(d), _run_pool(e)
    for n in got:
        assert _same_bits(got[n], same[n]), n
    w = R.pool_worst(R.pool_figures(got, R.pool_case_f64(e)))
    for g in R.POOL_GROUPS:
        assert w[g] < R.POOL_TOL[g], (g, w[g])
    for row in (2, 3, 16):
        assert not got["c"][row].any() and not got["ghs"][row].any() and not got["ghg"][row].any()
    d["lengths"][:] = 0
    got = _run_pool(d)
    for n in got:
        assert not got[n].any(), n


def test_unsupported_shapes_are_refused_with_the_numbers():
    z = lambda *s: torch.zeros(*s, device=DEV)      # noqa: E731
    n = torch.ones(2, dtype=torch.int64, device=DEV)
    with pytest.raises(hip_ops.abi.WhisprRecHipError, match="H=64 A=48"):
        hip_ops.narm_pool_fwd(z(2, 20, 64), z(2, 64), n, z(48, 64), z(48, 64), z(48))
    with pytest.raises(hip_ops.abi.WhisprRecHipError, match="H=128 A=16"):
        hip_ops.narm_pool(z(2, 20, 128), z(2, 128), n, z(16, 128), z(16, 128), z(16))
    with pytest.raises(hip_ops.abi.WhisprRecHipError, match="E=128 H=64"):
        hip_ops.gru_seq(z(2, 20, 128), n, z(192, 128), z(192, 64), z(192), z(192))
    assert not hip_ops.narm_pool_supports(64, 8, 20) and hip_ops.narm_pool_supports(32, 64, 5000)
    assert hip_ops.narm_pool_workspace_bytes(4096, 200, 64, 16) == hip_ops.narm_pool_workspace_bytes(1, 1, 64, 16)


# ------------------------------------------------------------------------------------------------ the model
def _argv(path, tmp, model="NARM", extra=()):
    return ["--emb_size", "64", "--hidden_size", "64", "--history_max", "20", "--model_name", model, "--runner_name",
            "HipRunner", "--dataset", "ml-100k", "--path", path, "--epoch", "1", "--batch_size", "1024", "--eval_batch_size", "512",
            "--optimizer", "Adam", "--lr", "1e-3", "--l2", "0.0", "--log_file", str(tmp / "log.txt"), "--model_path",
            str(tmp / "m.pt"), "--num_workers", "0", "--topk", "5,10", "--metric", "NDCG, HR", "--random_seed", "3407"] + list(extra)


NATIVE = ["--gru_native", "1", "--pool_native", "1"]


@pytest.fixture(scope="module")
def ml100k(tmp_path_factory):
    from test_reader import _write_inter
    from whisprrec_amd import main as launcher
    tmp = tmp_path_factory.mktemp("narm")
    path = _write_inter(np.load(os.path.join(GOLD, "g8_reader.npz")), tmp)
    args, model_class, reader_class, runner_class = launcher.build_args(_argv(path, tmp, extra=NATIVE + ["--seq_eval_native", "1"]))
    args.device = torch.device("cuda")
    corpus = reader_class(args).corpus()
    return {"args": args, "model_class": model_class, "reader_class": reader_class, "runner_class": runner_class, "corpus": corpus,
            "tmp": tmp, "path": path}


def _pair(ml100k, model_class=None, args=None, **over):
    """the model with the native flags off and on from one state_dict"""
    from whisprrec_amd import main as launcher
    args = ml100k["args"] if args is None else args
    model_class = ml100k["model_class"] if model_class is None else model_class
    models = {}
    for flag in (0, 1):
        a = copy.copy(args)
        a.gru_native = a.pool_native = flag
        for k, v in over.items():
            setattr(a, k, v)
        launcher.init_seed(args.random_seed)
        models[flag] = model_class(a, ml100k["corpus"]).to(DEV)
    models[1].load_state_dict(models[0].state_dict())
    with torch.no_grad():
        for m in models.values():
            m.item_embedding.weight.mul_(8)          # a scale at which the gates leave their linear range
    return models


def _train_batch(model, ml100k, rows):
    ds = type(model).Dataset(model, ml100k["corpus"], "train")
    ds.actions_before_epoch()
    batch = ds.collate_batch([ds[i] for i in rows])
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def _first_step(models, batch):
    """{flag: (loss, {name: gradient})}"""
    out = {}
    for f, m in models.items():
        m.train()
        m.zero_grad()
        loss = m.predict(batch)
        loss.backward()
        out[f] = (float(loss.detach()), {n: p.grad.cpu().numpy() for n, p in m.named_parameters()})
    return out


def _three_adam_steps(models, batches):
    losses = {}
    for f, m in models.items():
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        m.train()
        losses[f] = []
        for batch in batches:
            opt.zero_grad()
            loss = m.predict(batch)
            loss.backward()
            opt.step()
            losses[f].append(float(loss.detach()))
    return losses, [abs(a - b) / abs(b) for a, b in zip(losses[1], losses[0])]


@pytest.mark.parametrize("train_loss", ["bpr", "softmax"])
def test_model_native_paths_agree_with_the_stock_paths(ml100k, train_loss):
    """--gru_native 1 --pool_native 1 against both off from one state_dict (B = 64, ml-100k rows): the first step's loss and every
    parameter's gradient within MODEL_TOL, the losses of three Adam steps to 1e-5 relative, DESIGN section 2's bar for fp32
    losses"""
    from whisprrec_amd import main as launcher
    models = _pair(ml100k, train_loss=train_loss)
    launcher.init_seed(5)
    batches = [_train_batch(models[0], ml100k, range(64 * k, 64 * k + 64)) for k in range(3)]
    assert len({int(x) for x in batches[0]["lengths"]}) > 3          # rows of several lengths
    step = _first_step(models, batches[0])
    assert models[1]._gru_native_ok and all(models[1]._gru_native_ok.values()), "the GRU kernels refused the test's shape"
    assert models[1]._pool_native_ok and all(models[1]._pool_native_ok.values()), "the pooling kernels refused the test's shape"
    assert not models[0]._gru_native_ok and not models[0]._pool_native_ok
    w, per = R.model_figures(step[1][0], step[1][1], step[0][0], step[0][1])
    print(R.model_fmt("%s native against flag-off" % train_loss, w), {n: "%.1e" % v for n, v in per.items()})
    assert len(per) == 13
    for g in R.MODEL_GROUPS:
        assert w[g] < R.MODEL_TOL[g], (g, w[g], per)
    losses, rel = _three_adam_steps(models, batches)
    print("parity narm model %s three Adam steps, losses native %s stock %s, relative %s" % (train_loss, losses[1], losses[0],
                                                                                          ["%.1e" % r for r in rel]))
    assert all(r < 1e-5 for r in rel), rel


def test_each_flag_alone(ml100k):
    """one flag on, the other off: the nn.GRU states past a row's length are not zero, and the pooling kernel never reads them"""
    from whisprrec_amd import main as launcher
    launcher.init_seed(5)
    ref = None
    for gru_native, pool_native in ((0, 0), (1, 0), (0, 1)):
        a = copy.copy(ml100k["args"])
        a.gru_native, a.pool_native = gru_native, pool_native
        launcher.init_seed(a.random_seed)
        m = ml100k["model_class"](a, ml100k["corpus"]).to(DEV)
        with torch.no_grad():
            m.item_embedding.weight.mul_(8)
        if ref is None:
            batch = _train_batch(m, ml100k, range(64))
        step = _first_step({0: m}, batch)[0]
        if ref is None:
            ref = step
            continue
        w, per = R.model_figures(step[0], step[1], ref[0], ref[1])
        print(R.model_fmt("gru_native %d pool_native %d against flag-off" % (gru_native, pool_native), w))
        for g in R.MODEL_GROUPS:
            assert w[g] < R.MODEL_TOL[g], (g, w[g], per)


def test_unsupported_sizes_are_logged_once_and_keep_the_stock_path(ml100k, caplog):
    from whisprrec_amd import main as launcher
    a = copy.copy(ml100k["args"])
    a.hidden_size, a.attention_size = 48, 8
    launcher.init_seed(a.random_seed)
    m = ml100k["model_class"](a, ml100k["corpus"]).to(DEV)
    batch = _train_batch(m, ml100k, range(16))
    other = dict(batch, history_items=batch["history_items"][:, :7].contiguous(), lengths=batch["lengths"].clamp(max=7))
    with caplog.at_level(logging.WARNING):
        for fd in (batch, other, batch):
            loss = m.predict(fd)
    assert torch.isfinite(loss)
    assert set(m._gru_native_ok.values()) == {False} and set(m._pool_native_ok.values()) == {False} and len(m._gru_native_ok) == 2
    text = [r.getMessage() for r in caplog.records]
    assert sum("--gru_native 1" in t and "hidden_size=48" in t for t in text) == 1
    assert sum("--pool_native 1" in t and "attention_size=8" in t for t in text) == 1


def test_device_evaluation_returns_the_host_ranks(ml100k, monkeypatch):
    from whisprrec_amd import main as launcher, runner
    args, model_class, corpus = ml100k["args"], ml100k["model_class"], ml100k["corpus"]
    launcher.init_seed(args.random_seed)
    model = model_class(args, corpus).to(args.device)
    with torch.no_grad():
        model.item_embedding.weight.mul_(30)                               # scores that spread: few near-ties
    ds = model_class.Dataset(model, corpus, "dev")
    ds.data = {k: np.asarray(v)[:200] for k, v in ds.data.items()}
    host_run = runner.BaseRunner(args)
    pred = host_run.interface(ds).astype(np.float64)
    target, S = pred[:, 0], pred[:, 1:].copy()
    S[np.arange(len(ds)), np.asarray(ds.data["item_id"])] = np.nan
    fin = np.isfinite(S)
    margin = np.where(fin, np.abs(S - target[:, None]), np.inf).min(axis=1)
    ok = margin > 1e-5 * np.abs(S[fin]).max()
    assert ok.mean() >= 0.9
    ds.data = {k: np.asarray(v)[ok] for k, v in ds.data.items()}          # the rows without a near-tie: their ranks are decided
    n = int(ok.sum())
    host_rank = np.argwhere((-pred[ok]).argsort(axis=1) == 0)[:, 1] + 1
    host_metrics = host_run.evaluate(ds, [5, 10], ["NDCG", "HR"])
    run = ml100k["runner_class"](args)
    monkeypatch.setattr(runner.BaseRunner, "interface", lambda *a: pytest.fail("the host path ran"))
    assert run._seq_eval_ok(ds)
    rank = run.rank_rows(ds)
    print("narm device evaluation: rows kept %.3f, ranks differing on them %d" % (ok.mean(), int((rank != host_rank).sum())))
    assert rank.shape == (n,) and np.array_equal(rank, host_rank)
    res = run.evaluate(ds, [5, 10], ["NDCG", "HR"])
    print("narm device evaluation: metrics device %s host %s" % (res, host_metrics))
    assert set(res) == {"NDCG@5", "HR@5", "NDCG@10", "HR@10"} == set(host_metrics)
    assert all(abs(res[k] - host_metrics[k]) < 1e-6 for k in res), (res, host_metrics)       # the device path's own reduction
    assert 0 < res["HR@10"] < 1 or len(set(rank)) > 1                      # ranks that differ: the cut at k matters
    items, _ = run.recommend_rows(ds, 5, rows=[0, 7])
    users, pos = np.asarray(ds.data["user_id"]), np.asarray(ds.data["position"])
    his = [corpus.user_his[users[r]][:pos[r]] for r in (0, 7)]
    nx, _ = run.recommend_next(model, corpus, [[x[0] for x in h] for h in his], 5, users=users[[0, 7]])
    assert items.shape == (2, 5) and np.array_equal(items, nx)


def test_row_lazy_native_paths_agree_with_the_stock_paths(ml100k):
    """--emb_lazy 1 on both sides, --gru_native 1 --pool_native 1 against both off from one state_dict: the first step's loss and
    every dense parameter's gradient within MODEL_TOL (the item table gets no dense gradient), the losses of three steps through
    the models' RowLazyOptimizer to 1e-5 relative (the later losses see the row-lazy table's updates)"""
    from whisprrec_amd import main as launcher
    from whisprrec_amd.sasrec import RowLazyOptimizer
    models = _pair(ml100k, emb_lazy=1)
    assert all(m.emb_lazy and isinstance(m.optimizer, RowLazyOptimizer) for m in models.values())
    launcher.init_seed(5)
    batches = [_train_batch(models[0], ml100k, range(64 * k, 64 * k + 64)) for k in range(3)]
    losses, first = {}, {}
    for f, m in models.items():
        m.train()
        losses[f] = []
        for k, batch in enumerate(batches):
            m.optimizer.zero_grad()
            loss = m.predict(batch)
            loss.backward()
            if k == 0:
                assert m.item_embedding.weight.grad is None
                first[f] = {n: p.grad.cpu().numpy() for n, p in m.named_parameters() if n != "item_embedding.weight"}
            m.optimizer.step()
            losses[f].append(float(loss.detach()))
    assert all(models[1]._gru_native_ok.values()) and all(models[1]._pool_native_ok.values()) and models[1]._pool_native_ok
    assert not models[0]._gru_native_ok and not models[0]._pool_native_ok
    w, per = R.model_figures(losses[1][0], first[1], losses[0][0], first[0])
    print(R.model_fmt("emb_lazy native against flag-off", w), {n: "%.1e" % v for n, v in per.items()})
    assert len(per) == 12
    for g in R.MODEL_GROUPS:
        assert w[g] < R.MODEL_TOL[g], (g, w[g], per)
    rel = [abs(a - b) / abs(b) for a, b in zip(losses[1], losses[0])]
    print("parity narm model emb_lazy three steps, losses native %s stock %s, relative %s" % (losses[1], losses[0],
                                                                                           ["%.1e" % r for r in rel]))
    assert all(r < 1e-5 for r in rel), rel


def test_row_lazy_item_table_trains(ml100k, tmp_path):
    from whisprrec_amd import main as launcher
    from whisprrec_amd.sasrec import RowLazyOptimizer
    args, model_class, reader_class, runner_class = launcher.build_args(_argv(ml100k["path"], tmp_path, extra=NATIVE + ["--emb_lazy", "1"]))
    args.device = torch.device("cuda")
    launcher.init_seed(args.random_seed)
    model = model_class(args, ml100k["corpus"]).to(args.device)
    assert model.emb_lazy and isinstance(model.optimizer, RowLazyOptimizer)
    before = model.item_embedding.weight.detach().clone()
    ds = model_class.Dataset(model, ml100k["corpus"], "train")
    loss = runner_class(args).fit(ds, epoch=1)
    assert np.isfinite(loss) and 0.0 < loss < 1.0
    assert all(model._gru_native_ok.values()) and all(model._pool_native_ok.values()) and model._pool_native_ok
    assert model.item_embedding.weight.grad is None                        # no dense gradient was built
    model.eval()
    assert (model.item_embedding.weight.detach() != before).any(dim=1)[1:].any()      # the flushed table holds moved rows


def test_launcher_runs_one_epoch_end_to_end(ml100k, tmp_path):
    from whisprrec_amd import main as launcher
    argv = _argv(ml100k["path"], tmp_path, extra=NATIVE + ["--seq_eval_native", "1", "--save_rec", "5"])
    res = launcher.main(argv)
    assert "NDCG@5" in res and "HR@10" in res
    assert os.path.exists(os.path.join(ml100k["path"], "ml-100k", "rec-NARM.csv"))
    assert os.path.exists(str(tmp_path / "m.pt"))


# ------------------------------------------------------------------------------------------------ GRU4Rec --num_layers 2
def test_gru4rec_two_layers_native_agrees_with_the_stock_path(ml100k, tmp_path):
    """layer 0 through gru_seq, layer 1 through gru_last, against nn.GRU(num_layers=2): the loss to 1e-5 relative, the gradient of
    every nn.GRU parameter within gru_ref's tolerances of its group; two runs give equal bits"""
    from whisprrec_amd import main as launcher
    args, model_class, _, _ = launcher.build_args(_argv(ml100k["path"], tmp_path, "GRU4Rec", ["--num_layers", "2", "--emb_size", "32"]))
    args.device = torch.device("cuda")
    models = {}
    for flag in (0, 1):
        a = copy.copy(args)
        a.gru_native = flag
        launcher.init_seed(args.random_seed)
        models[flag] = model_class(a, ml100k["corpus"]).to(DEV)
    models[1].load_state_dict(models[0].state_dict())
    with torch.no_grad():
        for m in models.values():
            m.item_embedding.weight.mul_(8)
    launcher.init_seed(5)
    batch = _train_batch(models[0], ml100k, range(64))
    step = _first_step(models, batch)
    assert models[1]._gru_native_ok == {batch["history_items"].shape[1]: True}
    names = [n for n in step[0][1] if n.startswith("rnn.")]
    assert len(names) == 8
    err = {n: R.rel_err(step[1][1][n], step[0][1][n]) for n in step[0][1]}
    rel = abs(step[1][0] - step[0][0]) / abs(step[0][0])
    print("parity narm gru4rec two layers: loss %.2e (tol 1e-05) " % rel + " ".join("%s %.2e" % (n, v) for n, v in err.items()))
    assert rel < 1e-5
    for n in names:
        assert err[n] < G.TOL["gw" if "weight" in n else "gb"], (n, err[n])
    again = _first_step({1: models[1]}, batch)[1]
    assert again[0] == step[1][0]
    for n in again[1]:
        assert _same_bits(again[1][n], step[1][1][n]), n
