"""Time-interval attention on the device (K25: wr_ti_attention_fwd / _bwd) against the float64 restatement of tests/tisas_ref.py
under the tolerances measured there, bit for bit against itself, and through TiSASRec, HipRunner and the launcher.
Run with -rP for the `parity ti_attention` lines."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tisas_ref as R  # noqa: E402
from whisprrec_amd import hip_ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CASES = {}


def _case(i, pattern):
    """(inputs, float64 result) of SHAPES[i] with this time pattern, computed once"""
    key = (i, pattern)
    if key not in _CASES:
        c = R.make_case(i, pattern)
        _CASES[key] = (c, R.case_f64(c))
    return _CASES[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(c, err_word=None, min_interval=None):
    """forward and backward through hip_ops.ti_attention under autograd -> dict(out, gq, gk, gv, gtk, gtv) of numpy arrays"""
    leaves = {n: _t(c[n]).requires_grad_(True) for n in ("q", "k", "v", "tk", "tv")}
    m = _t(c["min_interval"] if min_interval is None else min_interval)
    out = hip_ops.ti_attention(leaves["q"], leaves["k"], leaves["v"], _t(c["times"]), m, leaves["tk"], leaves["tv"], c["heads"],
                               c["time_max"], err_word=err_word)
    out.backward(_t(c["gout"]))
    res = {"out": out.detach().cpu().numpy()}
    for n in ("q", "k", "v", "tk", "tv"):
        res["g" + n] = leaves[n].grad.cpu().numpy()
    return res


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=["x".join(map(str, s)) for s in R.SHAPES])
def test_parity_with_float64(shape, pattern):
    c, ref = _case(shape, pattern)
    B, T, D, heads, time_max = R.SHAPES[shape]
    assert hip_ops.ti_attention_supports(D, heads, T, time_max)
    got = _run(c)
    fig = R.figures(got, ref)
    print(R.fmt("%s %s" % (R.SHAPES[shape], pattern), fig))
    w = R.worst(fig)
    for g in R.GROUPS:
        assert w[g] < R.TOL[g], (g, w[g], fig)
    # rows of the tables no pair lands on receive exactly nothing
    used = np.zeros(time_max + 1, bool)
    used[np.unique(R.intervals(c["times"], c["min_interval"], time_max)[:, np.tril(np.ones((T, T), bool))])] = True
    assert not got["gtk"][~used].any() and not got["gtv"][~used].any()


@pytest.mark.parametrize("shape,pattern", [(2, "equal"), (4, "far"), (5, "spread")])
def test_two_identical_calls_give_equal_bits(shape, pattern):
    c = R.make_case(shape, pattern)
    a, b = _run(c), _run(c)
    for n in a:
        assert np.array_equal(a[n].view(np.int32), b[n].view(np.int32)), n


# ------------------------------------------------------------------------------------------------ several visits per workgroup
def _walk_case(i, pattern):
    key = ("walk", i, pattern)
    if key not in _CASES:
        c = R.make_case(i, pattern, R.WALK_SHAPES, R.WALK_SEED)
        _CASES[key] = (c, R.case_f64(c))
    return _CASES[key]


def _assert_walk(tag, got, ref):
    fig = R.figures(got, ref)
    print(R.fmt("walk %s" % tag, fig, R.WALK_TOL))
    print("parity ti_attention walk %s visits (b < %d | later): %s" % (tag, R.BWD_WG, R.visit_fmt(R.visit_figures(got, ref, R.BWD_WG))))
    w = R.worst(fig)
    for g in R.GROUPS:
        assert w[g] < R.WALK_TOL[g], (g, w[g], fig)


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("shape", range(len(R.WALK_SHAPES)), ids=["x".join(map(str, s)) for s in R.WALK_SHAPES])
def test_walk_parity_with_float64(shape, pattern):
    """B above kTiBwdWg (and, at B = 4099, above kTiFwdWg): a workgroup of the backward adds the pairs of several sequences into
    its slab of the two table gradients"""
    c, ref = _walk_case(shape, pattern)
    B, T, D, heads, time_max = R.WALK_SHAPES[shape]
    assert hip_ops.ti_attention_supports(D, heads, T, time_max)
    got = _run(c)
    _assert_walk("%s %s" % (R.WALK_SHAPES[shape], pattern), got, ref)
    used = np.zeros(time_max + 1, bool)                                   # rows no pair lands on receive exactly nothing
    used[np.unique(R.intervals(c["times"], c["min_interval"], time_max)[:, np.tril(np.ones((T, T), bool))])] = True
    assert not got["gtk"][~used].any() and not got["gtv"][~used].any()
    if pattern == "equal":
        assert used.sum() == 1 and used[0]


def test_walk_two_identical_calls_give_equal_bits():
    """the shape with the most visits (16 - 17 per workgroup of the backward), every pair on row 0 of the tables"""
    c, _ = _walk_case(R.WALK_SHAPES.index((4099, 2, 32, 1, 4)), "equal")
    a, b = _run(c), _run(c)
    for n in a:
        assert np.array_equal(a[n].view(np.int32), b[n].view(np.int32)), n


def test_walk_bad_min_interval_on_a_later_visit_is_clamped_and_reported():
    """min_interval 0 and -7 at sequences b >= kTiBwdWg only: the error word is set, the result is that of the scale 1"""
    shape = R.WALK_SHAPES.index((259, 7, 32, 2, 8))
    c = dict(_walk_case(shape, "spread")[0])
    rng = np.random.RandomState(5)
    c["times"] = 1_000 + np.cumsum(rng.randint(0, 4, c["times"].shape), axis=1)     # gaps of a few units, as in the test below
    bad = c["min_interval"].copy()
    bad[[R.BWD_WG, R.BWD_WG + 2]] = [0, -7]
    assert (bad[:R.BWD_WG] >= 1).all()
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = _run(c, err_word=err, min_interval=bad)
    assert int(err.item()) == 1
    c["min_interval"] = np.maximum(bad, 1)
    _assert_walk("clamped scale", got, R.case_f64(c))
    err.zero_()
    _run(c, err_word=err)
    assert int(err.item()) == 0


def test_zero_min_interval_sets_the_error_word_and_is_clamped():
    c, _ = _case(1, "spread")
    c = dict(c)
    # gaps of a few units, so that a scale of 1 keeps quotients on both sides of the clamp
    rng = np.random.RandomState(5)
    c["times"] = 1_000 + np.cumsum(rng.randint(0, 4, c["times"].shape), axis=1)
    bad = c["min_interval"].copy()
    bad[[0, 3]] = [0, -7]
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = _run(c, err_word=err, min_interval=bad)
    assert int(err.item()) == 1
    c["min_interval"] = np.maximum(bad, 1)
    ref = R.case_f64(c)
    w = R.worst(R.figures(got, ref))
    print(R.fmt("clamped scale", R.figures(got, ref)))
    for g in R.GROUPS:
        assert w[g] < R.TOL[g], (g, w[g])
    err.zero_()
    _run(c, err_word=err)
    assert int(err.item()) == 0


def test_integer_division_where_float_division_rounds_up():
    c, _ = _case(1, "spread")
    c = dict(c)
    gap, m = 300 * 65535 - 1, 65535                                        # fp32: 300; integers: 299
    c["time_max"] = 512
    rng = np.random.RandomState(6)
    c["tk"], c["tv"] = (rng.standard_normal((513, c["q"].shape[2])).astype(np.float32) * 0.4 for _ in range(2))
    c["times"] = np.tile(1_000 + gap * np.arange(c["times"].shape[1], dtype=np.int64), (c["times"].shape[0], 1))
    c["min_interval"] = np.full(c["times"].shape[0], m, np.int64)
    assert R.intervals(c["times"], c["min_interval"], 512)[0, 1, 0] == 299
    got, ref = _run(c), R.case_f64(c)
    w = R.worst(R.figures(got, ref))
    for g in R.GROUPS:
        assert w[g] < R.TOL[g], (g, w[g])
    assert got["gtk"][299].any() and not got["gtk"][300].any()


def test_unsupported_shapes_are_refused_with_the_numbers():
    q = torch.zeros(2, 20, 128, device=DEV)
    tab = torch.zeros(513, 128, device=DEV)
    with pytest.raises(hip_ops.abi.WhisprRecHipError, match="D=128"):
        hip_ops.ti_attention_fwd(q, q, q, torch.zeros(2, 20, dtype=torch.int64, device=DEV),
                                 torch.ones(2, dtype=torch.int64, device=DEV), tab, tab, 4, 512)
    assert not hip_ops.ti_attention_supports(64, 8, 20, 512) and not hip_ops.ti_attention_supports(64, 4, 65, 512)
    assert hip_ops.ti_attention_workspace_bytes(4096, 64, 64, 4, 512) == hip_ops.ti_attention_workspace_bytes(1, 1, 64, 4, 512)


# ------------------------------------------------------------------------------------------------ the model
class _Corpus:
    """what TiSASRec reads from a reader: sizes and user_his"""

    def __init__(self, n_users, n_items, user_his):
        self.n_users, self.n_items, self.user_his = n_users, n_items, user_his


def _model(ti_native, history_max, time_max, n_users=50, n_items=300, dropout=0.0, D=64, heads=4, seed=11):
    from whisprrec_amd.tisasrec import TiSASRec
    args = argparse.Namespace(device=DEV, model_path="", buffer=1, num_neg=1, test_all=1, history_max=history_max, emb_size=D,
                              num_layers=1, num_heads=heads, dropout=dropout, time_max=time_max, ti_native=ti_native, emb_lazy=0,
                              random_seed=3407)
    rng = np.random.RandomState(seed)
    his = {u: [(1, int(t)) for t in np.cumsum(rng.randint(0, 50, 6))] for u in range(n_users)}
    torch.manual_seed(seed)
    model = TiSASRec(args, _Corpus(n_users, n_items, his)).to(DEV)
    with torch.no_grad():
        # parameters away from their initial 0 / 1, tables at a scale where the attention is not flat
        for n, p in model.named_parameters():
            if n.endswith("bias") or "layer_norm" in n:
                p.add_(0.05 * torch.randn_like(p))
            elif "embedding" in n:
                p.mul_(8)
    return model


def _batch(B, T, n_users, n_items, seed, full=False):
    rng = np.random.RandomState(seed)
    lengths = np.full(B, T) if full else rng.randint(1, T + 1, B)
    lengths[:2] = [T, 1]
    valid = np.arange(T)[None, :] < lengths[:, None]
    hist = rng.randint(1, n_items, (B, T)) * valid
    times = (1_000_000 + np.cumsum(rng.randint(0, 400, (B, T)), axis=1)) * valid
    return {"history_items": _t(hist), "history_times": _t(times), "lengths": _t(lengths), "user_id": _t(rng.randint(0, n_users, B)),
            "pos_item": _t(rng.randint(1, n_items, B)), "neg_items": _t(rng.randint(1, n_items, (B, 1))), "batch_size": B,
            "phase": "train"}


def _qk_group(name):
    return any(s in name for s in ("q_linear", "k_linear", "time_k_embedding", "position_k_embedding"))


def test_model_native_path_agrees_with_the_torch_path():
    """g15-sized input: B = 12, T = 20, D = 64, 4 heads, time_max = 32; loss and every parameter gradient"""
    off, on = _model(0, 20, 32), _model(1, 20, 32)
    on.load_state_dict(off.state_dict())
    batch = _batch(12, 20, 50, 300, 3)
    res = {}
    for tag, m in (("off", off), ("on", on)):
        m.train()
        m.zero_grad()
        loss = m.predict(batch)
        loss.backward()
        res[tag] = (float(loss.detach()), {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()})
    assert on._ti_native_ok == {20: True}, "the attention kernels refused the test's shape"
    on.check_train_extras()
    fig = {"loss": abs(res["on"][0] - res["off"][0]) / abs(res["off"][0])}
    kb, kw = "transformer_block.0.masked_attn_head.k_linear.bias", "transformer_block.0.masked_attn_head.k_linear.weight"
    for n, g in res["off"][1].items():
        if n == kb:                   # mathematically zero: absolutely, against the weight's (tests/sasblock_ref.py)
            fig[n] = float(np.max(np.abs(res["on"][1][n] - g))) / float(np.max(np.abs(res["off"][1][kw])))
        else:
            fig[n] = R.rel_err(res["on"][1][n], g)
    print("model ti_native 1 against 0: " + " ".join("%s %.1e" % (n.replace("transformer_block.0.", ""), v) for n, v in fig.items()))
    assert fig["loss"] < R.TOL["out"], fig["loss"]
    for n in res["off"][1]:
        assert fig[n] < R.TOL["gqk" if _qk_group(n) else "gv"], (n, fig[n])


@pytest.mark.parametrize("ti_native", [0, 1])
def test_model_forward_matches_the_float64_restatement(ti_native):
    """both attention paths against tisas_ref.model_forward_f64.  Tolerance: the output of one whole block in fp32 — the same
    residual / layer-norm / feed-forward structure as K13's block, whose measured floor is 3.3e-7 and tolerance 3e-6
    (tests/sasblock_ref.py)"""
    model = _model(ti_native, 20, 32).eval()
    batch = _batch(12, 20, 50, 300, 3)
    with torch.no_grad():
        got = model.forward(batch).cpu().numpy()
    sd = {n: v.cpu().numpy() for n, v in model.state_dict().items()}
    users = batch["user_id"].cpu().numpy()
    ref = R.model_forward_f64(sd, batch["history_items"].cpu().numpy(), batch["lengths"].cpu().numpy(),
                              batch["history_times"].cpu().numpy(), sd["min_interval"][users], 4, 32)
    err = R.rel_err(got, ref)
    print("model forward ti_native %d against float64: %.2e" % (ti_native, err))
    assert got.shape == (12, 64) and err < 3e-6, err


def test_peak_memory_of_a_training_step():
    """B = 256, T = 48, D = 64: the native path must not build the two gathered [B, T, T, D] arrays"""
    B, T, D = 256, 48, 64
    batch = _batch(B, T, 50, 300, 4, full=True)
    peak = {}
    for flag in (1, 0):
        model = _model(flag, T, 512, dropout=0.1)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        model.train()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        opt.zero_grad()
        loss = model.predict(batch)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        peak[flag] = torch.cuda.max_memory_allocated(DEV) - base
        assert np.isfinite(float(loss))
        if flag:
            assert model._ti_native_ok == {T: True}
            hip_ops._WS.clear()       # the kernels' scratch is counted in the flag-on peak and freed before the flag-off run
        del model, opt, loss
    gathered = 2 * B * T * T * D * 4
    print("peak memory of one step: ti_native 1 %.1f MB, ti_native 0 %.1f MB, two gathered arrays %.1f MB"
          % (peak[1] / 1e6, peak[0] / 1e6, gathered / 1e6))
    assert peak[1] <= peak[0] - gathered, (peak, gathered)


# ------------------------------------------------------------------------------------------------ runner and launcher
def _argv(path, tmp, extra=()):
    return ["--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--dropout", "0.0", "--history_max", "20",
            "--time_max", "64", "--model_name", "TiSASRec", "--runner_name", "HipRunner", "--dataset", "ml-100k", "--path", path,
            "--epoch", "1", "--batch_size", "1024", "--eval_batch_size", "512", "--optimizer", "Adam", "--lr", "1e-3", "--l2", "0.0",
            "--log_file", str(tmp / "log.txt"), "--model_path", str(tmp / "m.pt"), "--num_workers", "0", "--topk", "5,10",
            "--metric", "NDCG, HR", "--random_seed", "3407"] + list(extra)


@pytest.fixture(scope="module")
def ml100k(tmp_path_factory):
    from test_reader import _write_inter
    from whisprrec_amd import main as launcher
    tmp = tmp_path_factory.mktemp("tisasrec")
    path = _write_inter(np.load(os.path.join(GOLD, "g8_reader.npz")), tmp)
    args, model_class, reader_class, runner_class = launcher.build_args(_argv(path, tmp, ["--ti_native", "1", "--seq_eval_native", "1"]))
    args.device = torch.device("cuda")
    corpus = reader_class(args).corpus()
    return {"args": args, "model_class": model_class, "runner_class": runner_class, "corpus": corpus, "tmp": tmp, "path": path}


class _FirstBatch(Exception):
    pass


def test_fit_batch_loop_sees_the_loader_batches_and_trains(ml100k, monkeypatch):
    from whisprrec_amd import main as launcher, runner
    args, model_class, corpus = ml100k["args"], ml100k["model_class"], ml100k["corpus"]
    launcher.init_seed(args.random_seed)
    model = model_class(args, corpus).to(args.device)
    ds = model_class.Dataset(model, corpus, "train")
    seen = {}

    def capture(batch):
        seen["batch"] = {k: v.detach().cpu().clone() for k, v in batch.items() if isinstance(v, torch.Tensor)}
        raise _FirstBatch()

    # the reference loop: per-sample feed dicts collated by the DataLoader; stopped at its first batch
    launcher.init_seed(7)
    monkeypatch.setattr(model, "predict", capture)
    with pytest.raises(_FirstBatch):
        runner.BaseRunner(args).fit(ds, epoch=1)
    loader = seen.pop("batch")
    monkeypatch.undo()
    # the batch loop: slices of device columns, the times travelling with the rows; one whole epoch
    launcher.init_seed(7)
    model.optimizer = None
    real = model.predict

    def spy(batch):
        if "batch" not in seen:
            seen["batch"] = {k: v.detach().cpu().clone() for k, v in batch.items() if isinstance(v, torch.Tensor)}
        return real(batch)

    monkeypatch.setattr(model, "predict", spy)
    run = ml100k["runner_class"](args)
    loss = run.fit(ds, epoch=1)
    assert np.isfinite(loss) and 0.0 < loss < 1.0
    assert all(model._ti_native_ok.values()) and model._ti_native_ok, "the attention kernels refused the test's shape"
    mine = seen["batch"]
    w = loader["history_items"].shape[1]
    for k in ("user_id", "pos_item", "lengths"):
        assert torch.equal(mine[k].reshape(-1), loader[k].reshape(-1)), k
    assert torch.equal(mine["neg_items"].reshape(-1), loader["neg_items"].reshape(-1))
    for k in ("history_items", "history_times"):
        assert torch.equal(mine[k][:, :w], loader[k]) and not mine[k][:, w:].any(), k


def test_device_evaluation_returns_the_host_ranks(ml100k, monkeypatch):
    from whisprrec_amd import main as launcher, runner
    args, model_class, corpus = ml100k["args"], ml100k["model_class"], ml100k["corpus"]
    launcher.init_seed(args.random_seed)
    model = model_class(args, corpus).to(args.device)
    with torch.no_grad():
        model.item_embedding.weight.mul_(30)                               # scores that spread: few near-ties
    ds = model_class.Dataset(model, corpus, "dev")
    ds.data = {k: np.asarray(v)[:200] for k, v in ds.data.items()}
    pred = runner.BaseRunner(args).interface(ds).astype(np.float64)
    host_rank = np.argwhere((-pred).argsort(axis=1) == 0)[:, 1] + 1
    target, S = pred[:, 0], pred[:, 1:].copy()
    S[np.arange(len(ds)), np.asarray(ds.data["item_id"])] = np.nan
    fin = np.isfinite(S)
    margin = np.where(fin, np.abs(S - target[:, None]), np.inf).min(axis=1)
    ok = margin > 1e-5 * np.abs(S[fin]).max()
    run = ml100k["runner_class"](args)
    monkeypatch.setattr(runner.BaseRunner, "interface", lambda *a: pytest.fail("the host path ran"))
    assert run._seq_eval_ok(ds)
    rank = run.rank_rows(ds)
    print("tisasrec device evaluation: rows kept %.3f, ranks differing on kept rows %d"
          % (ok.mean(), int((rank[ok] != host_rank[ok]).sum())))
    assert rank.shape == (200,) and ok.mean() >= 0.9
    assert np.array_equal(rank[ok], host_rank[ok])
    res = run.evaluate(ds, [5, 10], ["NDCG", "HR"])
    assert set(res) == {"NDCG@5", "HR@5", "NDCG@10", "HR@10"}
    # top-K through the same queries; recommend_next needs the times and the users
    items, _ = run.recommend_rows(ds, 5, rows=[0, 7])
    users, pos = np.asarray(ds.data["user_id"]), np.asarray(ds.data["position"])
    his = [corpus.user_his[users[r]][:pos[r]] for r in (0, 7)]
    nx, _ = run.recommend_next(model, corpus, [[x[0] for x in h] for h in his], 5, users=users[[0, 7]],
                               times=[[x[1] for x in h] for h in his])
    assert np.array_equal(items, nx)
    with pytest.raises(ValueError, match="times="):
        run.recommend_next(model, corpus, [[1, 2]], 5, users=[1])


def test_launcher_runs_one_epoch_end_to_end(ml100k, tmp_path):
    from whisprrec_amd import main as launcher
    argv = _argv(ml100k["path"], tmp_path, ["--ti_native", "1", "--seq_eval_native", "1", "--dropout", "0.1", "--save_rec", "5"])
    res = launcher.main(argv)
    assert "NDCG@5" in res and "HR@10" in res
    assert os.path.exists(os.path.join(ml100k["path"], "ml-100k", "rec-TiSASRec.csv"))
    assert os.path.exists(str(tmp_path / "m.pt"))
