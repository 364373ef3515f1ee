"""Row-lazy Adam / SGD for a table fed by (index, gradient row) pairs (whisprrec_amd/csrc/wr_rowopt.hip, hip_ops.RowLazyTable,
--emb_lazy of SASRec / ContraRec / IF4Rec) on the GPU.

Cases, reference and tolerances: tests/rowopt_ref.py and tests/test_emb_lazy_contract.py (TOL = 8 x the fp32 floor).
  1 bitwise: per step "zero table, scatter_add_rows, adam_dense / sgd_dense" against RowLazyTable.step, flushed at the end;
    the same positions handed as three lists;  2 the lazy gather before every step against gather_rows on the dense arm's table,
    and nothing but its output written;  3 float64 parity on the update;  4 the lag bound, and the same bits for max_lag 0 / 4 /
    None;  5 ids outside the table;  6 SASRec and ContraRec through HipRunner.fit, --emb_lazy 1 against 0;  7 no table-sized
    temporary;  8 the fall-backs;  9 the pair face (hip_ops.RowLazyEmaTable) with momentum 1 against the single table.

Model bound (6).  Floor: the --emb_lazy 0 run (fp32, GPU) against a float64 run of the model's stock torch path on the CPU —
nn.Embedding in place of HipEmbedding, torch.optim.Adam, the very batches the GPU run trained on — as max over the parameters of
max|got - ref| / max|ref - before| after the 10 steps, and max relative error of the 10 losses.  The key biases are measured
apart, against the largest update of any parameter: their gradient is zero in exact arithmetic (a softmax does not see a shift
of its row), so Adam turns rounding noise into steps of lr in fp32 and into nothing in float64 — no run can agree with another
on them beyond that.  The floors are measured again and printed by every run of the test (the bounds are the constants below);
recorded on an MI355X (other native flags off / on), bound = 8 x the model's larger floor, rounded up to one digit:
    SASRec     update 4.27e-5 / 3.64e-5 -> 4e-4   key biases 9.21e-3 / 5.83e-3 -> 8e-2   losses 8.91e-8 / 8.91e-8 -> 8e-7
    ContraRec  update 5.94e-4 / 4.13e-4 -> 5e-3   key biases 5.91e-2 / 3.74e-2 -> 5e-1   losses 6.86e-8 / 1.20e-7 -> 1e-6
  and --emb_lazy 1 against --emb_lazy 0 in the same runs: SASRec update 1.3e-5 / 1.1e-5, key biases 3.6e-3 / 3.8e-3, losses
  8.6e-8 / 8.4e-8; ContraRec update 1.2e-5 / 1.4e-5, key biases 2.6e-2 / 3.0e-2, losses 0 / 1.1e-7.
"""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowopt_ref as R  # noqa: E402
from test_emb_lazy_contract import TOL, case_runs, figures  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAGS = (0, 4, None)

# 8 x the measured floors of the module docstring
MODEL_TOLS = {"SASRec": {"update": 4e-4, "k_bias": 8e-2, "loss": 8e-7}, "ContraRec": {"update": 5e-3, "k_bias": 5e-1, "loss": 1e-6}}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _device_case(case):
    n_rows, D, pad, _ = case
    W0, steps = R.make_case(n_rows, D, pad)
    rng = np.random.RandomState(99)
    # the query of the gather test: duplicates, the padding row, the hot row, the rows with gaps, rows used once, rows never
    # used (first and last rows of the table) and random rows inside and outside any step; two-dimensional on purpose
    q = np.concatenate([[0, 0, R.HOT_ROW, R.HOT_ROW, 1, 2, n_rows - 1, n_rows - 1, n_rows - 3],
                        R.GAP_ROW0 + np.asarray(sorted(R.GAP_USES)), np.arange(R.ONCE_ROW0, R.ONCE_ROW0 + R.N_ONCE),
                        rng.randint(0, n_rows, 294)]).astype(np.int64).reshape(4, 80)
    return _t(W0), [(_t(i), _t(s)) for i, s in steps], _t(q)


def _dense_arm(opt, case, on_step=None):
    """arm A; on_step(t, W) sees the table before step t"""
    from whisprrec_amd import hip_ops
    _, _, pad, l2 = case
    W0, steps, _ = _device_case(case)
    W, m, v = W0.clone(), torch.zeros_like(W0), torch.zeros_like(W0)
    for t, (idx, src) in enumerate(steps, start=1):
        if on_step is not None:
            on_step(t, W)
        G = torch.zeros_like(W)
        hip_ops.scatter_add_rows(G, idx, src, padding_idx=pad)
        if opt == "Adam":
            hip_ops.adam_dense(W, m, v, G, t, R.LR[opt], l2)
        else:
            hip_ops.sgd_dense(W, G, R.LR[opt], l2)
    return W, m, v


def _lazy_arm(opt, case, max_lag, split=False, on_step=None):
    """arm B; on_step(t, table) before step t; -> the flushed table object"""
    from whisprrec_amd import hip_ops
    _, _, pad, l2 = case
    W0, steps, _ = _device_case(case)
    tab = hip_ops.RowLazyTable(W0.clone(), opt, R.LR[opt], l2, max_lag=max_lag, padding_idx=pad)
    for t, (idx, src) in enumerate(steps, start=1):
        if on_step is not None:
            on_step(t, tab)
        if split and idx.numel() >= 3:
            a, b = idx.numel() // 3, idx.numel() // 2
            tab.step([idx[:a], idx[a:b], idx[b:]], [src[:a], src[a:b], src[b:]])
        else:
            tab.step([idx], [src])
        assert tab.t == t
    return tab


def _state(tab):
    return [x.clone() for x in (tab.w, tab.m, tab.v, tab.last) if x is not None]


# ------------------------------------------------------------------------------------------------ 1, 2, 4: bits and lag
@pytest.mark.parametrize("opt", ["Adam", "SGD"])
@pytest.mark.parametrize("case", R.CASES)
def test_lazy_table_holds_the_bits_of_the_dense_kernels(opt, case):
    from whisprrec_amd import hip_ops
    n_rows, D, pad, l2 = case
    _, _, q = _device_case(case)
    dense_rows = {}
    Wd, md, vd = _dense_arm(opt, case, on_step=lambda t, W: dense_rows.__setitem__(t, hip_ops.gather_rows(W, q)))
    never = torch.arange(n_rows - R.N_NEVER, n_rows, device=DEV)
    for lag in LAGS:
        behind = []

        def before_step(t, tab):
            keep = _state(tab)
            got = tab.gather(q)
            assert got.shape == q.shape + (D,) and torch.equal(got, dense_rows[t]), (lag, t)       # 2: the gather
            assert all(torch.equal(a, b) for a, b in zip(keep, _state(tab))), (lag, t)             #    wrote nothing else
            if tab.stateful:
                behind.append(tab.behind())
                if lag == 0 and t > 1:
                    assert int(tab.last[never].max()) == 0                                        # 4: never used: not touched

        tab = _lazy_arm(opt, case, lag, on_step=before_step)
        if tab.stateful:
            behind.append(tab.behind())
            if lag == 4:
                assert max(behind) <= 5, behind                                                   # 4: the bound (before the flush)
            if lag == 0:
                assert behind[-1] == R.N_STEPS
        tab.flush()
        if tab.stateful:
            assert int(tab.last.min()) == tab.t == R.N_STEPS and tab.behind() == 0
        assert torch.equal(tab.w, Wd), (lag, float((tab.w - Wd).abs().max()))                     # 1: bitwise
        if opt == "Adam":
            assert torch.equal(tab.m, md) and torch.equal(tab.v, vd), lag
        keep = _state(tab)
        tab.flush()                                                                               # a no-op when flushed
        assert all(torch.equal(a, b) for a, b in zip(keep, _state(tab)))
    tab = _lazy_arm(opt, case, None, split=True)                                                  # 1: three lists = one list
    tab.flush()
    assert torch.equal(tab.w, Wd)
    if opt == "Adam":
        assert torch.equal(tab.m, md) and torch.equal(tab.v, vd)


# ------------------------------------------------------------------------------------------------ 3: float64 parity
@pytest.mark.parametrize("opt", ["Adam", "SGD"])
@pytest.mark.parametrize("case", R.CASES)
def test_lazy_table_matches_the_float64_loop_on_the_update(opt, case):
    W0, _, ref, _, _ = case_runs(opt, case)
    tab = _lazy_arm(opt, case, None)
    tab.flush()
    state = {"m": tab.m.cpu().numpy(), "v": tab.v.cpu().numpy()} if opt == "Adam" else {}
    fig = figures(W0, ref, (tab.w.cpu().numpy(), state))
    tol = TOL[opt]
    print("parity emb_lazy %s %s: update/table %.1e | update_err %.2e (tol %.0e) row_update_err %.2e (tol %.0e) state_err %.2e "
          "(tol %.0e)" % (opt, case, fig["update_over_table"], fig["update"], tol["update"], fig["row"], tol["row"],
                          fig.get("state", 0.0), tol.get("state", 0.0)), flush=True)
    assert fig["update"] < tol["update"] and fig["row"] < tol["row"], fig
    if opt == "Adam":
        assert fig["state"] < tol["state"], fig


# ------------------------------------------------------------------------------------------------ 5: ids outside the table
@pytest.mark.parametrize("opt,l2", [("Adam", 0.0), ("SGD", 1e-3), ("SGD", 0.0)])
def test_ids_outside_the_table_raise_and_leave_it_unchanged(opt, l2):
    from whisprrec_amd import hip_ops
    case = R.CASES[0]
    n_rows, D = case[0], case[1]
    W0, steps, _ = _device_case(case)
    tab = hip_ops.RowLazyTable(W0.clone(), opt, R.LR[opt], l2, max_lag=4, padding_idx=0)
    for idx, src in steps[:2]:
        tab.step([idx], [src])
    keep, t = _state(tab), tab.t
    for bad in (n_rows, -1, 1 << 40):
        idx = torch.tensor([3, bad, 7, 7], device=DEV)
        with pytest.raises(IndexError):
            tab.gather(idx)
        with pytest.raises(IndexError):
            tab.step([steps[1][0], idx], [steps[1][1], torch.ones(4, D, device=DEV)])
        assert tab.t == t and all(torch.equal(a, b) for a, b in zip(keep, _state(tab))), bad
    tab.check()                                            # the findings were raised and cleared
    assert tab.gather(torch.tensor([3, 7], device=DEV)).shape == (2, D)
    if tab.stateful:
        # unchecked (a model's training loop): the id is skipped by the kernels, the finding waits for the flush
        rows = tab.gather(torch.tensor([[3, n_rows]], device=DEV), check=False)
        assert not rows[0, 1].any() and rows[0, 0].any()
        tab.step([torch.tensor([3, n_rows, -5], device=DEV)], [torch.ones(3, D, device=DEV)], check=False)
        assert tab.t == t + 1 and int(tab.last[3]) == t + 1
        with pytest.raises(IndexError):
            tab.flush()
        tab.flush()
        assert tab.behind() == 0


# ------------------------------------------------------------------------------------------------ 6: the models
def _corpus(n_items=500, n_users=41, per_user=9):
    """40 users with 9 items each in time order: 320 training rows (positions 1 .. 8), i.e. 10 batches of 32, histories 1 .. 8"""
    from whisprrec_amd import host
    rng = np.random.RandomState(5)
    his, frame, clicked = {}, {"user_id": [], "item_id": [], "position": []}, {}
    for u in range(1, n_users):
        items = (rng.permutation(n_items - 1)[:per_user] + 1).tolist()
        his[u] = [(it, t) for t, it in enumerate(items)]
        clicked[u] = set(items)
        for q, it in enumerate(items):
            frame["user_id"].append(u); frame["item_id"].append(it); frame["position"].append(q)
    train = {k: np.asarray(v, np.int64) for k, v in frame.items()}
    empty = {k: np.zeros(0, np.int64) for k in frame}
    corpus = host.Corpus(n_users, n_items, {"train": train, "dev": empty, "test": empty}, clicked, {u: set() for u in clicked})
    corpus.user_his = his
    return corpus


NATIVE = {"SASRec": ["--block_native", "1"], "ContraRec": ["--block_native", "1", "--ccc_native", "1", "--aug_native", "1"],
          "IF4Rec": ["--block_native", "1"]}
SHAPE = {"SASRec": ["--num_heads", "2", "--num_layers", "1", "--dropout", "0"], "ContraRec": [],
         "IF4Rec": ["--n_head", "2", "--encoder_dropout", "0"]}


def _setup(model_name, extra, corpus=None, device=DEV):
    from whisprrec_amd import main as launcher
    argv = ["--model_name", model_name, "--runner_name", "HipRunner", "--batch_size", "32", "--lr", "1e-3", "--l2", "0.0",
            "--emb_size", "64", "--history_max", "8", "--num_workers", "0", "--random_seed", "2024",
            "--model_path", "/tmp/wr_emb_lazy_gpu.pt", "--log_file", "/tmp/wr_emb_lazy_gpu.txt"] + SHAPE[model_name] + extra
    args, model_class, _, runner_class = launcher.build_args(argv)
    launcher.init_seed(args.random_seed)
    args.device = device
    corpus = corpus if corpus is not None else _corpus()
    model = model_class(args, corpus).to(device)
    return args, model, model_class.Dataset(model, corpus, "train"), runner_class(args)


def _emb(model):
    from whisprrec_amd.sasrec import HipEmbedding
    (name, mod), = [(n, m) for n, m in model.named_children() if isinstance(m, HipEmbedding)]
    return name, mod


def _fit(model_name, extra, epochs=1):
    """-> (model, runner, data, state before, batches, losses): one or more epochs through HipRunner.fit with predict spied on"""
    args, model, data, run = _setup(model_name, extra)
    before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    batches, losses = [], []
    predict = model.predict

    def spy(batch):
        batches.append({k: v.detach().cpu().clone() for k, v in batch.items() if isinstance(v, torch.Tensor)})
        loss = predict(batch)
        losses.append(loss.detach())
        return loss

    model.predict = spy
    for e in range(1, epochs + 1):
        run.fit(data, epoch=e)
    return model, run, data, before, batches, [float(x) for x in losses]


def _float64_run(model_name, before, batches):
    """the model's stock torch path in float64 on the CPU: nn.Embedding in place of HipEmbedding, torch.optim.Adam"""
    _, ref, _, _ = _setup(model_name, [], device=torch.device("cpu"))
    name, emb = _emb(ref)
    setattr(ref, name, nn.Embedding(emb.num_embeddings, emb.embedding_dim, padding_idx=emb.padding_idx if emb.padding_idx >= 0 else None))
    ref.load_state_dict(before)
    ref.double().train()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3, weight_decay=0.0)
    losses = []
    for b in batches:
        opt.zero_grad()
        loss = ref.predict(b)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return {k: v.detach() for k, v in ref.state_dict().items()}, losses


def _is_k_bias(name):
    return name.endswith("k_linear.bias")


def _update_err(got, other, ref, before):
    """-> (max over the parameters of max|got - other| / max|ref - before| of that parameter, the same for the key biases against
    the largest update of ANY parameter).  The gradient of a key bias is zero in exact arithmetic (a softmax does not see a shift
    of its row), so what Adam makes of it is the sign of rounding noise: lr per step in fp32, nothing in float64."""
    upd = {k: float((ref[k].double() - before[k].double()).abs().max()) for k in ref}
    diff = {k: float((got[k].double().cpu() - other[k].double().cpu()).abs().max()) for k in ref}
    rest = max(diff[k] / upd[k] for k in ref if not _is_k_bias(k) and upd[k] > 0)
    kb = max([diff[k] / max(upd.values()) for k in ref if _is_k_bias(k)] or [0.0])
    return rest, kb


@pytest.mark.parametrize("native", [0, 1])
@pytest.mark.parametrize("model_name", ["SASRec", "ContraRec"])
def test_models_train_the_same_with_the_lazy_table(model_name, native):
    from whisprrec_amd.sasrec import RowLazyOptimizer
    extra = NATIVE[model_name] if native else []
    MODEL_TOL = MODEL_TOLS[model_name]
    dense, _, _, before, batches, losses_d = _fit(model_name, extra + ["--emb_lazy", "0"])
    lazy, run, data, before_l, batches_l, losses_l = _fit(model_name, extra + ["--emb_lazy", "1"])
    assert len(batches) == len(batches_l) == 10 and len(data) == 320
    assert all(torch.equal(before[k], before_l[k]) for k in before)
    assert all(set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a) for a, b in zip(batches, batches_l))
    assert isinstance(lazy.optimizer, RowLazyOptimizer) and lazy.emb_lazy and not isinstance(dense.optimizer, RowLazyOptimizer)
    _, emb = _emb(lazy)
    table = lazy.optimizer.table()
    assert emb.weight.grad is None and table.t == 10
    assert _emb(dense)[1].weight.grad is not None
    ref, losses_r = _float64_run(model_name, before, batches)
    sd_d = dense.state_dict()
    sd_l = lazy.state_dict()                                  # flushes
    assert table.behind() == 0
    floor_u, floor_k = _update_err(sd_d, ref, ref, before)
    floor_l = max(abs(a - b) / abs(b) for a, b in zip(losses_d, losses_r))
    err_u, err_k = _update_err(sd_l, sd_d, ref, before)
    err_l = max(abs(a - b) / abs(b) for a, b in zip(losses_l, losses_d))
    print("parity emb_lazy model %s native %d: floor update %.2e key biases %.2e loss %.2e | lazy against dense update %.2e (tol "
          "%.0e) key biases %.2e (tol %.0e) loss %.2e (tol %.0e)" % (model_name, native, floor_u, floor_k, floor_l, err_u,
                                                                    MODEL_TOL["update"], err_k, MODEL_TOL["k_bias"], err_l,
                                                                    MODEL_TOL["loss"]), flush=True)
    assert err_u < MODEL_TOL["update"] and err_k < MODEL_TOL["k_bias"] and err_l < MODEL_TOL["loss"]
    # eval in the middle of training flushes; the checkpoint round-trips; a second epoch continues the same optimizer state
    lazy.train()
    lazy.optimizer.zero_grad()
    fd = {k: v.to(DEV) for k, v in batches[0].items()}
    lazy.predict(fd).backward()
    lazy.optimizer.step()
    assert table.t == 11 and (table.behind() > 0 or not table.stateful)
    lazy.eval()
    assert table.behind() == 0
    sd = {k: v.clone() for k, v in lazy.state_dict().items()}
    lazy.load_state_dict(sd)
    assert all(torch.equal(v, lazy.state_dict()[k]) for k, v in sd.items())
    m_before = table.m.clone()
    run.fit(data, epoch=2)
    assert lazy.optimizer.table() is table and table.t == 21 and emb.weight.grad is None
    assert float(m_before.abs().sum()) > 0 and not torch.equal(table.m, m_before)
    assert lazy.optimizer.inner.state[next(p for p in lazy.parameters() if p is not emb.weight)]["step"] == 21


# ------------------------------------------------------------------------------------------------ 7: no table-sized temporary
def _step_peak(flag):
    n_items, B, T = 200_000, 32, 8
    args, model, _, _ = _setup("SASRec", ["--emb_lazy", str(flag)], corpus=_corpus(n_items=n_items))
    if model.optimizer is None:
        model.optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    rng = np.random.RandomState(3)
    model.train()

    def step():
        lens = rng.randint(1, T + 1, B)
        hist = rng.randint(1, n_items, (B, T)) * (np.arange(T)[None, :] < lens[:, None])
        fd = {"history_items": _t(hist), "lengths": _t(lens), "pos_item": _t(rng.randint(1, n_items, B)),
              "neg_items": _t(rng.randint(1, n_items, (B, 1)))}
        model.optimizer.zero_grad()
        model.predict(fd).backward()
        model.optimizer.step()

    step(); step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(); step(); step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / float(n_items * 64 * 4)


def test_no_table_sized_temporary():
    lazy, dense = _step_peak(1), _step_peak(0)
    print("emb_lazy peak above the baseline, in table sizes (200,000 x 64): lazy %.3f dense %.3f" % (lazy, dense), flush=True)
    assert lazy < 0.5 and dense > 1.0


# ------------------------------------------------------------------------------------------------ 8: fall-backs
@pytest.mark.parametrize("model_name,extra,word", [("SASRec", ["--optimizer", "Adagrad"], "Adagrad"),
                                                    ("IF4Rec", ["--interest_native", "1"], "interest_native")])
def test_fallbacks_train_on_the_dense_path_and_log_once(model_name, extra, word, caplog):
    with caplog.at_level(logging.WARNING):
        args, model, data, run = _setup(model_name, extra + ["--emb_lazy", "1"])
        assert model.emb_lazy is False and model.optimizer is None
        before = _emb(model)[1].weight.detach().clone()
        loss = run.fit(data, epoch=1)
    assert sum("--emb_lazy 1" in r.getMessage() and word in r.getMessage() for r in caplog.records) == 1
    assert np.isfinite(loss) and isinstance(model.optimizer, torch.optim.Optimizer)
    assert _emb(model)[1]._lazy is None and not torch.equal(_emb(model)[1].weight.detach(), before)


# ------------------------------------------------------------------------------------------------ 9: one family, two faces
@pytest.mark.parametrize("max_lag", [0, 4])
@pytest.mark.parametrize("opt", ["Adam", "SGD"])
@pytest.mark.parametrize("case", [(1000, 20, -1, 1e-3), (1000, 64, -1, 0.0)])
def test_pair_with_momentum_one_is_the_single_table(case, opt, max_lag):
    """RowLazyEmaTable with momentum 1 leaves its target alone (ema_elem(t, w, 1, 0) = t for finite w and t != 0), so its online
    table must go through the bits of RowLazyTable: the same gathers before every step, the same table and moments at the end"""
    from whisprrec_amd import hip_ops
    assert case in R.CASES
    n_rows, D, pad, l2 = case
    W0, steps, q = _device_case(case)
    T0 = np.random.RandomState(7).standard_normal((n_rows, D)).astype(np.float32)
    T0[T0 == 0] = 1.0
    T0 = _t(T0)
    one = hip_ops.RowLazyTable(W0.clone(), opt, R.LR[opt], l2, max_lag=max_lag)
    pair = hip_ops.RowLazyEmaTable(W0.clone(), T0.clone(), opt, R.LR[opt], l2, 1.0, max_lag=max_lag)
    for t, (idx, src) in enumerate(steps, start=1):
        assert torch.equal(one.gather(q), pair.gather(q)[0]), t
        one.step([idx], [src])
        pair.step([idx], [src])
    one.flush()
    pair.flush()
    assert one.t == pair.t == R.N_STEPS and torch.equal(one.w, pair.w)
    if opt == "Adam":
        assert torch.equal(one.m, pair.m) and torch.equal(one.v, pair.v)
    assert torch.equal(pair.tgt, T0)
