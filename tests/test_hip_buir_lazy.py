"""BUIR's row-lazy (online, target) pairs (whisprrec_amd/csrc/wr_rowopt.hip K24, hip_ops.RowLazyEmaTable, --emb_lazy 1 on BUIR) on
the GPU.

Cases, reference and tolerances: tests/buir_lazy_ref.py and tests/test_buir_lazy_contract.py (TOL = 8 x the fp32 floor).
  1 bitwise: per step "zero table, scatter_add_rows, adam_dense / sgd_dense, ema_update_" against RowLazyEmaTable.step, flushed at
    the end, for max_lag 0 / 4 / None; the same positions handed as three lists; a second flush;  2 the gather before every step
    against gather_rows on the dense arm's W and T, nothing else written, the lag bound;  3 float64 parity on the update of both
    tables and the state;  4 ids outside the table;  5 the loss kernel on the gathered rows against the full tables;  6 BUIR
    through HipRunner.fit, --emb_lazy 1 against 0;  7 no table-sized temporary;  8 the fall-backs.

Model bound (6).  Floor: the --emb_lazy 0 run (fp32, GPU, --buir_native 1) against a float64 run of the stock torch model on the
CPU on the very batches the GPU run trained on — max over the parameters (the target tables included) of max|got - ref| /
max|ref - before| after the 10 steps, and the max relative error of the 10 losses.  The floors are measured again and printed by
every run (the bounds are the constants below); recorded on an MI355X, bound = 8 x the floor, rounded up to one digit:
    Adam (lr 1e-3, l2 1e-4)  update 7.11e-4 -> 6e-3   losses 9.71e-8 -> 8e-7
    SGD  (lr 0.1,  l2 1e-4)  update 4.85e-3 -> 4e-2   losses 8.36e-8 -> 7e-7
  and --emb_lazy 1 against --emb_lazy 0 in the same runs: Adam update 5.5e-5, losses 6.1e-8; SGD update 2.2e-5, losses 0.
"""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buir_lazy_ref as B  # noqa: E402
from test_buir_lazy_contract import TOL, case_runs, figures, tol  # noqa: E402

R = B.R
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LAGS = (0, 4, None)

# 8 x the measured floors of the module docstring
MODEL_TOLS = {"Adam": {"update": 6e-3, "loss": 8e-7}, "SGD": {"update": 4e-2, "loss": 7e-7}}
MODEL_LR = {"Adam": "1e-3", "SGD": "0.1"}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _device_case(case, seed=0):
    n_rows, D, _, _ = case
    W0, steps = B.make_case(n_rows, D, seed)
    rng = np.random.RandomState(99)
    # the query of the gather test: duplicates, the hot row, the rows with gaps, rows used once, rows never used (first and last
    # rows of the table) and random rows inside and outside any step; two-dimensional on purpose
    q = np.concatenate([[0, 0, R.HOT_ROW, R.HOT_ROW, 1, 2, n_rows - 1, n_rows - 1, n_rows - 3],
                        R.GAP_ROW0 + np.asarray(sorted(R.GAP_USES)), np.arange(R.ONCE_ROW0, R.ONCE_ROW0 + R.N_ONCE),
                        rng.randint(0, n_rows, 294)]).astype(np.int64).reshape(4, 80)
    return _t(W0), [(_t(i), _t(s)) for i, s in steps], _t(q)


def _dense_arm(opt, case, on_step=None, seed=0, n_steps=None):
    """arm A; on_step(t, W, T) sees the tables before step t; -> (W, T, m, v)"""
    from whisprrec_amd import hip_ops
    _, _, l2, mom = case
    W0, steps, _ = _device_case(case, seed)
    W, T, m, v = W0.clone(), W0.clone(), torch.zeros_like(W0), torch.zeros_like(W0)
    for t, (idx, src) in enumerate(steps[:n_steps], start=1):
        if on_step is not None:
            on_step(t, W, T)
        G = torch.zeros_like(W)
        hip_ops.scatter_add_rows(G, idx, src)
        if opt == "Adam":
            hip_ops.adam_dense(W, m, v, G, t, B.LR[opt], l2)
        else:
            hip_ops.sgd_dense(W, G, B.LR[opt], l2)
        hip_ops.ema_update_(T, W, mom)
    return W, T, m, v


def _new_table(opt, case, max_lag, seed=0):
    from whisprrec_amd import hip_ops
    _, _, l2, mom = case
    W0, _, _ = _device_case(case, seed)
    return hip_ops.RowLazyEmaTable(W0.clone(), W0.clone(), opt, B.LR[opt], l2, mom, max_lag=max_lag)


def _lazy_arm(opt, case, max_lag, split=False, on_step=None, seed=0, n_steps=None):
    """arm B; on_step(t, table) before step t; -> the table object, not flushed"""
    _, steps, _ = _device_case(case, seed)
    tab = _new_table(opt, case, max_lag, seed)
    for t, (idx, src) in enumerate(steps[:n_steps], start=1):
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
    return [x.clone() for x in (tab.w, tab.tgt, tab.m, tab.v, tab.last) if x is not None]


# ------------------------------------------------------------------------------------------------ 1, 2: bits, gather, lag
@pytest.mark.parametrize("opt", ["Adam", "SGD"])
@pytest.mark.parametrize("case", B.CASES)
def test_lazy_pair_holds_the_bits_of_the_dense_kernels(opt, case):
    from whisprrec_amd import hip_ops
    n_rows, D, l2, mom = case
    _, _, q = _device_case(case)
    dense_rows = {}
    Wd, Td, md, vd = _dense_arm(opt, case, on_step=lambda t, W, T: dense_rows.__setitem__(
        t, (hip_ops.gather_rows(W, q), hip_ops.gather_rows(T, q))))
    never = torch.arange(n_rows - R.N_NEVER, n_rows, device=DEV)

    def same_as_dense(tab, what):
        assert torch.equal(tab.w, Wd), (what, float((tab.w - Wd).abs().max()))
        assert torch.equal(tab.tgt, Td), (what, float((tab.tgt - Td).abs().max()))
        if opt == "Adam":
            assert torch.equal(tab.m, md) and torch.equal(tab.v, vd), what

    for lag in LAGS:
        behind = []

        def before_step(t, tab):
            keep = _state(tab)
            got_w, got_t = tab.gather(q)
            assert got_w.shape == got_t.shape == q.shape + (D,)
            assert torch.equal(got_w, dense_rows[t][0]) and torch.equal(got_t, dense_rows[t][1]), (lag, t)   # 2: the gather
            assert all(torch.equal(a, b) for a, b in zip(keep, _state(tab))), (lag, t)                       #    wrote nothing else
            behind.append(tab.behind())
            if lag == 0 and t > 1:
                assert int(tab.last[never].max()) == 0                                                      # never used: not touched

        tab = _lazy_arm(opt, case, lag, on_step=before_step)
        behind.append(tab.behind())
        if lag == 4:
            assert max(behind) <= 5, behind                                                                 # the bound (before the flush)
        if lag == 0:
            assert behind[-1] == R.N_STEPS
        tab.flush()
        assert int(tab.last.min()) == int(tab.last.max()) == tab.t == R.N_STEPS and tab.behind() == 0
        same_as_dense(tab, lag)                                                                             # 1: bitwise
        keep = _state(tab)
        tab.flush()                                                                                         # a no-op when flushed
        assert all(torch.equal(a, b) for a, b in zip(keep, _state(tab)))
    tab = _lazy_arm(opt, case, None, split=True)                                                            # 1: three lists = one list
    tab.flush()
    same_as_dense(tab, "split")


# ------------------------------------------------------------------------------------------------ 3: float64 parity
@pytest.mark.parametrize("opt", ["Adam", "SGD"])
@pytest.mark.parametrize("case", B.CASES)
def test_lazy_pair_matches_the_float64_loop_on_the_update(opt, case):
    W0, _, ref, _, _ = case_runs(opt, case)
    mom = case[3]
    tab = _lazy_arm(opt, case, None)
    tab.flush()
    state = {"m": tab.m.cpu().numpy(), "v": tab.v.cpu().numpy()} if opt == "Adam" else {}
    fig = figures(W0, ref, (tab.w.cpu().numpy(), tab.tgt.cpu().numpy(), state))
    names = ["update", "row", "t_update", "t_row"] + (["state"] if opt == "Adam" else [])
    print("parity buir_lazy %s %s: update/table %.1e (target %.1e) | %s" % (
        opt, case, fig["update_over_table"], fig["t_update_over_table"],
        " ".join("%s_err %.2e (tol %.0e)" % (n, fig[n], tol(opt, n, mom)) for n in names)), flush=True)
    for n in names:
        assert fig[n] < tol(opt, n, mom), (n, fig)


# ------------------------------------------------------------------------------------------------ 4: ids outside the table
@pytest.mark.parametrize("opt,l2", [("Adam", 0.0), ("SGD", 1e-3), ("SGD", 0.0)])
def test_ids_outside_the_table_raise_and_leave_it_unchanged(opt, l2):
    from whisprrec_amd import hip_ops
    case = B.CASES[0]
    n_rows, D = case[0], case[1]
    W0, steps, _ = _device_case(case)
    tab = hip_ops.RowLazyEmaTable(W0.clone(), W0.clone(), opt, B.LR[opt], l2, 0.9, max_lag=4)
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
    assert tab.gather(torch.tensor([3, 7], device=DEV))[1].shape == (2, D)
    # unchecked (a model's training loop): the id is skipped by the kernels, the finding waits for the flush
    rows_w, rows_t = tab.gather(torch.tensor([[3, n_rows]], device=DEV), check=False)
    assert not rows_w[0, 1].any() and not rows_t[0, 1].any() and rows_w[0, 0].any() and rows_t[0, 0].any()
    tab.step([torch.tensor([3, n_rows, -5], device=DEV)], [torch.ones(3, D, device=DEV)], check=False)
    assert tab.t == t + 1 and int(tab.last[3]) == t + 1
    with pytest.raises(IndexError):
        tab.flush()
    tab.flush()
    assert tab.behind() == 0
    tab.step([], [])                                       # a step without positions still counts
    assert tab.t == t + 2 and tab.behind() == 1


# ------------------------------------------------------------------------------------------------ 5: the loss kernel on gathered rows
@pytest.mark.parametrize("opt", ["Adam", "SGD"])
def test_loss_kernel_on_the_gathered_rows_has_the_bits_of_the_full_tables(opt):
    from whisprrec_amd import hip_ops
    case = B.CASES[0]
    assert case[:2] == (1000, 64)
    D = case[1]
    users, items = _device_case(case, 0)[1][1][0], _device_case(case, 1)[1][1][0]          # the ids of step 2: B = 333
    assert users.numel() == items.numel() == 333
    rng = np.random.RandomState(11)
    W, b = _t((rng.standard_normal((D, D)) * 0.17).astype(np.float32)), _t(rng.standard_normal(D).astype(np.float32))
    Ud, UTd, _, _ = _dense_arm(opt, case, seed=0, n_steps=1)
    Id, ITd, _, _ = _dense_arm(opt, case, seed=1, n_steps=1)
    ut, it = _lazy_arm(opt, case, 0, seed=0, n_steps=1), _lazy_arm(opt, case, 0, seed=1, n_steps=1)
    assert ut.behind() == 1 and it.behind() == 1
    uo, utg = ut.gather(users)
    io, itg = it.gather(items)
    pos = torch.arange(333, device=DEV)
    got = hip_ops.buir_loss_grad(uo, io, utg, itg, W, b, pos, pos)
    want = hip_ops.buir_loss_grad(Ud, Id, UTd, ITd, W, b, users, items)
    for name, g, w in zip(("loss", "gU", "gI", "gW", "gb"), got, want):
        assert torch.equal(g, w), name
    assert float(got[0]) > 0 and float(got[1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 6: the model
def _corpus(n_items=500, n_users=41, per_user=8):
    """40 users with 8 training items each: 320 training rows, i.e. 10 batches of 32; one held-out item per user in dev / test"""
    from whisprrec_amd import host
    rng = np.random.RandomState(5)
    frame, held, clicked, residual = {"user_id": [], "item_id": []}, {"user_id": [], "item_id": []}, {}, {}
    for u in range(1, n_users):
        items = (rng.permutation(n_items - 1)[:per_user + 1] + 1).tolist()
        clicked[u], residual[u] = set(items[:per_user]), {items[per_user]}
        for it in items[:per_user]:
            frame["user_id"].append(u); frame["item_id"].append(it)
        held["user_id"].append(u); held["item_id"].append(items[per_user])
    train = {k: np.asarray(v, np.int64) for k, v in frame.items()}
    dev = {k: np.asarray(v, np.int64) for k, v in held.items()}
    return host.Corpus(n_users, n_items, {"train": train, "dev": dev, "test": dev}, clicked, residual)


def _setup(opt, extra, corpus=None, device=DEV, emb="64"):
    from whisprrec_amd import main as launcher
    argv = ["--model_name", "BUIR", "--runner_name", "HipRunner", "--batch_size", "32", "--optimizer", opt, "--lr", MODEL_LR.get(opt, "1e-3"),
            "--l2", "1e-4", "--embedding_size", emb, "--num_workers", "0", "--random_seed", "2024", "--topk", "5,10",
            "--metric", "NDCG,HR", "--model_path", "/tmp/wr_buir_lazy_gpu.pt", "--log_file", "/tmp/wr_buir_lazy_gpu.txt"] + extra
    args, model_class, _, runner_class = launcher.build_args(argv)
    launcher.init_seed(args.random_seed)
    args.device = device
    corpus = corpus if corpus is not None else _corpus()
    model = model_class(args, corpus).to(device)
    return args, model, corpus, model_class.Dataset(model, corpus, "train"), runner_class(args)


def _fit(opt, extra):
    """-> (model, runner, corpus, data, state before, batches, losses): one epoch through HipRunner.fit with predict spied on"""
    args, model, corpus, data, run = _setup(opt, extra)
    before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    batches, losses = [], []
    predict = model.predict

    def spy(batch):
        batches.append({k: v.detach().cpu().clone() for k, v in batch.items() if isinstance(v, torch.Tensor)})
        loss = predict(batch)
        losses.append(loss.detach())
        return loss

    model.predict = spy
    run.fit(data, epoch=1)
    model.predict = predict
    return model, run, corpus, data, before, batches, [float(x) for x in losses]


def _float64_run(opt, before, batches):
    """the stock torch model in float64 on the CPU: torch.optim over every parameter, the target update in the step hook"""
    _, ref, _, _, _ = _setup(opt, ["--buir_native", "0"], device=torch.device("cpu"))
    ref.load_state_dict(before)
    ref.double().train()
    ref.optimizer = getattr(torch.optim, opt)(ref.parameters(), lr=float(MODEL_LR[opt]), weight_decay=1e-4)
    losses = []
    for b in batches:
        ref.optimizer.zero_grad()
        loss = ref.predict(b)
        loss.backward()
        ref.optimizer.step()
        losses.append(float(loss.detach()))
    return {k: v.detach() for k, v in ref.state_dict().items()}, losses


def _update_err(got, other, ref, before):
    """max over the parameters of max|got - other| / max|ref - before| of that parameter"""
    upd = {k: float((ref[k].double() - before[k].double()).abs().max()) for k in ref}
    assert all(u > 0 for u in upd.values()), upd
    return max(float((got[k].double().cpu() - other[k].double().cpu()).abs().max()) / upd[k] for k in ref)


@pytest.mark.parametrize("opt", ["Adam", "SGD"])
def test_model_trains_the_same_with_the_lazy_tables(opt):
    from whisprrec_amd.buir import BuirLazyOptimizer
    MODEL_TOL = MODEL_TOLS[opt]
    dense, _, _, _, before, batches, losses_d = _fit(opt, ["--buir_native", "1", "--emb_lazy", "0"])
    lazy, run, corpus, data, before_l, batches_l, losses_l = _fit(opt, ["--buir_native", "1", "--emb_lazy", "1"])
    assert len(batches) == len(batches_l) == 10 and len(data) == 320
    assert all(torch.equal(before[k], before_l[k]) for k in before) and len(before) == 6
    assert all(set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a) for a, b in zip(batches, batches_l))
    assert isinstance(lazy.optimizer, BuirLazyOptimizer) and lazy.emb_lazy and isinstance(dense.optimizer, torch.optim.Optimizer)
    tables = lazy.optimizer.tables()
    assert all(t.t == 10 for t in tables) and "_optimizer_hook" not in lazy.__dict__
    for emb in (lazy.user_online, lazy.user_target, lazy.item_online, lazy.item_target):
        assert emb.weight.grad is None
    assert dense.user_online.weight.grad is not None and lazy.predictor.weight.grad is not None
    ref, losses_r = _float64_run(opt, before, batches)
    sd_d = dense.state_dict()
    assert any(t.behind() > 0 for t in tables)
    sd_l = lazy.state_dict()                                  # flushes
    assert all(t.behind() == 0 for t in tables)
    floor_u = _update_err(sd_d, ref, ref, before)
    floor_l = max(abs(a - b) / abs(b) for a, b in zip(losses_d, losses_r))
    err_u = _update_err(sd_l, sd_d, ref, before)
    err_l = max(abs(a - b) / abs(b) for a, b in zip(losses_l, losses_d))
    print("parity buir_lazy model %s: floor update %.2e loss %.2e | lazy against dense update %.2e (tol %.0e) loss %.2e (tol %.0e)"
          % (opt, floor_u, floor_l, err_u, MODEL_TOL["update"], err_l, MODEL_TOL["loss"]), flush=True)
    assert err_u < MODEL_TOL["update"] and err_l < MODEL_TOL["loss"]
    # a state_dict in the middle of training holds flushed tables; the checkpoint round-trips; evaluation agrees with a model
    # loaded from it
    lazy.train()
    lazy.optimizer.zero_grad()
    lazy.predict({k: v.to(DEV) for k, v in batches[0].items()}).backward()
    lazy.optimizer.step()
    assert all(t.t == 11 for t in tables) and any(t.behind() > 0 for t in tables)
    sd = {k: v.detach().clone() for k, v in lazy.state_dict().items()}
    assert all(t.behind() == 0 for t in tables)
    dev_data = type(data)(lazy, corpus, "dev")
    got = run.evaluate(dev_data, [5, 10], ["NDCG", "HR"])
    assert all(t.behind() == 0 for t in tables)
    _, fresh, _, _, run2 = _setup(opt, ["--buir_native", "1", "--emb_lazy", "0"], corpus=corpus)
    fresh.load_state_dict(sd)
    assert all(torch.equal(v, fresh.state_dict()[k]) for k, v in sd.items())
    want = run2.evaluate(type(data)(fresh, corpus, "dev"), [5, 10], ["NDCG", "HR"])
    assert got == want and len(got) == 4, (got, want)
    lazy.load_state_dict(sd)
    assert all(torch.equal(v, lazy.state_dict()[k]) for k, v in sd.items())
    # an id outside a table, unchecked in the training loop, is raised by the flush of model.eval()
    lazy.train()
    lazy.optimizer.zero_grad()
    fd = {k: v.to(DEV).clone() for k, v in batches[0].items()}
    fd["user_id"][3] = lazy.user_num
    lazy.predict(fd).backward()
    lazy.optimizer.step()
    with pytest.raises(IndexError):
        lazy.eval()
    lazy.eval()


# ------------------------------------------------------------------------------------------------ 7: no table-sized temporary
def _step_peak(flag):
    n, Bsz = 200_000, 2048
    from whisprrec_amd import host
    none = np.zeros(0, np.int64)
    corpus = host.Corpus(n, n, {"train": {"user_id": none, "item_id": none}}, {}, {})
    _, model, _, _, _ = _setup("Adam", ["--buir_native", "1", "--emb_lazy", str(flag)], corpus=corpus)
    if model.optimizer is None:
        model.optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    rng = np.random.RandomState(3)
    model.train()

    def step():
        fd = {"user_id": _t(rng.randint(0, n, Bsz)), "pos_item": _t(rng.randint(0, n, Bsz))}
        model.optimizer.zero_grad()
        model.predict(fd).backward()
        model.optimizer.step()

    step(); step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step(); step(); step()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / float(n * 64 * 4)
    grads = [e.weight.grad for e in (model.user_online, model.user_target, model.item_online, model.item_target)]
    return peak, grads


def test_no_table_sized_temporary():
    (lazy, grads), (dense, _) = _step_peak(1), _step_peak(0)
    print("buir_lazy peak above the resting level, in table sizes (200,000 x 64 = 51 MB): lazy %.3f dense %.3f" % (lazy, dense), flush=True)
    assert lazy < 1.0 and dense > 1.0
    assert all(g is None for g in grads)


# ------------------------------------------------------------------------------------------------ 8: fall-backs
@pytest.mark.parametrize("extra,emb,word", [(["--buir_native", "0"], "64", "buir_native"),
                                            (["--buir_native", "1", "--optimizer", "Adagrad"], "64", "Adagrad"),
                                            (["--buir_native", "1"], "20", "embedding_size=20")])
def test_fallbacks_train_on_the_dense_path_and_log_once(extra, emb, word, caplog):
    opt = "Adagrad" if "Adagrad" in extra else "Adam"
    extra = [a for a in extra if a not in ("--optimizer", "Adagrad")]
    with caplog.at_level(logging.WARNING):
        _, model, _, data, run = _setup(opt, extra + ["--emb_lazy", "1"], emb=emb)
        assert model.emb_lazy is False and model.optimizer is None
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        loss = run.fit(data, epoch=1)
    said = [r.getMessage() for r in caplog.records if "--emb_lazy 1" in r.getMessage() or "--buir_native 1" in r.getMessage()]
    assert len(said) == 1 and "--emb_lazy 1" in said[0] and word in said[0], said
    assert np.isfinite(loss) and isinstance(model.optimizer, torch.optim.Optimizer)
    assert model.user_online.weight.grad is not None
    assert all(not torch.equal(v, before[k]) for k, v in model.state_dict().items())
