"""Adam, Adagrad and Adadelta steps against a float64 reference, measured on the update and on the optimizer state
(oracle/optim_parity.py: the regimes, the measured fp32 floors and the tolerances derived from them; tests/test_optim_power.py:
what these checks can see).  Every run here is one entry of optim_parity.VARIANTS in one of the forms the library offers for
it, and every form must meet the float64 reference — not only the project's own dense kernel."""
import numpy as np
import pytest
import torch

from oracle import optim_parity as op

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _T(a, dtype=None):
    t = torch.from_numpy(np.array(a))                     # a copy: the cases' arrays are shared and read-only
    return (t if dtype is None else t.to(dtype)).to(_dev())


def _setup(variant, overlap=False):
    """(hip_ops, case data, float64 reference, fresh device tables, plan) of one entry of optim_parity.VARIANTS"""
    from whisprrec_amd import hip_ops
    c, ref = op.variant_reference(*variant)
    u, p, n = (_T(c[k], torch.int32) for k in "upn")
    if overlap:
        arena = hip_ops.PlanArena(_dev(), u.numel(), c["B"], overlap_items=c["nI"])
        plan = hip_ops.BatchPlan(u, p, n, c["B"], c["nU"], c["nI"], arena=arena, overlap=True)
    else:
        plan = hip_ops.BatchPlan(u, p, n, c["B"], c["nU"], c["nI"])
    return hip_ops, c, ref, hip_ops.BprmfTables(_T(c["U0"]), _T(c["I0"])), plan


def _adam_dense(ops, tabs, plan, steps, lr, l2):
    """wr_bprmf_grads + wr_adam_dense on both tables, every step: (losses, state)"""
    z = torch.zeros_like
    gU, gI, mU, vU, mI, vI = z(tabs.U), z(tabs.I), z(tabs.U), z(tabs.U), z(tabs.I), z(tabs.I)
    losses = []
    for k in range(steps):
        loss, sid = tabs.grads(plan, k, gU, gI)
        losses.append(loss.clone())
        ops.adam_dense(tabs.U, mU, vU, gU, k + 1, lr, l2, stamp=tabs.stamp_u, step_id=sid)
        ops.adam_dense(tabs.I, mI, vI, gI, k + 1, lr, l2, stamp=tabs.stamp_i, step_id=sid)
    return torch.stack(losses), {"m": (mU, mI), "v": (vU, vI)}


def _adam_lazy(st, plan, steps):
    """the native loop in two calls, then flush(): (losses, state)"""
    cut = max(2, steps // 3)
    losses = torch.cat([st.run(plan, 0, cut), st.run(plan, cut, steps - cut)])
    behind = (int(st.last_u.min()), int(st.last_i.min()))
    st.flush()
    torch.cuda.synchronize()
    return losses, op.state_of(st), behind


def _check(tag, key, ref, tabs, losses, state):
    torch.cuda.synchronize()
    return op.check_optim_run(tag, ref, tabs.U, tabs.I, losses, op.TOL[key], state)


# --------------------------------------------------------------------------------------------------- A: the eps regime
@pytest.mark.parametrize("form", ["dense", "default", "unfolded"])
def test_eps_regime_large_batch(form):
    """70K x 200K, B = 8,192, tables N(0, 0.01^2): the gradients are a few 1e-7, eps = 1e-8 is percent-level in the
    denominator.  default: rows / B = 24, so the catch-up is folded into the step kernels, and with the overlap marks in the
    plan the steps go out as one launch each (wr_bprmf_run_adam_folded_chain)."""
    variant = op.VARIANTS["A"][0]
    ops, c, ref, tabs, plan = _setup(variant, overlap=form == "default")
    assert op.median_abs_grad(ref) < 100 * 1e-8
    if form == "dense":
        losses, state = _adam_dense(ops, tabs, plan, c["steps"], c["lr"], 0.0)
    else:
        st = ops.LazyOptimizerState(tabs, "Adam", c["lr"], 0.0, **({} if form == "default" else {"fold": False}))
        if form == "default":
            assert plan.overlap is not None and plan.hot is None and st._folds(plan)
        losses, state, _ = _adam_lazy(st, plan, c["steps"])
        tabs.check_chain()
        assert (st.chain_calls > 0) == (form == "default")
    _check("A %s" % form, "A", ref, tabs, losses, state)


def test_eps_regime_d128():
    variant = op.VARIANTS["A"][1]
    ops, c, ref, tabs, plan = _setup(variant, overlap=True)
    st = ops.LazyOptimizerState(tabs, "Adam", c["lr"], 0.0)
    losses, state, _ = _adam_lazy(st, plan, c["steps"])
    tabs.check_chain()
    assert st.chain_calls > 0
    _check("A D=128 default", "A", ref, tabs, losses, state)


# --------------------------------------------------------------------------------------------------- B: long gaps
@pytest.mark.parametrize("form", ["default", "max_lag_0", "dense"])
@pytest.mark.parametrize("key,i", [("B", 0), ("B", 1), ("B_l2", 0), ("B_l2", 1)])
def test_long_gaps_small_batch(key, i, form):
    """10K x 8K, B = 64, 160 steps: a row misses ~156 steps between two uses, so the default is the bounded lag
    (wr_bprmf_run_adam_lazy_bounded); bias corrections and the constants table at steps well past 50.  With l2 > 0 every row
    moves at every step: the reference runs on the whole tables."""
    variant = op.VARIANTS[key][i]
    ops, c, ref, tabs, plan = _setup(variant)
    l2, steps = variant[4], c["steps"]
    assert (ref["rows"] is None) == (l2 > 0)
    if form == "dense":
        losses, state = _adam_dense(ops, tabs, plan, steps, c["lr"], l2)
    else:
        st = ops.LazyOptimizerState(tabs, "Adam", c["lr"], l2, **({} if form == "default" else {"max_lag": 0}))
        assert not st._folds(plan)
        assert ops._auto_lag(st, plan) == (st.MAX_LAG if form == "default" else 0)
        losses, state, behind = _adam_lazy(st, plan, steps)
        # before the flush: the window keeps every row within MAX_LAG steps; without it rows no batch has are still at 0
        assert min(behind) >= steps - 1 - st.MAX_LAG if form == "default" else min(behind) == 0
    _check("%s D=%d %s" % (key, variant[2], form), key, ref, tabs, losses, state)


def test_adam_consts_match_the_float64_formulas_across_a_growth():
    """wr_adam_consts, steps 1 .. 8,192 (LazyOptimizerState starts with 4,096 entries and doubles): step_size = lr / (1 -
    beta1^t) and 1 / sqrt(1 - beta2^t) evaluated in float64 at the fp32 lr and betas the entry point receives, to one fp32
    rounding; entry 0 is the neutral (0, 1); growing the table changes no entry.  Printed as well: the distance to the same
    formulas at the double betas 0.9 / 0.999 that torch uses (1 - float(0.999) is 1.3e-5 below 0.001)."""
    from whisprrec_amd import hip_ops
    lr, b1, b2 = 1e-3, 0.9, 0.999
    small, big = hip_ops.adam_consts(4096, lr, b1, b2).numpy().reshape(-1, 2), hip_ops.adam_consts(8193, lr, b1, b2).numpy().reshape(-1, 2)
    assert np.array_equal(small, big[:4096]) and tuple(big[0]) == (0.0, 1.0)
    t = np.arange(1, 8193, dtype=np.float64)
    f = lambda x: float(np.float32(x))
    want = np.stack([f(lr) / (1.0 - f(b1) ** t), 1.0 / np.sqrt(1.0 - f(b2) ** t)], axis=1)
    got = big[1:].astype(np.float64)
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    worst = float(np.max(np.abs(got - want) / ulp))
    torch_way = np.stack([lr / (1.0 - b1 ** t), 1.0 / np.sqrt(1.0 - b2 ** t)], axis=1)
    print("adam consts 1..8192: worst |c - c64| = %.3f ulp; against double betas: %.2e relative (step %d)" % (
        worst, float(np.max(np.abs(got - torch_way) / torch_way)), int(np.argmax(np.max(np.abs(got - torch_way) / torch_way, axis=1))) + 1))
    assert worst <= 0.5 + 1e-3, worst
    st = hip_ops.LazyOptimizerState(hip_ops.BprmfTables(torch.zeros(4, 16, device=_dev()), torch.zeros(4, 16, device=_dev())),
                                    "Adam", lr, 0.0)
    assert st.n_consts == 4096 and np.array_equal(st.consts.cpu().numpy().reshape(-1, 2), small)
    st._grow_consts(2 * st.n_consts)
    assert np.array_equal(st.consts.cpu().numpy().reshape(-1, 2), big[:8192])


# --------------------------------------------------------------------------------------------------- C: hot rows
@pytest.mark.parametrize("form", ["default", "dense"])
@pytest.mark.parametrize("key", ["C", "C_l2"])
def test_hot_rows(key, form):
    """D = 32, Zipf items and a hot user: the plan has hot runs, the step takes the pieces + combine kernels"""
    variant = op.VARIANTS[key][0]
    ops, c, ref, tabs, plan = _setup(variant)
    assert plan.hot is not None and int(plan.hot["counts_host"].view(-1, 4)[:, 3].min()) >= 1
    if form == "dense":
        losses, state = _adam_dense(ops, tabs, plan, c["steps"], c["lr"], variant[4])
    else:
        losses, state, _ = _adam_lazy(ops.LazyOptimizerState(tabs, "Adam", c["lr"], variant[4]), plan, c["steps"])
    _check("%s %s" % (key, form), key, ref, tabs, losses, state)


# --------------------------------------------------------------------------------------------------- D: saturated scores
@pytest.mark.parametrize("form", ["default", "unfolded", "dense"])
def test_saturated_scores(form):
    """tables N(0, 0.7^2): score differences reach +-19, gradient elements span 1e-2 .. 2e-11, v goes down to 4e-29"""
    variant = op.VARIANTS["D"][0]
    ops, c, ref, tabs, plan = _setup(variant)
    if form == "dense":
        losses, state = _adam_dense(ops, tabs, plan, c["steps"], c["lr"], 0.0)
    else:
        st = ops.LazyOptimizerState(tabs, "Adam", c["lr"], 0.0, **({} if form == "default" else {"fold": False}))
        losses, state, _ = _adam_lazy(st, plan, c["steps"])
    _check("D %s" % form, "D", ref, tabs, losses, state)


# --------------------------------------------------------------------------------------------------- E: Adagrad, Adadelta
def _stateful_variants():
    out = []
    for key in ("E_adagrad", "E_adagrad_zipf", "E_adadelta"):
        for i, v in enumerate(op.VARIANTS[key]):
            for lag in ((0,) if v[0] == "Adagrad" else (0, 1, 3)):
                out.append(pytest.param(key, i, lag, id="%s-D%d-%s-lag%d" % (v[0], v[2], "zipf" if v[3] else "uniform", lag)))
    return out


@pytest.mark.parametrize("key,i,lag", _stateful_variants())
def test_adagrad_adadelta_fused(key, i, lag):
    """the shape of test_hip_optimizers.py::test_sparse_fused_equals_dense_restatement; lag: Adadelta's rotating window"""
    variant = op.VARIANTS[key][i]
    ops, c, ref, tabs, plan = _setup(variant)
    assert plan.hot is not None or not variant[3]
    st = ops.StatefulSparseState(tabs, variant[0], ref["lr"], max_lag=lag)
    steps = plan.n_batches
    losses = torch.cat([st.run(plan, 0, 5), st.run(plan, 5, steps - 5)])
    if lag:
        assert int(st.last_u.min()) >= steps - 1 - lag
    _check("%s D=%d %s lag %d" % (variant[0], variant[2], "zipf" if variant[3] else "uniform", lag), key, ref, tabs, losses,
           op.state_of(st))


def test_adadelta_long_gaps():
    """Adadelta at regime B's shape: a row misses ~150 decays between two updates; the default is the bounded lag"""
    variant = op.VARIANTS["E_gaps"][0]
    ops, c, ref, tabs, plan = _setup(variant)
    st = ops.StatefulSparseState(tabs, "Adadelta", ref["lr"])
    assert ops._auto_lag(st, plan) == st.MAX_LAG
    losses = torch.cat([st.run(plan, 0, 70), st.run(plan, 70, c["steps"] - 70)])
    assert int(st.last_u.min()) >= c["steps"] - 1 - st.MAX_LAG
    _check("E_gaps default", "E_gaps", ref, tabs, losses, op.state_of(st))
