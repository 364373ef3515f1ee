"""The forms of the row-lazy optimizers that hold four rows per wave, and the stride loops of their catch-up, on the GPU
(whisprrec_amd/csrc/wr_rowopt.hip, wr_lazy.hip; hip_ops.RowLazyTable, RowLazyEmaTable, LazyOptimizerState).

Both sources pick a kernel form by the size of a call: below 32,768 positions / rows / keys a wave holds one row (R = 1), from
there on four (R = 4), and the R = 4 catch-up walks a table in strides of 256 * 32 workgroups x 4 waves x 4 rows = 131,072 rows.
The cases of tests/test_hip_emb_lazy.py, test_hip_buir_lazy.py and test_hip_lazy_optim.py stay below those sizes; the cases here
(tests/rowopt_ref.py WIDE_CASES / RUN_CASES, tests/buir_lazy_ref.py, oracle/optim_parity.py regime F) are the smallest above
them, and tests/test_emb_lazy_contract.py::test_wide_cases_cross_the_thresholds_of_the_sources reads the sizes out of the
sources.  Tolerances: TOL_WIDE of the two contract modules and optim_parity.TOL["F"], ["F_l2"], TOL_F_SGD — 8 x the fp32 floor.

Inventory — the instance, and the test that runs it against the dense kernels bit for bit and against float64:
  gather_rows_kernel<ADAM, L2, EMA, 4>, the seven launched ones (32,771 positions, tail group of three, ids outside the table)
    <1,0,0> <1,1,0> <0,1,0> (one table: Adam l2 = 0, Adam l2, SGD) <1,1,1> <1,0,1> <0,1,1> <0,0,1> (pair: Adam, SGD, both l2)
                                                        test_gather_on_both_sides_of_the_threshold (a)
  catchup_ema_kernel<ADAM, L2, 4> x 4, its stride loop (140,003 rows at the flush), windows of 35,001 rows that start at rows
    that are no multiples of 4 (max_lag 4) and of 70,002 rows (max_lag 2)
                                                        test_wide_tables_hold_the_bits_of_the_dense_kernels[pair-*] (b)
  adam_catchup_all_kernel<false, 4>, <true, 4>, sgd_catchup_all_kernel<4> through RowLazyTable: the flush and its stride loop,
    the same windows                                    test_wide_tables_hold_the_bits_of_the_dense_kernels[one-*] (b)
  rows_sparse_kernel / run_sum (no R): 40,003 positions per step in (b); runs of exactly 1, 15, 16, 17, 63, 64, 65, 128, 129
    and 300 positions, a run that ends on a 64-entry trip in the middle of a step and at its last position, D = 100
                                                        test_run_lengths_hold_the_bits_of_the_dense_kernels (c)
  adam_lazy_rows_kernel<false, 4>, <true, 4> (32,768 user keys, 65,536 item keys; the short last batch has 21,846 user keys: R = 1
    again), adam_catchup_all_kernel<*, 4> on 70,001 and 140,003 rows (flush) and on windows of 35,001 / 70,002 rows
                                                        test_bprmf_adam_at_four_rows_per_wave (d)
  sgd_lazy_rows_kernel<4>, sgd_catchup_all_kernel<4> on the tables and on the same windows
                                                        test_bprmf_sgd_weight_decay_at_four_rows_per_wave (d)

Recorded on an MI355X (every test prints its "parity ..." line with the margin tolerance / figure; the lags give the same
bits, so the same figures).  Smallest margin of a measure over the cases of a group, with the figure it belongs to:
    wide, one table  Adam: update 26 x (1.53e-5), row 17 x (2.38e-5), state 15 x (1.31e-5); SGD: update 9.9 x (5.04e-7), row 8.3 x
                     (9.64e-6)
    wide, pair       Adam: update 15 x, row 18 x, state 15 x, t_update 17 x (1.78e-3), t_row 9.1 x (2.20e-2); SGD: update 9.8 x, row
                     8.9 x, t_update 8.3 x (1.08e-6), t_row 8.1 x (3.69e-5)
    runs, one table  Adam: update / row 29 x (1.37e-5, D = 100), state 15 x; SGD: update 11 x (4.50e-7), row 43 x
    runs, pair       Adam: update 14 x, row 21 x, state 15 x, t_update 8.5 x (3.54e-3), t_row 15 x; SGD: update 8.9 x, row 28 x,
                     t_update 10 x, t_row 16 x
    regime F         all four forms alike — F: update 8.2 x (4.86e-6), row 6.8 x (7.36e-6), state 15 x, table 27 x; F_l2: update /
                     row 9.0 x (2.22e-5 / 2.23e-5), state 15 x, table 11 x; SGD with decay: update 9.2 x (3.25e-6), row 10 x (5.02e-6)
The whole file takes 15 s; the slowest test 1.3 s (the first one of a case builds its float64 reference, 140,003 x 64).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buir_lazy_ref as B  # noqa: E402
import rowopt_ref as R  # noqa: E402
import test_buir_lazy_contract as BC  # noqa: E402
import test_emb_lazy_contract as EC  # noqa: E402
from oracle import optim_parity as op, parity  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 12345.0


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ the two faces, one interface
# kind "one": a case is (n_rows, D, padding_idx, l2) of rowopt_ref; kind "pair": (n_rows, D, l2, momentum) of buir_lazy_ref
def _l2(kind, case):
    return case[3] if kind == "one" else case[2]


def _pad(kind, case):
    return case[2] if kind == "one" else -1


def _lr(opt):
    return R.LR[opt]


@functools.lru_cache(maxsize=None)
def _device_case(kind, case):
    """(W0, steps, the 320-position query of the per-step gather check) on the device: shared, never modified"""
    n_rows = case[0]
    W0, steps = (R if kind == "one" else B).make_any_case(case)
    rng = np.random.RandomState(99)
    head = [0, 0, R.HOT_ROW, R.HOT_ROW, 1, 2, n_rows - 1, n_rows - 1, n_rows - 3]
    if n_rows == R.WIDE_ROWS:
        head += [12, 13, 14, 15] + [row for row, _ in R.WIDE_GAP_ROWS.values()] + [row for row, _ in R.WIDE_HIGH_GAP_ROWS.values()]
        head += list(R.WIDE_ONCE_ROWS) + [b + j for b in R.WIDE_MIX_ROW0 for j in range(8)] + sorted(R.wide_edge_rows(n_rows))
    else:
        head += sorted(set(R.RUN_ROW_OF[0].values()))
    q = np.concatenate([head, rng.randint(0, n_rows, 320 - len(head))]).astype(np.int64).reshape(4, 80)
    return _t(W0), [(_t(i), _t(s)) for i, s in steps], _t(q)


def _new_table(kind, opt, case, max_lag):
    from whisprrec_amd import hip_ops
    W0, _, _ = _device_case(kind, case)
    if kind == "one":
        return hip_ops.RowLazyTable(W0.clone(), opt, _lr(opt), case[3], max_lag=max_lag, padding_idx=case[2])
    return hip_ops.RowLazyEmaTable(W0.clone(), W0.clone(), opt, _lr(opt), case[2], case[3], max_lag=max_lag)


def _dense_arm(kind, opt, case, n_steps=None, query=None):
    """zero table, scatter_add_rows, adam_dense / sgd_dense (a pair: then ema_update_), step by step.
    -> ({"w", "tgt", "m", "v"}, {t: the rows of `query` before step t, as the lazy gather returns them}, gather(q): the rows
    of another query from the tables as they stand now)"""
    from whisprrec_amd import hip_ops
    W0, steps, _ = _device_case(kind, case)
    W, m, v = W0.clone(), torch.zeros_like(W0), torch.zeros_like(W0)
    T = W0.clone() if kind == "pair" else None
    rows = {}

    def gather(q):
        got = hip_ops.gather_rows(W, q)
        return got if T is None else (got, hip_ops.gather_rows(T, q))

    for t, (idx, src) in enumerate(steps[:n_steps], start=1):
        if query is not None:
            rows[t] = gather(query)
        G = torch.zeros_like(W)
        hip_ops.scatter_add_rows(G, idx, src, padding_idx=_pad(kind, case))
        if opt == "Adam":
            hip_ops.adam_dense(W, m, v, G, t, _lr(opt), _l2(kind, case))
        else:
            hip_ops.sgd_dense(W, G, _lr(opt), _l2(kind, case))
        if T is not None:
            hip_ops.ema_update_(T, W, case[3])
    return {"w": W, "tgt": T, "m": m if opt == "Adam" else None, "v": v if opt == "Adam" else None}, rows, gather


@functools.lru_cache(maxsize=None)
def _dense_run(kind, opt, case):
    """the whole dense arm of a case with the per-step rows of the 320-position query: computed once, shared by the lags"""
    out, rows, _ = _dense_arm(kind, opt, case, query=_device_case(kind, case)[2])
    return out, rows


def _state(tab):
    return [x.clone() for x in (tab.w, tab.tgt, tab.m, tab.v, tab.last) if x is not None]


def _same_state(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _as_pair(x):
    return x if isinstance(x, tuple) else (x,)


def _assert_bits(tab, dense, what):
    for name in ("w", "tgt", "m", "v"):
        got, want = getattr(tab, name), dense[name]
        assert (got is None) == (want is None), (what, name)
        if got is not None:
            assert torch.equal(got, want), (what, name, float((got - want).abs().max()))


def _figures(kind, opt, case, tab):
    """-> (the figures of the flushed table against the float64 loop, [(name, tolerance)])"""
    state = {"m": tab.m.cpu().numpy(), "v": tab.v.cpu().numpy()} if opt == "Adam" else {}
    if kind == "one":
        W0, _, ref, _ = EC.wide_runs(opt, case)
        fig = EC.figures(W0, ref, (tab.w.cpu().numpy(), state))
        names = ["update", "row"] + (["state"] if opt == "Adam" else [])
        return fig, [(n, EC.TOL_WIDE[opt][n]) for n in names]
    W0, _, ref, _ = BC.wide_runs(opt, case)
    fig = BC.figures(W0, ref, (tab.w.cpu().numpy(), tab.tgt.cpu().numpy(), state))
    names = ["update", "row", "t_update", "t_row"] + (["state"] if opt == "Adam" else [])
    return fig, [(n, BC.tol_wide(opt, n, case[3])) for n in names]


def _check_float64(tag, kind, opt, case, tab):
    fig, bounds = _figures(kind, opt, case, tab)
    print("parity rowopt_wide %s %s %s %s: update/table %.1e | %s" % (
        tag, kind, opt, case, fig["update_over_table"],
        " ".join("%s_err %.2e (tol %.0e, margin %.1f x)" % (n, fig[n], b, b / max(fig[n], 1e-300)) for n, b in bounds)), flush=True)
    for n, b in bounds:
        assert fig[n] < b, (n, fig)


# ------------------------------------------------------------------------------------------------ a: the gather threshold
# the seven gather_rows_kernel<ADAM, L2, EMA, 4> that are launched (one table under SGD without decay keeps no state and
# gathers with wr_gather_rows)
GATHER_FACES = [("one", "Adam", R.WIDE_CASES[0]), ("one", "Adam", R.WIDE_CASES[1]), ("one", "SGD", R.WIDE_CASES[1]),
                ("pair", "Adam", B.WIDE_CASES[0]), ("pair", "Adam", B.WIDE_CASES[1]),
                ("pair", "SGD", B.WIDE_CASES[0]), ("pair", "SGD", B.WIDE_CASES[1])]


@pytest.mark.parametrize("kind,opt,case", GATHER_FACES, ids=["%s-%s-D%d-l2_%g" % (k, o, c[1], _l2(k, c)) for k, o, c in GATHER_FACES])
def test_gather_on_both_sides_of_the_threshold(kind, opt, case):
    """the table after three wide steps, unflushed: the gather of 32,771 positions (four per wave, a tail group of three)
    against gather_rows on the dense arm's tables and against the gathers of its first 32,767 (one per wave) and 32,768
    positions; nothing but the output is written, not even next to it; ids outside the table come back as zero rows"""
    from whisprrec_amd import hip_ops
    n_rows, D = case[0], case[1]
    assert {(k, o, _l2(k, c) != 0) for k, o, c in GATHER_FACES} == {
        ("one", "Adam", False), ("one", "Adam", True), ("one", "SGD", True),
        ("pair", "Adam", True), ("pair", "Adam", False), ("pair", "SGD", True), ("pair", "SGD", False)}
    q = _t(R.make_wide_query(n_rows))
    n = q.numel()
    assert n == R.WIDE_GATHER_N == 32771
    _, steps, _ = _device_case(kind, case)
    _, _, dense_gather = _dense_arm(kind, opt, case, n_steps=3)
    want = _as_pair(dense_gather(q))
    tab = _new_table(kind, opt, case, 0)
    for idx, src in steps[:3]:
        tab.step([idx], [src])
    assert tab.stateful and tab.t == 3 and tab.behind() == 3
    last = tab.last[q]
    assert {0, 1, 2, 3} <= set(last[:64].tolist()) and int(last[0]) == 3                     # current and late rows side by side
    keep = _state(tab)
    got = _as_pair(tab.gather(q))
    assert len(got) == len(want) == (1 if kind == "one" else 2)
    for g, w in zip(got, want):
        assert g.shape == (n, D) and torch.equal(g, w), float((g - w).abs().max())           # R = 4 against the dense arm
    for cut in (32767, 32768):                                                               # R = 1, and the first R = 4 size
        part = _as_pair(tab.gather(q[:cut]))
        assert all(torch.equal(p, g[:cut]) for p, g in zip(part, got)), cut
    assert _same_state(keep, _state(tab))                                                    # nothing but the output is written
    # once through the entry with the outputs inside larger buffers: the rows on both sides of them stay as they were
    bufs = [torch.full((n + 16, D), SENTINEL, device=DEV) for _ in got]
    outs = [b[8:8 + n] for b in bufs]
    tab._call("gather", 0, n_rows, (hip_ops._p(q), n, tab.t), (*map(hip_ops._p, outs), hip_ops._p(tab.err)))
    tab.check()
    for b, g in zip(bufs, got):
        assert torch.equal(b[8:8 + n], g) and bool((b[:8] == SENTINEL).all()) and bool((b[8 + n:] == SENTINEL).all())
    # ids outside the table in one group of four, unchecked: zero rows, the neighbours right, the finding waits for check()
    bad = q.clone()
    bad[41], bad[42] = n_rows, -1
    assert 40 % 4 == 0
    rows = _as_pair(tab.gather(bad, check=False))
    ok = torch.ones(n, dtype=torch.bool, device=DEV)
    ok[41] = ok[42] = False
    for r, g in zip(rows, got):
        assert not r[41].any() and not r[42].any() and torch.equal(r[ok], g[ok]) and bool(g[40].any()) and bool(g[43].any())
    with pytest.raises(IndexError):
        tab.check()
    tab.check()                                                                              # raised once, then cleared
    assert _same_state(keep, _state(tab))


# ------------------------------------------------------------------------------------------------ b: wide tables
def _wide_params():
    out = []
    for kind, cases in (("one", R.WIDE_CASES), ("pair", B.WIDE_CASES)):
        for case in cases:
            for opt in ("Adam", "SGD"):
                for lag in R.WIDE_LAGS:
                    out.append(pytest.param(kind, opt, case, lag, id="%s-%s-D%d-l2_%g-lag%d" % (kind, opt, case[1], _l2(kind, case), lag)))
    return out


@pytest.mark.parametrize("kind,opt,case,lag", _wide_params())
def test_wide_tables_hold_the_bits_of_the_dense_kernels(kind, opt, case, lag):
    """140,003 rows, steps of 40,003 / 333 / 0 / 1 positions: the gather before every step, the window (max_lag 4: 35,001 rows
    from rows that are no multiples of 4; max_lag 2: 70,002 rows) and the flush (more than one stride of 131,072 rows) leave the
    bits of the dense kernels, and the flushed tables meet the float64 loop"""
    n_rows, D = case[0], case[1]
    dense, dense_rows = _dense_run(kind, opt, case)
    _, steps, q = _device_case(kind, case)
    tab = _new_table(kind, opt, case, lag)
    behind = []
    for t, (idx, src) in enumerate(steps, start=1):
        keep = _state(tab)
        got = _as_pair(tab.gather(q))
        for g, w in zip(got, _as_pair(dense_rows[t])):
            assert g.shape == q.shape + (D,) and torch.equal(g, w), (t, float((g - w).abs().max()))
        assert _same_state(keep, _state(tab)), t
        if tab.stateful:
            behind.append(tab.behind())
        tab.step([idx], [src])
        assert tab.t == t
    assert tab.t == R.WIDE_N_STEPS == 6
    if tab.stateful:
        behind.append(tab.behind())
        if lag:
            assert max(behind) <= lag + 1, behind                                # the bound, before the flush
        else:
            assert behind[-1] == tab.t                                           # the never-used rows
            assert int(tab.last[R.WIDE_STRIDE:].max()) > 0 and int(tab.last[R.WIDE_STRIDE:].min()) == 0
    else:
        assert (kind, opt, _l2(kind, case)) == ("one", "SGD", 0.0)
    tab.flush()
    if tab.stateful:
        assert int(tab.last.min()) == int(tab.last.max()) == tab.t and tab.behind() == 0
    _assert_bits(tab, dense, lag)
    _check_float64("lag %d" % lag, kind, opt, case, tab)


# ------------------------------------------------------------------------------------------------ c: run lengths
def _run_params():
    return [pytest.param(kind, opt, case, id="%s-%s-D%d-l2_%g" % (kind, opt, case[1], _l2(kind, case)))
            for kind, cases in (("one", R.RUN_CASES), ("pair", B.RUN_CASES)) for case in cases for opt in ("Adam", "SGD")]


@pytest.mark.parametrize("kind,opt,case", _run_params())
def test_run_lengths_hold_the_bits_of_the_dense_kernels(kind, opt, case):
    """runs of exactly 1, 15, 16, 17, 63, 64, 65, 128, 129 and 300 positions in one step, the run of 128 (step 2: of 64) at the
    step's last positions; D = 100 has lanes without an element in the second element trip"""
    dense, dense_rows = _dense_run(kind, opt, case)
    _, steps, q = _device_case(kind, case)
    tab = _new_table(kind, opt, case, None)
    for t, (idx, src) in enumerate(steps, start=1):
        for g, w in zip(_as_pair(tab.gather(q)), _as_pair(dense_rows[t])):
            assert torch.equal(g, w), t
        tab.step([idx], [src])
    tab.flush()
    _assert_bits(tab, dense, "runs")
    _check_float64("runs", kind, opt, case, tab)


# ------------------------------------------------------------------------------------------------ d: BPRMF at regime F
def _T(a, dtype=None):
    t = torch.from_numpy(np.array(a))                     # a copy: the cases' arrays are shared and read-only
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _f_setup(c):
    from whisprrec_amd import hip_ops
    u, p, n = (_T(c[k], torch.int32) for k in "upn")
    plan = hip_ops.BatchPlan(u, p, n, c["B"], c["nU"], c["nI"])
    assert plan.hot is None and plan.n_batches == c["steps"] == 4
    return hip_ops, hip_ops.BprmfTables(_T(c["U0"]), _T(c["I0"])), plan


@functools.lru_cache(maxsize=None)
def _f_adam_dense(key):
    """wr_bprmf_grads + wr_adam_dense on both tables, every step: (U, I, losses, state), shared by the forms"""
    variant = op.VARIANTS[key][0]
    c, _ = op.variant_reference(*variant)
    ops, tabs, plan = _f_setup(c)
    z = torch.zeros_like
    gU, gI, mU, vU, mI, vI = z(tabs.U), z(tabs.I), z(tabs.U), z(tabs.U), z(tabs.I), z(tabs.I)
    losses = []
    for k in range(c["steps"]):
        loss, sid = tabs.grads(plan, k, gU, gI)
        losses.append(loss.clone())
        ops.adam_dense(tabs.U, mU, vU, gU, k + 1, c["lr"], variant[4], stamp=tabs.stamp_u, step_id=sid)
        ops.adam_dense(tabs.I, mI, vI, gI, k + 1, c["lr"], variant[4], stamp=tabs.stamp_i, step_id=sid)
    torch.cuda.synchronize()
    return tabs.U, tabs.I, torch.stack(losses), {"m": (mU, mI), "v": (vU, vI)}


@pytest.mark.parametrize("form", ["dense", "default", "unfolded", "unfolded_lag2"])
@pytest.mark.parametrize("key", ["F", "F_l2"])
def test_bprmf_adam_at_four_rows_per_wave(key, form):
    """70,001 x 140,003, B = 32,768, 4 steps, short last batch.  default: rows / B = 4, folded (the flush is
    adam_catchup_all_kernel<L2, 4> over more than one stride); unfolded: wr_adam_rows_lazy on 32,768 user keys and 65,536 item
    keys (adam_lazy_rows_kernel<L2, 4>); unfolded_lag2: before every step windows of 35,001 and 70,002 rows.  Every form meets
    the float64 reference, the unfolded forms also the bits of the dense kernels."""
    variant = op.VARIANTS[key][0]
    c, ref = op.variant_reference(*variant)
    l2 = variant[4]
    assert (ref["rows"] is None) == (l2 > 0)
    Ud, Id, losses_d, state_d = _f_adam_dense(key)
    if form == "dense":
        op.check_optim_run("%s D=%d dense" % (key, variant[2]), ref, Ud, Id, losses_d, op.TOL[key], state_d)
        return
    ops, tabs, plan = _f_setup(c)
    kw = {"default": {}, "unfolded": {"fold": False, "max_lag": 0}, "unfolded_lag2": {"fold": False, "max_lag": 2}}[form]
    st = ops.LazyOptimizerState(tabs, "Adam", c["lr"], l2, **kw)
    assert st._folds(plan) == (form == "default") and ops._auto_lag(st, plan) == kw.get("max_lag", 0)
    losses = torch.cat([st.run(plan, 0, 2), st.run(plan, 2, c["steps"] - 2)])
    behind = (int(st.last_u.min()), int(st.last_i.min()))
    if form == "unfolded_lag2":
        assert min(behind) >= c["steps"] - 1 - 2, behind
    else:
        assert min(behind) == 0, behind                    # rows no batch has: the flush replays them (whole tables, four per wave)
    st.flush()
    torch.cuda.synchronize()
    assert int(st.last_u.min()) == int(st.last_i.min()) == c["steps"]
    state = op.state_of(st)
    op.check_optim_run("%s D=%d %s" % (key, variant[2], form), ref, tabs.U, tabs.I, losses, op.TOL[key], state)
    if form != "default":
        assert torch.equal(losses, losses_d)
        for a, b in ((tabs.U, Ud), (tabs.I, Id), (st.m_u, state_d["m"][0]), (st.m_i, state_d["m"][1]),
                     (st.v_u, state_d["v"][0]), (st.v_i, state_d["v"][1])):
            assert torch.equal(a, b), (form, float((a - b).abs().max()))


@functools.lru_cache(maxsize=None)
def _f_sgd_dense():
    c, _ = op.sgd_f_reference()
    _, tabs, plan = _f_setup(c)
    losses = torch.stack([tabs.step_sgd(plan, k, op.F_SGD["lr"], op.F_SGD["l2"]).clone() for k in range(c["steps"])])
    torch.cuda.synchronize()
    return tabs.U, tabs.I, losses


@pytest.mark.parametrize("max_lag", [0, 2])
def test_bprmf_sgd_weight_decay_at_four_rows_per_wave(max_lag):
    """LazyOptimizerState("SGD", lr, 1e-2) at regime F's shape: sgd_lazy_rows_kernel<4> on the batch's keys,
    sgd_catchup_all_kernel<4> on the windows (max_lag 2) and at the flush — the bits of step_sgd with dense decay, and the
    update against float64 SGD with weight decay"""
    c, ref = op.sgd_f_reference()
    lr, l2 = op.F_SGD["lr"], op.F_SGD["l2"]
    Ud, Id, losses_d = _f_sgd_dense()
    ops, tabs, plan = _f_setup(c)
    st = ops.LazyOptimizerState(tabs, "SGD", lr, l2, max_lag=max_lag)
    losses = torch.cat([st.run(plan, 0, 2), st.run(plan, 2, c["steps"] - 2)])
    behind = min(int(st.last_u.min()), int(st.last_i.min()))
    assert behind >= c["steps"] - 1 - max_lag if max_lag else behind == 0
    st.flush()
    torch.cuda.synchronize()
    assert int(st.last_u.min()) == int(st.last_i.min()) == c["steps"]
    assert torch.equal(losses, losses_d) and torch.equal(tabs.U, Ud) and torch.equal(tabs.I, Id)
    fig = parity.sgd_run_errors(c["U0"], c["I0"], ref, tabs.U.cpu().numpy(), tabs.I.cpu().numpy())
    loss_err = parity.table_err(losses.cpu().numpy().astype(np.float64), ref[2])
    tol = op.TOL_F_SGD
    print("parity F SGD D=64 max_lag %d: lr %.4g l2 %g update/table %.1e | update_err %.2e (tol %.0e) row_update_err %.2e (tol %.0e) "
          "table_err %.2e (tol %.0e) loss_err %.2e (tol %.0e)" % (
              max_lag, lr, l2, fig["update_over_table"], fig["update_err"], tol["update"], fig["row_update_err"], tol["row"],
              fig["table_err"], op.TOL_LOSS, loss_err, op.TOL_LOSS), flush=True)
    assert fig["update_err"] < tol["update"] and fig["row_update_err"] < tol["row"]
    assert fig["table_err"] < op.TOL_LOSS and loss_err < op.TOL_LOSS
