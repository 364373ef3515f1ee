"""What the optimizer parity checks can and cannot see (CPU only; oracle/optim_parity.py).

Floor: the fp32 oracle (oracle.bpr_dense_grads + adam_dense / adagrad_dense / adadelta_dense) against the float64 reference —
the reference against itself in lower precision, never the code under test — at every run of optim_parity.VARIANTS, the
runs of tests/test_hip_optim_parity.py.  optim_parity.TOL[regime] is 8 x the largest floor of the regime, rounded up to one
significant digit, and every floor leaves a factor 4.

Power: wrong steps, written here in NumPy fp32, must exceed the row_update_err tolerance of the regimes listed in SEES; the
same wrong steps at the shapes and learning rates of the tests that existed before stay under those tests' table bounds
(OLD_BOUND_MISSES), which is the recorded reason for the update-normalised checks.

Which regime sees what (SEES; everything is printed, the listed ones are asserted):
  - eps under the square root, eps added before the division by sqrt(bc2), bias correction of step t +- 1, one occurrence
    missing from a shared row's sum: every Adam regime.
  - one zero-gradient step of one row not replayed (l2 = 0): A, B and C.  Regime D cannot see it (7.9e-2 against a row
    tolerance of 2e-1: its floor is the conditioning of saturated gradients).  The bitwise tests of
    tests/test_hip_lazy_optim.py see it as well, as long as wr_adam_dense itself is right — which only these checks establish
    outside D = 64.
  - decoupled weight decay: the l2 regimes (B_l2, C_l2).
  - Adadelta replayed one rho decay short, every row: E_adadelta and E_gaps.  One row, once: E_adadelta only — in E_gaps the
    state has decayed by rho^150 before the row's next update, so one decay more or less is invisible there (1.1e-5, the floor).
  - Adagrad state not accumulated for one row in one step (the row's second): both Adagrad regimes.
  - regime F (the shape at which wr_lazy.hip's kernels hold four rows per wave) sees every Adam wrong step, smallest
    row_update_err: one missed replay step 1.99e-1 (F, tolerance 5e-5), one missing occurrence 1.36e-2 (F_l2, tolerance 2e-4).
    SGD with weight decay at that shape: one missed decay step of one row 2.5e-1 of the row's update (tolerance 5e-5).
"""
import functools
import math

import numpy as np
import pytest

import oracle
from conftest import rel_err
from oracle import load_golden, optim_parity as op, parity

F32 = np.float32
ADAM_MUTANTS = ("eps_under_sqrt", "eps_before_bc2", "bias_t_plus_1", "bias_t_minus_1", "replay_skip", "missing_occurrence")
L2_MUTANTS = ("decoupled_decay",)


# --------------------------------------------------------------------------------------------------- the fp32 oracle
def _oracle_run(opt, U0, I0, u, p, n, B, lr, l2=0.0):
    """the fp32 oracle, dense semantics: (U, I, state dict, losses)"""
    U, I = np.array(U0, dtype=F32), np.array(I0, dtype=F32)
    z = np.zeros_like
    S = {name: (z(U), z(I)) for name in op.STATE_NAMES[opt]}
    losses = []
    for k in range((u.size + B - 1) // B):
        sl = slice(k * B, (k + 1) * B)
        gU, gI, loss = oracle.bpr_dense_grads(U, I, u[sl], p[sl], n[sl])
        losses.append(loss)
        for side, (W, G) in enumerate(((U, gU), (I, gI))):
            if opt == "Adam":
                oracle.adam_dense(W, G, S["m"][side], S["v"][side], k + 1, lr, l2)
            elif opt == "Adagrad":
                oracle.adagrad_dense(W, G, S["state_sum"][side], lr)
            else:
                oracle.adadelta_dense(W, G, S["square_avg"][side], S["acc_delta"][side], lr)
    return U, I, S, np.asarray(losses)


@functools.lru_cache(maxsize=None)
def _floor(variant):
    c, ref = op.variant_reference(*variant)
    U, I, S, losses = _oracle_run(ref["opt"], ref["U0"], ref["I0"], *ref["ids"], ref["batch"], ref["lr"], ref["l2"])
    fig = op._errors(ref, U, I, S)
    fig["loss_err"] = parity.table_err(losses, ref["losses"])
    print("floor %s: update/table %.1e update_err %.2e row_update_err %.2e state_err %.2e table_err %.2e loss_err %.2e" % (
        variant, fig["update_over_table"], fig["update_err"], fig["row_update_err"], fig["state_err"], fig["table_err"],
        fig["loss_err"]))
    return fig


def _round_up_one_digit(x):
    e = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / e - 1e-9) * e


@pytest.mark.parametrize("key", list(op.VARIANTS))
def test_tolerances_are_eight_times_the_largest_floor(key):
    floors = [_floor(v) for v in op.VARIANTS[key]]
    for name, fig_key in (("update", "update_err"), ("row", "row_update_err"), ("state", "state_err")):
        worst = max(f[fig_key] for f in floors)
        assert math.isclose(op.TOL[key][name], _round_up_one_digit(8 * worst), rel_tol=1e-9), (key, name, worst)
        assert 4 * worst < op.TOL[key][name]
    worst = max(f["table_err"] for f in floors)
    assert math.isclose(op.TOL[key]["table"], max(op.TOL_LOSS, _round_up_one_digit(8 * worst)), rel_tol=1e-9), (key, worst)
    assert 4 * worst < op.TOL[key]["table"]
    assert op.TOL_LOSS == 1e-5 and all(4 * f["loss_err"] < op.TOL_LOSS for f in floors)


@functools.lru_cache(maxsize=None)
def _sgd_f_run(skip=None):
    """the fp32 C oracle's SGD with weight decay at regime F's shape; skip = (k, user row): the row is not in batch k and its
    decay of that step does not happen (a missed replay)"""
    c, _ = op.sgd_f_reference()
    U, I = np.array(c["U0"]), np.array(c["I0"])
    B, losses = c["B"], []
    for k in range(c["steps"]):
        sl = slice(k * B, (k + 1) * B)
        keep = U[skip[1]].copy() if skip is not None and k == skip[0] else None
        losses.append(oracle.bprmf_step_sgd(U, I, c["u"][sl], c["p"][sl], c["n"][sl], op.F_SGD["lr"], op.F_SGD["l2"]))
        if keep is not None:
            U[skip[1]] = keep
    return U, I, np.asarray(losses)


def test_sgd_decay_tolerances_at_regime_f_are_eight_times_the_floor():
    """SGD with weight decay at regime F's shape (tests/test_hip_rowopt_wide.py): TOL_F_SGD from the fp32 C oracle against
    parity.bprmf_sgd_f64(l2=...), and one missed decay step of one row exceeds it"""
    c, ref = op.sgd_f_reference()
    U, I, losses = _sgd_f_run()
    fig = parity.sgd_run_errors(c["U0"], c["I0"], ref, U, I)
    loss_err = parity.table_err(losses, ref[2])
    print("floor F SGD lr %g l2 %g: update/table %.1e update_err %.2e row_update_err %.2e table_err %.2e loss_err %.2e" % (
        op.F_SGD["lr"], op.F_SGD["l2"], fig["update_over_table"], fig["update_err"], fig["row_update_err"], fig["table_err"], loss_err))
    for name, key in (("update", "update_err"), ("row", "row_update_err")):
        assert math.isclose(op.TOL_F_SGD[name], _round_up_one_digit(8 * fig[key]), rel_tol=1e-9), (name, fig[key])
        assert 4 * fig[key] < op.TOL_F_SGD[name]
    assert 4 * fig["table_err"] < op.TOL_LOSS and 4 * loss_err < op.TOL_LOSS
    k, row = _victim(c["u"], c["B"], c["steps"], "replay_skip")
    U, I, _ = _sgd_f_run((k + 1, row))
    mut = parity.sgd_run_errors(c["U0"], c["I0"], ref, U, I)
    print("F SGD replay_skip: update_err %.2e row_update_err %.2e (tol %.0e)" % (mut["update_err"], mut["row_update_err"], op.TOL_F_SGD["row"]))
    assert mut["row_update_err"] > op.TOL_F_SGD["row"]


def test_eps_regime_is_the_eps_regime():
    """case A: the median |g| of a touched element is below 100 eps — eps is percent-level in sqrt(v) / sqrt(bc2) + eps"""
    c, ref = op.variant_reference(*op.VARIANTS["A"][0])
    assert op.median_abs_grad(ref) < 100 * 1e-8


# --------------------------------------------------------------------------------------------------- wrong steps
def _grads(U, I, u, p, n, skip=None):
    """dense BPR gradients in the tables' dtype (dot products and row sums carried in double and rounded once, as in
    wr_oracle.c).  skip = t: the positive-item occurrence of triplet t is left out of its row's sum."""
    dt = U.dtype
    ue, pe, ne = U[u], I[p], I[n]
    x = (ue * pe).sum(axis=1, dtype=np.float64).astype(dt) - (ue * ne).sum(axis=1, dtype=np.float64).astype(dt)
    s = dt.type(1) / (dt.type(1) + np.exp(-x))
    c = -(s * (dt.type(1) - s) / (dt.type(parity.GAMMA) + s)) / dt.type(u.size)
    cu = c[:, None] * ue
    pos = cu.copy()
    if skip is not None:
        pos[skip] = 0
    gU, gI = np.zeros_like(U), np.zeros_like(I)
    ru, gu = parity._row_sums(u, (c[:, None] * pe).astype(np.float64) - (c[:, None] * ne).astype(np.float64))
    ri, gi = parity._row_sums(np.concatenate([p, n]), np.concatenate([pos, -cu]).astype(np.float64))
    gU[ru], gI[ri] = gu.astype(dt), gi.astype(dt)
    return gU, gI


def _victim(u, B, nb, mutant):
    """(step, user row) of the mutants that hit one row.  replay_skip: the row is in batch `step` and not in the next one;
    decay_short_one_row: the same, and a later batch has the row again; state_skip: batch `step` is the row's second."""
    batches = [np.unique(u[k * B:(k + 1) * B]) for k in range(nb)]
    if mutant == "state_skip":
        seen = batches[0]
        for k in range(1, nb):
            again = np.intersect1d(batches[k], seen)
            if again.size:
                return k, int(again[0])
            seen = np.union1d(seen, batches[k])
    if mutant in ("replay_skip", "decay_short_one_row"):
        for k in range(nb - 1):
            cand = np.setdiff1d(batches[k], batches[k + 1])
            if mutant == "decay_short_one_row":
                cand = np.intersect1d(cand, np.concatenate(batches[k + 2:] + [np.zeros(0, u.dtype)]))
            if cand.size:
                return k, int(cand[0])
    assert mutant not in ("state_skip", "replay_skip", "decay_short_one_row"), "no such row in this run"
    return None


def _np_run(opt, U0, I0, u, p, n, B, lr, l2=0.0, mutant=None, dtype=F32):
    """the step of optim_parity.optim_f64 in NumPy `dtype`, with one wrong step built in (mutant)"""
    f = dtype
    W = [np.array(U0, dtype=f), np.array(I0, dtype=f)]
    S = {name: [np.zeros_like(W[0]), np.zeros_like(W[1])] for name in op.STATE_NAMES[opt]}
    lr, l2 = f(F32(lr)), f(F32(l2))
    b1, b2, omb1, omb2, eps = f(F32(0.9)), f(F32(0.999)), f(F32(1.0 - 0.9)), f(F32(1.0 - 0.999)), f(F32(1e-8))
    if mutant == "one_minus_beta_in_fp32":      # what wr_oracle.c and adam_elem do: 1.0f - 0.999f = 0.00099998713, not 0.001f
        omb1, omb2 = f(F32(1) - F32(0.9)), f(F32(1) - F32(0.999))
    rho = f(F32(0.9))
    nb = (u.size + B - 1) // B
    touched_before = [np.zeros(W[0].shape[0], bool), np.zeros(W[1].shape[0], bool)]
    victim = _victim(u, B, nb, mutant)
    occ_step = None
    if mutant == "missing_occurrence":
        # the first step in which an item row is shared and one of its occurrences is a positive item
        for k in range(nb):
            sl = slice(k * B, (k + 1) * B)
            rows, cnt = np.unique(np.concatenate([p[sl], n[sl]]), return_counts=True)
            shared = [r for r in rows[np.argsort(-cnt, kind="stable")][:8] if cnt[rows == r][0] >= 2 and (p[sl] == r).any()]
            if shared:
                occ_step, occ_row = k, shared[0]
                break
        assert occ_step is not None
    for k in range(nb):
        sl = slice(k * B, (k + 1) * B)
        skip = None
        if mutant == "missing_occurrence" and k == occ_step:  # the most-shared item row of that step loses one occurrence
            skip = int(np.flatnonzero(p[sl] == occ_row)[0])
        G = _grads(W[0], W[1], u[sl], p[sl], n[sl], skip)
        now = [np.zeros(W[0].shape[0], bool), np.zeros(W[1].shape[0], bool)]
        now[0][u[sl]] = True
        now[1][p[sl]] = True
        now[1][n[sl]] = True
        for side in (0, 1):
            w, g = W[side], G[side]
            keep = None
            if opt == "Adam":
                t = k + 1
                tb = {"bias_t_plus_1": t + 1, "bias_t_minus_1": max(t - 1, 1)}.get(mutant, t)
                bc1, bc2 = 1.0 - 0.9 ** tb, 1.0 - 0.999 ** tb
                m, v = S["m"][side], S["v"][side]
                if mutant == "replay_skip" and side == 0 and k == victim[0] + 1:
                    keep = [a[victim[1]].copy() for a in (w, m, v)]
                if l2 != 0 and mutant != "decoupled_decay":
                    g = g + l2 * w
                m += omb1 * (g - m)
                v *= b2
                v += omb2 * g * g
                if mutant == "eps_under_sqrt":
                    denom = np.sqrt(v / f(bc2) + eps)
                elif mutant == "eps_before_bc2":
                    denom = (np.sqrt(v) + eps) / f(math.sqrt(bc2))
                else:
                    denom = np.sqrt(v) / f(math.sqrt(bc2)) + eps
                if l2 != 0 and mutant == "decoupled_decay":
                    w *= f(1) - lr * l2
                w -= f(lr / bc1) * (m / denom)
                if keep is not None:
                    w[victim[1]], m[victim[1]], v[victim[1]] = keep
            elif opt == "Adagrad":
                s = S["state_sum"][side]
                g2 = g * g
                if mutant == "state_skip" and side == 0 and k == victim[0]:
                    g2[victim[1]] = 0                         # the row's step is taken, its state is not accumulated
                s += g2
                w -= lr * (g / (np.sqrt(s) + f(F32(1e-10))))
            else:
                sq, ac = S["square_avg"][side], S["acc_delta"][side]
                e6 = f(F32(1e-6))
                if mutant == "decay_short":                   # a row's first missed decay after each update is not replayed
                    short = touched_before[side] & ~now[side]
                    keep = (sq[short].copy(), ac[short].copy())
                if mutant == "decay_short_one_row" and side == 0 and k == victim[0] + 1:     # ... of one row, once
                    short = np.zeros(w.shape[0], bool)
                    short[victim[1]] = True
                    keep = (sq[short].copy(), ac[short].copy())
                sq *= rho
                sq += (f(1) - rho) * (g * g)
                delta = np.sqrt(ac + e6) / np.sqrt(sq + e6) * g
                ac *= rho
                ac += (f(1) - rho) * (delta * delta)
                w -= lr * delta
                if keep is not None:
                    sq[short], ac[short] = keep
        touched_before = now
    return W[0], W[1], {name: tuple(S[name]) for name in S}


def test_numpy_step_without_a_mutant_is_the_reference():
    """the step the mutants are built into, in float64 and unmutated, is optim_parity.optim_f64"""
    for variant in (op.VARIANTS["C_l2"][0], op.VARIANTS["E_adagrad"][0], op.VARIANTS["E_adadelta"][1]):
        c, ref = op.variant_reference(*variant)
        U, I, S = _np_run(ref["opt"], ref["U0"], ref["I0"], *ref["ids"], ref["batch"], ref["lr"], ref["l2"], dtype=np.float64)
        fig = op._errors(ref, U, I, S)
        assert fig["update_err"] < 1e-9 and fig["state_err"] < 1e-9, (variant, fig)


# regime -> the wrong steps its row_update_err tolerance must reject (the first variant of the regime)
SEES = {
    "A": ("eps_under_sqrt", "eps_before_bc2", "bias_t_plus_1", "bias_t_minus_1", "replay_skip", "missing_occurrence"),
    "B": ("eps_under_sqrt", "eps_before_bc2", "bias_t_plus_1", "bias_t_minus_1", "replay_skip", "missing_occurrence"),
    "B_l2": ("eps_under_sqrt", "eps_before_bc2", "bias_t_plus_1", "bias_t_minus_1", "missing_occurrence", "decoupled_decay"),
    "C": ("eps_under_sqrt", "eps_before_bc2", "bias_t_plus_1", "bias_t_minus_1", "replay_skip", "missing_occurrence"),
    "C_l2": ("eps_under_sqrt", "eps_before_bc2", "bias_t_plus_1", "bias_t_minus_1", "missing_occurrence", "decoupled_decay"),
    "D": ("eps_under_sqrt", "eps_before_bc2", "bias_t_plus_1", "bias_t_minus_1", "missing_occurrence"),
    "E_adagrad": ("state_skip", "missing_occurrence"),
    "E_adagrad_zipf": ("state_skip", "missing_occurrence"),
    "E_adadelta": ("decay_short", "decay_short_one_row", "missing_occurrence"),
    "E_gaps": ("decay_short", "missing_occurrence"),
    "F": ("eps_under_sqrt", "eps_before_bc2", "bias_t_plus_1", "bias_t_minus_1", "replay_skip", "missing_occurrence"),
    "F_l2": ("eps_under_sqrt", "eps_before_bc2", "bias_t_plus_1", "bias_t_minus_1", "missing_occurrence", "decoupled_decay"),
}


def _mutants_of(key):
    opt, l2 = op.VARIANTS[key][0][0], op.VARIANTS[key][0][4]
    if opt == "Adam":
        return ADAM_MUTANTS + (L2_MUTANTS if l2 else ())
    return ("state_skip", "missing_occurrence") if opt == "Adagrad" else ("decay_short", "decay_short_one_row", "missing_occurrence")


@pytest.mark.parametrize("key", list(op.VARIANTS))
def test_wrong_steps_are_rejected(key):
    variant = op.VARIANTS[key][-1 if key in ("B", "B_l2") else 0]      # B: the D = 20 run (a third of the arithmetic)
    c, ref = op.variant_reference(*variant)
    for mutant in _mutants_of(key):
        if mutant == "replay_skip" and ref["l2"] != 0:
            continue
        U, I, S = _np_run(ref["opt"], ref["U0"], ref["I0"], *ref["ids"], ref["batch"], ref["lr"], ref["l2"], mutant)
        f = op._errors(ref, U, I, S)
        print("%s %s: update_err %.2e row_update_err %.2e (tol %.0e) state_err %.2e (tol %.0e) table_err %.2e" % (
            key, mutant, f["update_err"], f["row_update_err"], op.TOL[key]["row"], f["state_err"], op.TOL[key]["state"],
            f["table_err"]))
        if mutant in SEES[key]:
            assert f["row_update_err"] > op.TOL[key]["row"], (key, mutant, f)


def test_every_wrong_step_is_rejected_somewhere():
    seen = set(m for ms in SEES.values() for m in ms)
    assert seen == set(ADAM_MUTANTS + L2_MUTANTS + ("state_skip", "decay_short", "decay_short_one_row"))


# --------------------------------------------------------------------------------------------------- the old bounds
# wrong steps that stay under the table bounds of the tests that existed before, at those tests' shapes and learning rates
OLD_BOUND_MISSES = {
    "g1": ("one_minus_beta_in_fp32",),
    "g1_l2": ("one_minus_beta_in_fp32",),
    "E_adagrad": (),
    "E_adadelta": ("decay_short_one_row",),
}


def _g1_run(tag, mutant):
    g1 = load_golden("g1_bprmf_step")
    lr, l2 = (float(x) for x in g1[tag + "_hp"])
    u, p, n = (np.concatenate([g1["%s%d" % (c, k)] for k in range(5)]).astype(np.int64) for c in "upn")
    return _np_run("Adam", g1["U0"], g1["I0"], u, p, n, 512, lr, l2, mutant)


@pytest.mark.parametrize("tag", ["adam", "adaml2"])
def test_what_the_golden_table_bound_saw_of_the_wrong_adam_steps(tag):
    """tests/test_hip_bprmf.py::test_adam_trajectory_matches_reference_golden: 97 x 131, D = 64, B = 512, 5 steps, rel_err on
    the table < 1e-5.  Every row is in every batch there, so no step is ever replayed, and at lr = 1e-2 on 97 x 131 tables
    the coarse wrong steps are all far above the bound (printed).  What that bound never covered is every regime of
    optim_parity but this one — other D, gradients near eps, gaps, steps past 50 — and the optimizer state: forming 1 - beta
    in fp32, as the oracle and the kernels do, stays under it (asserted) while v is off by 1.3e-5."""
    Uo, Io, _ = _g1_run(tag, None)
    key = "g1" if tag == "adam" else "g1_l2"
    for mutant in ADAM_MUTANTS + (L2_MUTANTS if tag == "adaml2" else ()) + ("one_minus_beta_in_fp32",):
        if mutant == "replay_skip":
            continue
        Um, Im, _ = _g1_run(tag, mutant)
        e = max(rel_err(Um, Uo), rel_err(Im, Io))
        print("old bound %s %s: rel_err %.2e (bound 1e-5)" % (tag, mutant, e))
        if mutant in OLD_BOUND_MISSES[key]:
            assert e < 1e-5, (mutant, e)


@pytest.mark.parametrize("key", ["E_adagrad", "E_adadelta"])
def test_what_the_dense_restatement_bound_saw_of_the_wrong_replays(key):
    """tests/test_hip_optimizers.py::test_sparse_fused_equals_dense_restatement, its D = 64 uniform run (the first variant of
    regime E: same sizes, seed and learning rate): rel_err on the table < 1e-4"""
    c, ref = op.variant_reference(*op.VARIANTS[key][0])
    args = (ref["opt"], ref["U0"], ref["I0"], *ref["ids"], ref["batch"], ref["lr"], 0.0)
    Uo, Io, _ = _np_run(*args)
    for mutant in _mutants_of(key):
        Um, Im, _ = _np_run(*args, mutant)
        eu, ei = rel_err(Um, Uo), rel_err(Im, Io)
        f = op._errors(ref, Um, Im, None)
        print("old bound %s %s: rel_err users %.2e items %.2e (bound 1e-4); update_err %.2e row_update_err %.2e" % (
            key, mutant, eu, ei, f["update_err"], f["row_update_err"]))
        if mutant in OLD_BOUND_MISSES[key]:
            assert max(eu, ei) < 1e-4, (mutant, eu, ei)


def test_one_minus_beta_formed_in_fp32_is_the_adam_state_floor():
    """the Adam state floor of 1.3e-5 in every regime is not rounding: NumPy fp32 with torch's scalars (0.001f) is at 1e-6
    or below, the same step with 1.0f - 0.999f is where the fp32 oracle is"""
    c, ref = op.variant_reference(*op.VARIANTS["C"][0])
    args = (ref["opt"], ref["U0"], ref["I0"], *ref["ids"], ref["batch"], ref["lr"], 0.0)
    clean = op._errors(ref, *_np_run(*args))["state_err"]
    project = op._errors(ref, *_np_run(*args, "one_minus_beta_in_fp32"))["state_err"]
    print("state_err: torch's scalars %.2e, 1 - beta in fp32 %.2e, fp32 oracle %.2e" % (
        clean, project, _floor(op.VARIANTS["C"][0])["state_err"]))
    assert clean < 1e-6 and 1e-5 < project < 2e-5
