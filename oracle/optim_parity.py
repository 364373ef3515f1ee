"""Float64 references of the stateful optimizer steps (Adam, Adagrad, Adadelta on the two BPRMF tables) and the
update-normalised parity check for them — TEST INFRASTRUCTURE ONLY, as oracle/parity.py (``whisprrec_amd`` never imports it).

Why.  The Adam kernels were pinned to the reference only through ``conftest.rel_err`` on the TABLE (1e-5 / 1e-4, three runs
at D = 64), and the lazy forms only bitwise to the project's own dense kernel.  A table bound does not see a wrong update:
tests/test_optim_power.py lists wrong steps (eps under the square root, bias correction of the neighbouring step, a missed
replay step, Adadelta replayed one decay short) that pass the old bounds.  ``check_optim_run`` measures the error against the
UPDATE (parity.update_err / row_update_err) and against the optimizer STATE, with a float64 reference.

The references restate the reference loop's step (src/helpers/BaseRunner.py:194-200) with torch.optim's single-tensor
formulas, dense semantics (every row, every step), in NumPy float64:
    Adam      g += l2 * w (coupled weight decay); m.lerp_(g, 1 - beta1); v = beta2 * v + (1 - beta2) * g * g;
              denom = sqrt(v) / sqrt(bc2) + eps; w -= (lr / bc1) * m / denom; bc1, bc2 = 1 - beta ** t in double.
    Adagrad   as oracle.adagrad_dense;  Adadelta  as oracle.adadelta_dense (one state decay per step for every row).
Scalars are what an fp32 implementation sees: lr, l2, eps, the betas and rho rounded to fp32 once; for Adam 1 - beta is
rounded from the double difference (torch hands `1 - beta2`, a Python float, to an fp32 kernel: 0.001f), for Adagrad /
Adadelta it is the oracle's own expression.  The fp32 oracle and the kernels form 1.0f - beta2f = 0.00099998713 instead
(1.3e-5 below 0.001f): v is that much smaller and an update outside the eps regime 6e-6 larger.  That is a deviation from
torch, not a rounding; it is part of the floors below (about half of regime C's) and is recorded in DESIGN.md.

Compact tables.  With l2 = 0 a row no batch touches has zero state and never moves, so the reference may run on tables of the
touched rows (``reference(compact=True)``, as parity.check_sgd_run(rows=...)).  With l2 > 0 every row moves: the reference
then runs on the whole tables, and ``reference`` asserts that.

Regimes (``case``; shapes, seeds and scales shared by tests/test_optim_power.py and tests/test_hip_optim_parity.py):
    A  eps regime      70K x 200K, B = 8,192, 5 steps (short last batch), tables N(0, 0.01^2), lr 1e-3: the median |g| of a
                       touched element is < 100 eps, so eps is percent-level in the denominator; D = 64, 128
    B  long gaps       10K x 8K, B = 64, 160 steps: a row misses ~150 steps between two uses; D = 64, 20; l2 = 0 / 1e-3
    C  hot rows        3K x 2.5K, B = 256, 24 steps, Zipf items and one hot user; D = 32; l2 = 0 / 1e-3
    D  saturated       3K x 2.5K, B = 256, 12 steps, D = 64, tables N(0, 0.7^2) as of a trained model: score differences
                       reach +-19, gradient elements span 1e-2 .. 2e-11 and v goes down to 4e-29
    F  four rows per wave  70,001 x 140,003, B = 32,768, 4 steps (short last batch), uniform ids, tables N(0, 0.01^2) as A, lr 1e-3:
                       32,768 user keys and 65,536 item keys per batch and tables of 70,001 / 140,003 rows are at or above the
                       size (32,768) from which wr_lazy.hip's kernels hold four rows per wave; 140,003 rows are more than
                       one stride (131,072) of its catch-up; windows of max_lag = 2 have 35,001 and 70,002 rows; D = 64 with
                       l2 = 0 and D = 20 with l2 = 1e-3 (tests/test_hip_rowopt_wide.py)
    E  Adagrad / Adadelta  1.5K x 1.2K, B = 128, 14 steps (short last batch), uniform and Zipf, D = 64, 20; and Adadelta at
                       regime B's shape (E_gaps)

Tolerances are derived, not chosen (tests/test_optim_power.py asserts the derivation): per regime, the fp32 oracle
(oracle.bpr_dense_grads + oracle.adam_dense / adagrad_dense / adadelta_dense — the reference against itself in lower
precision, never the code under test) runs against the float64 reference; TOL = 8 x the largest floor of the regime,
rounded up to one significant digit (8 x: as oracle/parity.py — another summation order, fused multiply-adds, hardware exp,
rcp and sqrt are each worth a small multiple of one rounding).  state_err = max|state - state64| / max|state64|, the
largest over the state tables.

Measured floors (largest over the regime's variants):

    regime                                   update/table  update_err  row_update_err  state_err  table_err
    A                                        9.2e-2        1.23e-5     1.99e-5         1.29e-5    1.06e-6
    B     (l2 = 0)                           9.4e-2        7.10e-4     1.60e-3         2.52e-5    5.92e-5
    B_l2  (l2 = 1e-3)                        4.8e-1        2.28e-6     2.35e-6         1.35e-5    1.04e-6
    C     (l2 = 0)                           5.4e-2        2.33e-5     1.09e-4         1.33e-5    1.18e-6
    C_l2  (l2 = 1e-3)                        6.0e-2        6.47e-6     6.53e-6         1.32e-5    3.55e-7
    D                                        2.8e-3        7.67e-3     1.97e-2         1.50e-5    2.17e-5
    E_adagrad       (uniform ids)            2.0e-1        2.15e-6     4.26e-6         2.83e-7    3.38e-7
    E_adagrad_zipf  (hot rows)               2.7e-1        3.52e-4     9.43e-4         2.84e-7    6.93e-5
    E_adadelta      (uniform and Zipf)       6.1e-2        9.97e-6     2.59e-5         3.44e-7    1.69e-7
    E_gaps          (Adadelta, B's shape)    2.9e-2        5.62e-6     1.15e-5         3.85e-7    1.30e-7
    F     (l2 = 0, D = 64)                   7.6e-2        4.02e-6     6.10e-6         1.30e-5    3.04e-7
    F_l2  (l2 = 1e-3, D = 20)                8.4e-2        2.05e-5     2.06e-5         1.30e-5    1.69e-6
    F, SGD lr 1 with weight decay 1e-2 (TOL_F_SGD; fp32 C oracle against parity.bprmf_sgd_f64(l2=1e-2))
                                             4.1e-2        3.25e-6     5.02e-6         -          1.33e-7

The floors are not all roundings of a well-conditioned sum.  B and D (l2 = 0): a gradient element that is small by
cancellation (p_d - n_d ~ 1e-5 of its terms) carries a relative fp32 error of 1e-3, and where sqrt(v) / sqrt(bc2) is within a
factor of eps the update follows that error — one element in 1e4 (B), most of the rows with saturated scores (D, where
1 - sigmoid(x) has two digits left).  With l2 > 0 the decay term swamps such elements and the floor is 2e-6.  The Adam state
floor of 1.3e-5 is the (1 - beta2) deviation above, not a rounding (the Adagrad / Adadelta state floors are 3e-7).  The
loss floors are 4e-8 .. 3e-7 in every regime.

The table bound.  table_err = update_err x update/table, so where the fp32 oracle itself is above 1e-5 / 4 on the table (B,
D, E_adagrad_zipf) the bound on the table is the derived one, 8 x that floor; everywhere else it stays at 1e-5
(TOL[...]["table"] = max(1e-5, derived)).  The bound on the losses is 1e-5 in every regime.
"""
import functools

import numpy as np

from . import parity

F32 = np.float32

TOL = {
    "A": {"update": 1e-04, "row": 2e-04, "state": 2e-04, "table": 1e-05},
    "B": {"update": 6e-03, "row": 2e-02, "state": 3e-04, "table": 5e-04},
    "B_l2": {"update": 2e-05, "row": 2e-05, "state": 2e-04, "table": 1e-05},
    "C": {"update": 2e-04, "row": 9e-04, "state": 2e-04, "table": 1e-05},
    "C_l2": {"update": 6e-05, "row": 6e-05, "state": 2e-04, "table": 1e-05},
    "D": {"update": 7e-02, "row": 2e-01, "state": 2e-04, "table": 2e-04},
    "E_adagrad": {"update": 2e-05, "row": 4e-05, "state": 3e-06, "table": 1e-05},
    "E_adagrad_zipf": {"update": 3e-03, "row": 8e-03, "state": 3e-06, "table": 6e-04},
    "E_adadelta": {"update": 8e-05, "row": 3e-04, "state": 3e-06, "table": 1e-05},
    "E_gaps": {"update": 5e-05, "row": 1e-04, "state": 4e-06, "table": 1e-05},
    "F": {"update": 4e-05, "row": 5e-05, "state": 2e-04, "table": 1e-05},
    "F_l2": {"update": 2e-04, "row": 2e-04, "state": 2e-04, "table": 2e-05},
}
TOL_LOSS = parity.TOL_TABLE                 # the bound on the losses, and the least bound on the table: unchanged

# SGD with weight decay at regime F's shape (D = 64): hip_ops.LazyOptimizerState("SGD", lr, l2) against
# parity.bprmf_sgd_f64(l2=...).  The decay moves every row by lr * l2 = 1e-2 of itself per step; a row's gradient step is
# 0.5 * lr / B = 1.5e-5 of the table per occurrence — 1.5e-3 of the decay, and 60 times the tolerance on the row's update.
F_SGD = {"lr": 1.0, "l2": 1e-2}
TOL_F_SGD = {"update": 3e-5, "row": 5e-5}    # 8 x the floor of the fp32 C oracle (tests/test_optim_power.py)


def _f(x):
    return float(F32(x))


# --------------------------------------------------------------------------------------------------- regimes
def _ids(rng, nU, nI, N, zipf, hot_every):
    u = rng.randint(0, nU, N)
    p = np.minimum((rng.pareto(1.0, N) * 3).astype(np.int64), nI - 1) if zipf else rng.randint(0, nI, N)
    n = rng.randint(1, nI, N)
    if zipf:
        u[::hot_every] = 7                   # a hot user too: pieces + combine on that side
    return u, p, n


@functools.lru_cache(maxsize=None)
def case(regime, D=64, zipf=False):
    """the data of one run: dict(U0, I0 fp32 whole tables; u, p, n int64; B, steps, lr, nU, nI).  Do not modify it."""
    if regime == "A":
        nU, nI, B, steps, lr = 70_000, 200_000, 8192, 5, 1e-3
        rng = np.random.RandomState(100 + D)
        u, p, n = _ids(rng, nU, nI, steps * B - B // 3, False, 0)
        scale = 0.01
    elif regime == "B":
        nU, nI, B, steps, lr = 10_000, 8_000, 64, 160, 1e-3
        rng = np.random.RandomState(200 + D)
        u, p, n = _ids(rng, nU, nI, steps * B - 20, False, 0)
        scale = 0.1
    elif regime == "C":
        nU, nI, B, steps, lr = 3_000, 2_500, 256, 24, 1e-3
        rng = np.random.RandomState(300 + D)
        u, p, n = _ids(rng, nU, nI, steps * B, True, 5)
        scale = 0.1
    elif regime == "D":
        nU, nI, B, steps, lr = 3_000, 2_500, 256, 12, 1e-3
        rng = np.random.RandomState(400 + D)
        u, p, n = _ids(rng, nU, nI, steps * B, False, 0)
        scale = 0.7                          # score differences x ~ N(0, 5.5^2): |x| reaches about 20
    elif regime == "F":
        nU, nI, B, steps, lr = 70_001, 140_003, 32768, 4, 1e-3
        rng = np.random.RandomState(600 + D)
        u, p, n = _ids(rng, nU, nI, steps * B - B // 3, False, 0)
        scale = 0.01
    elif regime == "E":                      # tests/test_hip_optimizers.py::test_sparse_fused_equals_dense_restatement
        nU, nI, B, steps, lr = 1_500, 1_200, 128, 14, None      # lr: by optimizer (E_LR)
        rng = np.random.RandomState(5 + D)
        scale = 0.3
    else:
        raise ValueError(regime)
    U0 = (rng.standard_normal((nU, D)) * scale).astype(F32)
    I0 = (rng.standard_normal((nI, D)) * scale).astype(F32)
    if regime == "E":
        u, p, n = _ids(rng, nU, nI, steps * B - 40, zipf, 3)
    for a in (U0, I0, u, p, n):
        a.setflags(write=False)
    return {"U0": U0, "I0": I0, "u": u, "p": p, "n": n, "B": B, "steps": steps, "lr": lr, "nU": nU, "nI": nI}


E_LR = {"Adagrad": 0.05, "Adadelta": 1.5}

# tolerance key -> the runs it covers: (optimizer, case regime, D, zipf, l2)
VARIANTS = {
    "A": [("Adam", "A", 64, False, 0.0), ("Adam", "A", 128, False, 0.0)],
    "B": [("Adam", "B", 64, False, 0.0), ("Adam", "B", 20, False, 0.0)],
    "B_l2": [("Adam", "B", 64, False, 1e-3), ("Adam", "B", 20, False, 1e-3)],
    "C": [("Adam", "C", 32, True, 0.0)],
    "C_l2": [("Adam", "C", 32, True, 1e-3)],
    "D": [("Adam", "D", 64, False, 0.0)],
    "E_adagrad": [("Adagrad", "E", D, False, 0.0) for D in (64, 20)],
    "E_adagrad_zipf": [("Adagrad", "E", D, True, 0.0) for D in (64, 20)],
    "E_adadelta": [("Adadelta", "E", D, zipf, 0.0) for D in (64, 20) for zipf in (False, True)],
    "E_gaps": [("Adadelta", "B", 64, False, 0.0)],
    "F": [("Adam", "F", 64, False, 0.0)],
    "F_l2": [("Adam", "F", 20, False, 1e-3)],
}


@functools.lru_cache(maxsize=None)
def variant_reference(opt, regime, D, zipf, l2):
    """(case data, float64 reference) of one entry of VARIANTS, computed once per process and shared: do not modify"""
    c = case(regime, D, zipf)
    lr = c["lr"] if opt == "Adam" else E_LR[opt]
    return c, reference(opt, c["U0"], c["I0"], c["u"], c["p"], c["n"], c["B"], lr, l2, compact=l2 == 0.0)


@functools.lru_cache(maxsize=None)
def sgd_f_reference():
    """(case data of regime F at D = 64, (U64, I64, losses) of SGD with F_SGD's weight decay on the whole tables): shared, do
    not modify"""
    c = case("F", 64)
    return c, parity.bprmf_sgd_f64(c["U0"], c["I0"], c["u"], c["p"], c["n"], c["B"], F_SGD["lr"], l2=F_SGD["l2"])


# --------------------------------------------------------------------------------------------------- float64 steps
STATE_NAMES = {"Adam": ("m", "v"), "Adagrad": ("state_sum",), "Adadelta": ("square_avg", "acc_delta")}


def optim_f64(opt, U, I, u, p, n, batch, lr, l2=0.0, n_steps=None, betas=(0.9, 0.999), eps=None, rho=0.9):
    """The reference loop with torch.optim.<opt> on the tables U, I (the tables the ids index), dense semantics, in float64.
    A short last batch is allowed.  Returns {"U", "I", "state": {name: (user table, item table)}, "losses"}."""
    W = [np.array(U, dtype=np.float64), np.array(I, dtype=np.float64)]
    u, p, n = (np.asarray(a, dtype=np.int64) for a in (u, p, n))
    batch = int(batch)
    nb = (u.size + batch - 1) // batch if n_steps is None else int(n_steps)
    lr, l2 = _f(lr), _f(l2)
    assert opt == "Adam" or l2 == 0.0, "the fused Adagrad / Adadelta steps have no weight decay"
    S = {name: [np.zeros_like(W[0]), np.zeros_like(W[1])] for name in STATE_NAMES[opt]}
    if opt == "Adam":
        eps = _f(1e-8 if eps is None else eps)
        b1, b2, omb1, omb2 = _f(betas[0]), _f(betas[1]), _f(1.0 - betas[0]), _f(1.0 - betas[1])
    elif opt == "Adagrad":
        eps = _f(1e-10 if eps is None else eps)
    else:
        eps, rho = _f(1e-6 if eps is None else eps), _f(rho)
    losses = np.zeros(nb, np.float64)
    G = [np.zeros_like(W[0]), np.zeros_like(W[1])]
    for k in range(nb):
        sl = slice(k * batch, (k + 1) * batch)
        ru, gu, ri, gi, losses[k] = parity.bpr_row_grads_f64(W[0], W[1], u[sl], p[sl], n[sl])
        for side, (rows, g) in enumerate(((ru, gu), (ri, gi))):
            w, gd = W[side], G[side]
            gd[:] = 0.0
            gd[rows] = g
            if opt == "Adam":
                t = k + 1
                bc1, bc2 = 1.0 - betas[0] ** t, 1.0 - betas[1] ** t
                m, v = S["m"][side], S["v"][side]
                if l2 != 0.0:
                    gd += l2 * w
                m += omb1 * (gd - m)
                v *= b2
                v += omb2 * gd * gd
                w -= (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
            elif opt == "Adagrad":
                s = S["state_sum"][side]
                s += gd * gd
                w -= lr * (gd / (np.sqrt(s) + eps))
            else:
                sq, ac = S["square_avg"][side], S["acc_delta"][side]
                sq *= rho
                sq += (1.0 - rho) * (gd * gd)
                delta = np.sqrt(ac + eps) / np.sqrt(sq + eps) * gd
                ac *= rho
                ac += (1.0 - rho) * (delta * delta)
                w -= lr * delta
    return {"U": W[0], "I": W[1], "state": {name: tuple(S[name]) for name in S}, "losses": losses}


def reference(opt, U0, I0, u, p, n, batch, lr, l2=0.0, compact=True, **hyper):
    """The float64 run of one case, to be shared by every check against it: optim_f64's result plus what check_optim_run
    needs (the tables before the run, the rows compared, the ids on those rows).  compact: run on the tables of the touched
    rows — valid only without weight decay."""
    assert not (compact and float(l2) != 0.0), "with weight decay every row moves: the reference needs the whole tables"
    u, p, n = (np.asarray(a, dtype=np.int64) for a in (u, p, n))
    rows = parity.touched_rows(u, p, n) if compact else None
    if compact:
        U0, I0 = np.asarray(U0)[rows[0]], np.asarray(I0)[rows[1]]
        u, p, n = np.searchsorted(rows[0], u), np.searchsorted(rows[1], p), np.searchsorted(rows[1], n)
    ref = optim_f64(opt, U0, I0, u, p, n, batch, lr, l2, **hyper)
    ref.update(opt=opt, U0=np.asarray(U0), I0=np.asarray(I0), rows=rows, ids=(u, p, n), batch=int(batch), lr=float(lr), l2=float(l2))
    return ref


def median_abs_grad(ref):
    """median |g| over the elements of the rows the first batch touches, in the float64 reference"""
    u, p, n = (a[:ref["batch"]] for a in ref["ids"])
    _, gu, _, gi, _ = parity.bpr_row_grads_f64(ref["U0"].astype(np.float64), ref["I0"].astype(np.float64), u, p, n)
    return float(np.median(np.abs(np.concatenate([gu.ravel(), gi.ravel()]))))


def _cut(ref, U, I):
    if ref["rows"] is None:
        return (np.asarray(U.cpu() if hasattr(U, "cpu") else U), np.asarray(I.cpu() if hasattr(I, "cpu") else I))
    return parity.take_rows(U, ref["rows"][0]), parity.take_rows(I, ref["rows"][1])


def optim_run_errors(ref, got_U, got_I, state=None):
    """the figures of one run (whole tables, NumPy or torch) against its float64 reference: a dict.  state: {name: (user
    table, item table)} in the dense optimizer's terms, names as STATE_NAMES[opt]."""
    got_U, got_I = _cut(ref, got_U, got_I)
    return _errors(ref, got_U, got_I, None if state is None else {k: _cut(ref, *v) for k, v in state.items()})


def _errors(ref, got_U, got_I, state):
    """optim_run_errors on tables already restricted to the reference's rows"""
    assert got_U.shape == ref["U0"].shape and got_I.shape == ref["I0"].shape
    fig = parity.sgd_run_errors(ref["U0"], ref["I0"], (ref["U"], ref["I"]), got_U, got_I)
    if state is not None:
        assert set(state) == set(ref["state"]), (sorted(state), sorted(ref["state"]))
        fig["state_err"] = max(parity.table_err(g, r) for name in state for g, r in zip(state[name], ref["state"][name]))
    return fig


def _np64(t):
    return np.asarray(t.cpu() if hasattr(t, "cpu") else t, dtype=np.float64)


def state_of(st):
    """the optimizer state of a hip_ops.LazyOptimizerState (Adam, after flush()) or StatefulSparseState in the dense
    optimizer's terms, as check_optim_run takes it.  Adadelta keeps a row's two state rows as of the row's last update
    (``last``) and owes them one decay by rho per step since: applied here, in float64."""
    if hasattr(st, "m_u"):
        assert st.flushed_at == st.t, "flush() first: rows are behind"
        return {"m": (st.m_u, st.m_i), "v": (st.v_u, st.v_i)}
    if st.name == "Adagrad":
        return {"state_sum": (st.s1_u, st.s1_i)}
    owed = [_f(st.rho) ** (st.t - _np64(last))[:, None] for last in (st.last_u, st.last_i)]
    return {"square_avg": (_np64(st.s1_u) * owed[0], _np64(st.s1_i) * owed[1]),
            "acc_delta": (_np64(st.s2_u) * owed[0], _np64(st.s2_i) * owed[1])}


def check_optim_run(tag, ref, got_U, got_I, got_losses, tol, state=None):
    """One run against its float64 reference (``reference``), with the assertions every optimizer parity test makes:
    update_err < tol["update"], row_update_err < tol["row"], table_err < tol["table"], losses within 1e-5 of the float64 losses and,
    where the optimizer state is given, state_err < tol["state"].  got_U, got_I and the state tables: whole tables after the
    run (NumPy arrays or torch tensors).  Prints the figures once (pytest -s / -rP); a failure names the worst row (global id,
    user or item) and its occurrences per step.  Returns the figures."""
    fig = optim_run_errors(ref, got_U, got_I, state)
    if hasattr(got_losses, "cpu"):
        got_losses = got_losses.cpu().numpy()
    fig["loss_err"] = parity.table_err(np.asarray(got_losses, dtype=np.float64).reshape(-1), ref["losses"])
    state_txt = " state_err %.2e (tol %.0e)" % (fig["state_err"], tol["state"]) if state is not None else ""
    print("parity %s: %s lr %.4g l2 %g update/table %.1e | update_err %.2e (tol %.0e) row_update_err %.2e (tol %.0e) table_err "
          "%.2e (tol %.0e) loss_err %.2e (tol %.0e)%s" % (
              tag, ref["opt"], ref["lr"], ref["l2"], fig["update_over_table"], fig["update_err"], tol["update"],
              fig["row_update_err"], tol["row"], fig["table_err"], tol["table"], fig["loss_err"], TOL_LOSS, state_txt), flush=True)
    ok = (fig["update_err"] < tol["update"] and fig["row_update_err"] < tol["row"] and fig["table_err"] < tol["table"]
          and fig["loss_err"] < TOL_LOSS and (state is None or fig["state_err"] < tol["state"]))
    if not ok:
        kind, row = fig["worst"]
        cu, cp, cn = ref["ids"]
        B, nb = ref["batch"], ref["losses"].size
        cols = (cu,) if kind == "user" else (cp, cn)
        occ = [sum(int(np.sum(c[k * B:(k + 1) * B] == row)) for c in cols) for k in range(nb)]
        rows = ref["rows"]
        gid = row if rows is None else int(rows[0 if kind == "user" else 1][row])
        raise AssertionError("%s: %s; worst row: %s %d, occurrences per step %s" % (
            tag, {k: v for k, v in fig.items() if k != "worst"}, kind, gid, occ))
    return fig
