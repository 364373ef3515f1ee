"""NumPy restatement of "dense torch.optim.Adam / SGD on ONE table, then BUIR's momentum update of its target" — the reference of
the row-lazy pair tests (tests/test_buir_lazy_contract.py, tests/test_hip_buir_lazy.py; include/whisprrec_hip.h K24).  A helper,
not a test.

``dense_loop`` is tests/rowopt_ref.py's ``dense_loop`` plus the target: per step the gradient table from (idx, src), the optimizer
over the whole table, then ``T = T*mom + W*(1 - mom)`` (reference src/models/general/BUIR.py:71) — ``mom`` rounded to fp32 and
``1 - mom`` formed in double and then rounded, as ``hip_ops.ema_update_`` hands them to the kernel.  ``dtype=np.float64`` is the
reference, ``dtype=np.float32`` the same loop with every operation rounded to fp32 (the floors of the tolerances).  ``T0 = W0``.
Inputs: ``rowopt_ref.make_case(n_rows, D, -1, seed)`` — BUIR has no padding row.  ``mutant`` builds one wrong step into the loop.
"""
import math

import numpy as np

import rowopt_ref as R

F32 = np.float32
# (n_rows, D, l2, momentum): both table sizes with every D, both l2 and both momenta with each table size
CASES = ((1000, 64, 0.0, 0.995), (1000, 20, 1e-3, 0.9), (1000, 128, 1e-3, 0.995),
         (20000, 64, 1e-3, 0.9), (20000, 128, 0.0, 0.995), (20000, 20, 0.0, 0.9))
LR = R.LR
MUTANTS = ("ema_skip", "ema_before_step", "ema_stale", "sweep_unreplayed", "replay_skip", "run_short")
SKIP_ROW = R.GAP_ROW0 + 1                       # used at steps 1 and 3: step 2 is the one it misses
SKIP_STEP = R.GAP_USES[1][0] + 1
STALE_ROW = R.GAP_ROW0 + 7                      # used at steps 1 and 9: a replay of 7 steps
BEFORE_STEP = R.HOT_STEPS[0]                    # "ema_before_step": every row touched at this step


def make_case(n_rows, D, seed=0):
    return R.make_case(n_rows, D, -1, seed)


# the wide and run-length cases of rowopt_ref (four rows per wave, the stride loop, run lengths): (n_rows, D, l2, momentum)
WIDE_CASES = ((R.WIDE_ROWS, 64, 1e-3, 0.9), (R.WIDE_ROWS, 20, 0.0, 0.995))
RUN_CASES = ((R.RUN_ROWS, 20, 1e-3, 0.9), (R.RUN_ROWS, 64, 0.0, 0.995), (R.RUN_ROWS, 100, 0.0, 0.9), (R.RUN_ROWS, 128, 1e-3, 0.995))
WIDE_MUTANTS = R.WIDE_MUTANTS


def make_wide_case(n_rows, D, seed=0):
    return R.make_wide_case(n_rows, D, -1, seed)


def make_any_case(case, seed=0):
    """make_case / make_wide_case / rowopt_ref.make_run_case by the case tuple"""
    n_rows, D = case[:2]
    if case in RUN_CASES:
        return R.make_run_case(n_rows, D, -1, seed)
    return (make_wide_case if n_rows == R.WIDE_ROWS else make_case)(n_rows, D, seed)


def _f(x):
    return float(F32(x))


def dense_loop(opt, W0, steps, lr, l2, mom, dtype=np.float64, betas=(0.9, 0.999), eps=1e-8, mutant=None):
    """-> (W, T, {"m": m, "v": v}) (Adam) or (W, T, {}) (SGD) after the steps, in `dtype`.  mutant (one wrong step each):
    "ema_skip"         the target update of step SKIP_STEP does not happen for row SKIP_ROW (a missed step's update);
    "ema_before_step"  at step BEFORE_STEP the target update of every touched row uses w from before the optimizer step;
    "ema_stale"        row STALE_ROW's replayed target updates (the steps between its two uses) all move toward the w the row
                       has at the end of the replay instead of the w of each step;
    "sweep_unreplayed" the window sweep (max_lag = SWEEP_LAG) marks rows current without replaying them: the optimizer step AND
                       the target update of the lost (step, row) pairs do not happen;
    "replay_skip"      K22's: one zero-gradient optimizer step of row SKIP_ROW does not happen (its target update does);
    "run_short"        K22's: the last position of the hot row's run is left out of its sum;
    "fourth_row", "stride_tail", "window_offset"  the replay mutants of the wide cases (rowopt_ref.lost_of): the optimizer step
                       AND the target update of the lost (step, row) pairs do not happen;
    "run_trip"         K22's: a run whose length is a multiple of 64 loses its last 64 positions."""
    f = dtype
    W = np.array(W0, dtype=f)
    T = np.array(W0, dtype=f)
    n_rows = W.shape[0]
    lr, l2 = f(_f(lr)), f(_f(l2))
    b2, eps = f(_f(betas[1])), f(_f(eps))
    if f is np.float32:
        omb1, omb2 = F32(1) - F32(betas[0]), F32(1) - F32(betas[1])
    else:
        omb1, omb2 = f(_f(1.0 - betas[0])), f(_f(1.0 - betas[1]))
    mo, omm = f(_f(mom)), f(_f(1.0 - float(mom)))
    m, v = np.zeros_like(W), np.zeros_like(W)
    lost = {}
    if mutant == "replay_skip":
        lost = {SKIP_STEP: np.asarray([SKIP_ROW])}
    elif mutant == "sweep_unreplayed":
        lost = R.lost_by_unreplayed_sweep(steps, n_rows)
    elif mutant in R.WIDE_MUTANTS:
        lost = R.lost_of(mutant, steps, n_rows)
    stale_from, stale_to = R.GAP_USES[7]
    stale_T = None
    for t, (idx, src) in enumerate(steps, start=1):
        G = R.grad_table(idx, src, n_rows, -1, f, drop_last_of=R.HOT_ROW if (mutant == "run_short" and t == R.HOT_STEPS[0]) else None,
                         drop_trip=mutant == "run_trip")
        rows = lost.get(t)
        keep = None if rows is None else [a[rows].copy() for a in (W, m, v, T)]
        W_before = W.copy() if (mutant == "ema_before_step" and t == BEFORE_STEP) else None
        if l2 != 0:
            G += l2 * W
        if opt == "Adam":
            bc1, bc2 = 1.0 - betas[0] ** t, 1.0 - betas[1] ** t
            m += omb1 * (G - m)
            v *= b2
            v += omb2 * G * G
            W -= f(_f(lr) / bc1) * (m / (np.sqrt(v) / f(math.sqrt(bc2)) + eps))
        else:
            W -= lr * G
        if keep is not None and mutant == "replay_skip":
            W[rows], m[rows], v[rows] = keep[:3]                          # the optimizer step is lost, the update happens
        W_for_T = W
        if W_before is not None:
            touched = np.unique(idx)
            W_for_T = W.copy()
            W_for_T[touched] = W_before[touched]
        T_new = T * mo + W_for_T * omm
        if mutant == "ema_skip" and t == SKIP_STEP:
            T_new[SKIP_ROW] = T[SKIP_ROW]
        T = T_new
        if keep is not None and mutant != "replay_skip":
            W[rows], m[rows], v[rows], T[rows] = keep
        if mutant == "ema_stale":
            if t == stale_from:
                stale_T = T[STALE_ROW].copy()                             # the target after the row's first use
            elif t == stale_to - 1:
                x = stale_T                                               # the replay, all toward the row's w of step stale_to - 1
                for _ in range(stale_from + 1, stale_to):
                    x = x * mo + W[STALE_ROW] * omm
                T[STALE_ROW] = x
    return W, T, ({"m": m, "v": v} if opt == "Adam" else {})
