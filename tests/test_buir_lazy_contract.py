"""CPU checks for BUIR's row-lazy online / target tables (--emb_lazy 1 on BUIR; include/whisprrec_hip.h K24): the flag, the
tolerances of the float64 parity check of tests/test_hip_buir_lazy.py against the fp32 floor, and the wrong steps against those
tolerances.  No GPU.

Floor: tests/buir_lazy_ref.py's dense loop (optimizer over the whole table, then T = T*mom + W*(1 - mom)) in fp32 against the same
loop in float64 — the reference against itself in lower precision, never the code under test — on every case of
buir_lazy_ref.CASES, the cases of the GPU tests.  Measures: update_err / row_update_err of the online table (oracle/parity.py), the
same two of the target relative to T - T0 ("t_update", "t_row"), and state_err of the Adam moments.  TOL = 8 x the largest floor,
rounded up to one significant digit (tests/test_emb_lazy_contract.py's docstring has the argument for 8 x), and every floor
leaves a factor 4.

Measured floors (12 steps, tables ~ N(0, 0.1^2), gradient rows ~ N(0, 0.01^2); Adam lr 1e-3, SGD lr 0.5):

    Adam (n_rows, D, l2, momentum)     update/table (target)  update_err  row_update_err  t_update_err  t_row_update_err  state_err
    (1000, 64, 0.0, 0.995)             2.4e-02  (8.4e-04 )    1.29e-05    1.52e-05        4.79e-04      6.06e-04          1.31e-05
    (1000, 20, 0.001, 0.9)             3.1e-02  (1.4e-02 )    1.16e-05    1.57e-05        1.77e-05      2.41e-05          1.26e-05
    (1000, 128, 0.001, 0.995)          2.5e-02  (8.0e-04 )    3.00e-05    4.23e-05        4.03e-04      5.26e-04          1.34e-05
    (20000, 64, 0.001, 0.9)            2.6e-02  (1.2e-02 )    1.76e-05    1.79e-05        2.70e-05      2.75e-05          1.29e-05
    (20000, 128, 0.0, 0.995)           1.7e-02  (6.2e-04 )    1.64e-05    2.73e-05        1.09e-03      1.54e-02          1.32e-05
    (20000, 20, 0.0, 0.9)              1.8e-02  (9.2e-03 )    1.44e-05    2.66e-05        2.65e-05      2.13e-04          1.23e-05
    SGD  (n_rows, D, l2, momentum)     update/table (target)  update_err  row_update_err  t_update_err  t_row_update_err  state_err
    (1000, 64, 0.0, 0.995)             4.7e-01  (2.6e-02 )    4.56e-07    1.05e-06        1.96e-05      8.86e-05          -
    (1000, 20, 0.001, 0.9)             5.9e-01  (3.9e-01 )    4.55e-07    1.86e-06        5.58e-07      3.27e-06          -
    (1000, 128, 0.001, 0.995)          7.4e-01  (3.5e-02 )    3.80e-07    2.10e-06        1.06e-05      7.00e-05          -
    (20000, 64, 0.001, 0.9)            6.2e-01  (4.1e-01 )    5.76e-07    1.34e-05        5.95e-07      2.25e-05          -
    (20000, 128, 0.0, 0.995)           6.0e-01  (3.2e-02 )    3.95e-07    2.15e-06        2.12e-05      1.06e-03          -
    (20000, 20, 0.0, 0.9)              6.3e-01  (4.0e-01 )    3.72e-07    2.21e-06        6.54e-07      2.55e-05          -
    TOL = 8 x the largest floor -> one digit.  Adam: update 8 x 3.00e-5 -> 3e-4, row 8 x 4.23e-5 -> 4e-4, state 8 x 1.34e-5 -> 2e-4;
    SGD: update 8 x 5.76e-7 -> 5e-6, row 8 x 1.34e-5 -> 2e-4.
    The target's two measures are kept PER MOMENTUM: the target moves by about (1 - mom) of what the online table moves, its
    fp32 rounding does not shrink with it, so relative to T - T0 the floor at 0.995 is 20 .. 70 times the floor at 0.9 — one bound
    over both would be the 0.995 bound and blind at 0.9.  Each is 8 x the largest floor among the cases of that momentum:
      Adam  t_update 0.9: 8 x 2.70e-5 -> 3e-4   0.995: 8 x 1.09e-3 -> 9e-3    t_row 0.9: 8 x 2.13e-4 -> 2e-3   0.995: 8 x 1.54e-2 -> 2e-1
      SGD   t_update 0.9: 8 x 6.54e-7 -> 6e-6   0.995: 8 x 2.12e-5 -> 2e-4    t_row 0.9: 8 x 2.55e-5 -> 3e-4   0.995: 8 x 1.06e-3 -> 9e-3

Power (the wrong fp32 loops against TOL on the measure that sees them, smallest ratio figure / TOL over the cases that can show
them; every one is asserted to be at least 4):

    Adam: ema_skip 33 x (t_update 9.96e-3), ema_before_step 19 x (5.68e-3), ema_stale 9.8 x (8.81e-2), sweep_unreplayed 60 x
      (5.36e-1) on t_update; replay_skip 176 x (row 7.02e-2), run_short 207 x (row 8.27e-2).  ema_skip / ema_before_step are shown by
      the three momentum-0.9 cases only (see ``mutants``).
    SGD:  ema_skip 19 x (3.87e-3), ema_before_step 263 x (5.26e-2), ema_stale 5.0 x (9.98e-4, l2 != 0), sweep_unreplayed 1785 x
      (3.57e-1) on t_update; replay_skip 11 x (row 2.22e-3, l2 != 0), run_short 182 x (row 3.64e-2).

Wide and run-length cases (buir_lazy_ref.WIDE_CASES / RUN_CASES: the inputs of rowopt_ref's, 140,003 rows — four rows per wave,
more than one stride of the catch-up — and runs of exactly 1 .. 300 positions; tests/test_hip_rowopt_wide.py).  TOL_WIDE by the
same rule over these cases, a key of its own; TOL above is unchanged.  Floors:

    Adam (n_rows, D, l2, momentum)     update/table (target)  update_err  row_update_err  t_update_err  t_row_update_err  state_err
    (140003, 64, 0.001, 0.9)           1.1e-02  (3.2e-03 )    2.11e-05    2.11e-05        5.87e-05      5.92e-05          1.34e-05
    (140003, 20, 0.0, 0.995)           1.0e-02  (1.9e-04 )    1.95e-05    2.54e-05        1.78e-03      2.20e-02          1.31e-05
    (1000, 20, 0.001, 0.9)             4.6e-03  (6.6e-04 )    2.04e-05    2.04e-05        1.25e-04      1.25e-04          1.21e-05
    (1000, 64, 0.0, 0.995)             4.8e-03  (3.6e-05 )    2.02e-05    2.02e-05        3.47e-03      3.47e-03          1.32e-05
    (1000, 100, 0.0, 0.9)              5.0e-03  (7.2e-04 )    2.05e-05    2.05e-05        1.34e-04      1.34e-04          1.32e-05
    (1000, 128, 0.001, 0.995)          3.9e-03  (3.0e-05 )    2.10e-05    2.10e-05        3.54e-03      3.54e-03          1.29e-05
    SGD
    (140003, 64, 0.001, 0.9)           5.3e-01  (1.7e-01 )    4.09e-07    7.83e-06        1.08e-06      3.69e-05          -
    (140003, 20, 0.0, 0.995)           4.7e-01  (9.7e-03 )    2.38e-07    2.67e-06        3.59e-05      1.55e-03          -
    (1000, 20, 0.001, 0.9)             7.8e-01  (1.2e-01 )    4.39e-07    1.88e-06        8.90e-07      1.91e-05          -
    (1000, 64, 0.0, 0.995)             6.5e-01  (4.4e-03 )    4.50e-07    1.53e-06        2.63e-05      3.39e-04          -
    (1000, 100, 0.0, 0.9)              8.3e-01  (1.2e-01 )    4.18e-07    1.49e-06        8.62e-07      1.39e-05          -
    (1000, 128, 0.001, 0.995)          8.2e-01  (6.1e-03 )    2.89e-07    2.49e-06        1.72e-05      3.36e-04          -
    TOL_WIDE  Adam: update 8 x 2.11e-5 -> 2e-4, row 8 x 2.54e-5 -> 3e-4, state 8 x 1.34e-5 -> 2e-4, t_update 0.9: 8 x 1.34e-4 ->
      2e-3, 0.995: 8 x 3.54e-3 -> 3e-2, t_row 0.9: 8 x 1.34e-4 -> 2e-3, 0.995: 8 x 2.20e-2 -> 2e-1;  SGD: update 8 x 4.50e-7 -> 4e-6,
      row 8 x 7.83e-6 -> 7e-5, t_update 0.9: 8 x 1.08e-6 -> 9e-6, 0.995: 8 x 3.59e-5 -> 3e-4, t_row 0.9: 8 x 3.69e-5 -> 3e-4, 0.995:
      8 x 1.55e-3 -> 2e-2.
Power of the wide cases (``wide_mutants``; every one is asserted to exceed its tolerance at least 4 times; smallest figures):
    Adam, on row: fourth_row 7.06e-1 (2,354 x), stride_tail 7.06e-1, window_offset 3.56e-1 (1,188 x), run_trip 1.83 (6,114 x).
    SGD with decay, on row: fourth_row 1.24e-1 (1,774 x), stride_tail 1.22e-1, window_offset 3.84e-2 (549 x); without decay the
      online row does not move without a gradient and the target's rows show them, on t_row at momentum 0.995: fourth_row
      8.31e-1 (42 x), stride_tail 8.31e-1, window_offset 4.98e-1 (25 x); run_trip on row 6.97e-1 (9,954 x).
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buir_lazy_ref as B  # noqa: E402
from oracle import parity  # noqa: E402

# the tolerances tests/test_hip_buir_lazy.py imports
TOL = {"Adam": {"update": 3e-4, "row": 4e-4, "state": 2e-4, "t_update": {0.9: 3e-4, 0.995: 9e-3}, "t_row": {0.9: 2e-3, 0.995: 2e-1}},
       "SGD": {"update": 5e-6, "row": 2e-4, "t_update": {0.9: 6e-6, 0.995: 2e-4}, "t_row": {0.9: 3e-4, 0.995: 9e-3}}}
# ... and tests/test_hip_rowopt_wide.py: the wide and run-length cases (buir_lazy_ref.WIDE_CASES, RUN_CASES)
TOL_WIDE = {"Adam": {"update": 2e-4, "row": 3e-4, "state": 2e-4, "t_update": {0.9: 2e-3, 0.995: 3e-2}, "t_row": {0.9: 2e-3, 0.995: 2e-1}},
            "SGD": {"update": 4e-6, "row": 7e-5, "t_update": {0.9: 9e-6, 0.995: 3e-4}, "t_row": {0.9: 3e-4, 0.995: 2e-2}}}
POWER = 4.0                                  # a wrong step exceeds its tolerance at least this many times


def tol(opt, name, mom):
    """the tolerance of one measure; those of the target are kept per momentum (module docstring)"""
    t = TOL[opt][name]
    return t[mom] if isinstance(t, dict) else t


def figures(W0, ref, got):
    """the measures of a run (W, T, state) against the float64 run ref = (W64, T64, state64); T0 = W0"""
    fig = {"update": parity.update_err(got[0], ref[0], W0), "row": parity.row_update_err(got[0], ref[0], W0),
           "t_update": parity.update_err(got[1], ref[1], W0), "t_row": parity.row_update_err(got[1], ref[1], W0),
           "update_over_table": float(np.abs(ref[0] - W0).max() / np.abs(ref[0]).max()),
           "t_update_over_table": float(np.abs(ref[1] - W0).max() / np.abs(ref[1]).max())}
    if ref[2]:
        fig["state"] = max(parity.table_err(got[2][k], ref[2][k]) for k in ref[2])
    return fig


@functools.lru_cache(maxsize=None)
def case_runs(opt, case):
    """(W0, steps, float64 run, fp32 run, run(dtype, mutant)) of one case: computed once, shared, never modified"""
    n_rows, D, l2, mom = case
    W0, steps = B.make_case(n_rows, D)
    run = lambda dtype, mutant=None: B.dense_loop(opt, W0, steps, B.LR[opt], l2, mom, dtype, mutant=mutant)   # noqa: E731
    return W0, steps, run(np.float64), run(np.float32), run


def _round_up_one_digit(x):
    e = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / e - 1e-9) * e


# ------------------------------------------------------------------------------------------------ the flag
def test_flag_parses_for_buir():
    from whisprrec_amd import main as launcher
    base = ["--model_name", "BUIR", "--runner_name", "HipRunner"]
    args, model_class, _, _ = launcher.build_args(base)
    assert args.emb_lazy == 0 and model_class.__name__ == "BUIR"
    args, _, _, _ = launcher.build_args(base + ["--emb_lazy", "1", "--buir_native", "1"])
    assert args.emb_lazy == 1
    with pytest.raises(SystemExit):
        launcher.build_args(base + ["--emb_lazy", "2"])


def test_cases_hold_what_the_kernels_can_get_wrong():
    R = B.R
    assert B.CASES == ((1000, 64, 0.0, 0.995), (1000, 20, 1e-3, 0.9), (1000, 128, 1e-3, 0.995),
                       (20000, 64, 1e-3, 0.9), (20000, 128, 0.0, 0.995), (20000, 20, 0.0, 0.9))
    for n_rows in (1000, 20000):
        mine = [c for c in B.CASES if c[0] == n_rows]
        assert {c[1] for c in mine} == {64, 20, 128} and {c[2] for c in mine} == {0.0, 1e-3} and {c[3] for c in mine} == {0.995, 0.9}
    for n_rows, D, _, _ in B.CASES:
        W0, steps = B.make_case(n_rows, D)
        assert W0.shape == (n_rows, D) and len(steps) == 12 and [i.size for i, _ in steps] == list(R.STEP_SIZES)
        assert {i.size for i, _ in steps} == {0, 1, 333, 4099}
        used = [set(i.tolist()) for i, _ in steps]
        for k, (a, b) in R.GAP_USES.items():                     # absent exactly k steps between its two uses
            assert [t for t in range(1, 13) if R.GAP_ROW0 + k in used[t - 1]] == [a, b] and b - a - 1 == k
        assert sorted(R.GAP_USES) == [0, 1, 2, 3, 4, 5, 7]
        for t in R.HOT_STEPS:
            assert int((steps[t - 1][0] == R.HOT_ROW).sum()) == R.HOT_COUNT == 300
        every = np.concatenate([i for i, _ in steps])
        assert not np.isin(np.arange(n_rows - R.N_NEVER, n_rows), every).any() and every.min() >= 1 and every.max() < n_rows
        assert B.SKIP_ROW in used[0] and B.SKIP_ROW not in used[B.SKIP_STEP - 1] and B.STALE_ROW in used[0] and B.STALE_ROW in used[8]


def test_float64_loop_by_hand_on_one_row():
    """one Adam step with l2 and one target update, element by element"""
    W0 = np.asarray([[0.1, -0.2, 0.3, 0.4]], np.float32)
    src = np.asarray([[0.01, 0.02, -0.03, 0.0], [0.01, 0.0, 0.0, 0.0]], np.float32)
    W, T, S = B.dense_loop("Adam", W0, [(np.asarray([0, 0]), src)], 1e-3, 1e-3, 0.9, np.float64)
    f = lambda x: float(np.float32(x))   # noqa: E731
    g = src.astype(np.float64).sum(0) + f(1e-3) * W0[0].astype(np.float64)
    m, v = f(1 - 0.9) * g, f(1 - 0.999) * g * g
    w = W0[0] - (f(1e-3) / (1 - 0.9)) * (m / (np.sqrt(v) / math.sqrt(1 - 0.999) + f(1e-8)))
    t = W0[0].astype(np.float64) * f(0.9) + w * f(1.0 - 0.9)
    assert np.allclose(W[0], w, rtol=1e-13, atol=0) and np.allclose(S["m"][0], m, rtol=1e-13) and np.allclose(S["v"][0], v, rtol=1e-13)
    assert np.allclose(T[0], t, rtol=1e-13, atol=0) and f(1.0 - 0.9) != f(f(1.0) - f(0.9))
    # SGD without decay and without a gradient: w stays, the target of a row that has moved keeps following it
    W, T, _ = B.dense_loop("SGD", W0, [(np.asarray([0]), src[:1]), (np.zeros(0, np.int64), src[:0])], 0.5, 0.0, 0.9, np.float64)
    w = W0[0].astype(np.float64) - f(0.5) * src[0].astype(np.float64)
    t1 = W0[0].astype(np.float64) * f(0.9) + w * f(1.0 - 0.9)
    assert np.allclose(W[0], w, rtol=1e-13) and np.allclose(T[0], t1 * f(0.9) + w * f(1.0 - 0.9), rtol=1e-13)


# ------------------------------------------------------------------------------------------------ floors and tolerances
@pytest.mark.parametrize("opt", ["Adam", "SGD"])
def test_tolerances_are_eight_times_the_largest_floor(opt):
    floors = []
    for case in B.CASES:
        W0, _, ref, f32, _ = case_runs(opt, case)
        fig = figures(W0, ref, f32)
        print("floor %s %s: update/table %.1e (target %.1e) update_err %.2e row_update_err %.2e t_update_err %.2e t_row_update_err "
              "%.2e state_err %.2e" % (opt, case, fig["update_over_table"], fig["t_update_over_table"], fig["update"], fig["row"],
                                       fig["t_update"], fig["t_row"], fig.get("state", 0.0)))
        floors.append(fig)
    wrong = []
    for name, t in TOL[opt].items():
        for mom in (sorted(t) if isinstance(t, dict) else [None]):
            worst = max(f[name] for f, c in zip(floors, B.CASES) if mom is None or c[3] == mom)
            print("TOL %s %s %s: 8 x %.2e = %.1e -> %.0e" % (opt, name, mom or "", worst, 8 * worst, _round_up_one_digit(8 * worst)))
            if not (math.isclose(tol(opt, name, mom), _round_up_one_digit(8 * worst), rel_tol=1e-9) and 4 * worst < tol(opt, name, mom)):
                wrong.append((opt, name, mom, worst))
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------ wrong steps
SEEN_BY = {"ema_skip": "t_update", "ema_before_step": "t_update", "ema_stale": "t_update", "sweep_unreplayed": "t_update",
           "replay_skip": "row", "run_short": "row"}


def mutants(opt, case):
    """the wrong steps this case can show.  Without decay an SGD row without a gradient does not move: a lost zero-gradient step
    loses nothing ("replay_skip") and the w of every replayed step is the final one ("ema_stale").  ONE wrong target update under
    Adam at momentum 0.995 is 1.3e-2 .. 2.6e-2 of the target's update, below 4 x the tolerance there (9e-3: the target has moved
    by 6e-4 of its scale and fp32 rounds it at 1e-3 of that); the momentum-0.9 cases show those two."""
    _, _, l2, mom = case
    out = ["sweep_unreplayed", "run_short"]
    if not (opt == "Adam" and mom == 0.995):
        out += ["ema_skip", "ema_before_step"]
    if opt == "Adam" or l2 != 0:
        out += ["ema_stale", "replay_skip"]
    return out


@pytest.mark.parametrize("opt", ["Adam", "SGD"])
@pytest.mark.parametrize("case", B.CASES)
def test_wrong_steps_exceed_the_tolerances(opt, case):
    W0, _, ref, _, run = case_runs(opt, case)
    weak = []
    for mutant in mutants(opt, case):
        fig = figures(W0, ref, run(np.float32, mutant))
        name = SEEN_BY[mutant]
        bound = tol(opt, name, case[3])
        print("power %s %s %s: %s %.2e = %.1f x tol %.0e | update %.2e row %.2e t_update %.2e t_row %.2e" % (
            opt, case, mutant, name, fig[name], fig[name] / bound, bound, fig["update"], fig["row"], fig["t_update"], fig["t_row"]))
        if not fig[name] > POWER * bound:
            weak.append((mutant, name, fig[name], bound))
    assert not weak, (opt, case, weak)


def test_every_wrong_step_of_the_issue_is_exercised():
    seen = {m for opt in ("Adam", "SGD") for case in B.CASES for m in mutants(opt, case)}
    assert seen == set(B.MUTANTS) == set(SEEN_BY)
    for opt in ("Adam", "SGD"):                     # every wrong step meets both table sizes, with and without weight decay
        for m in B.MUTANTS:
            mine = [c for c in B.CASES if m in mutants(opt, c)]
            assert {c[0] for c in mine} == {1000, 20000} and 1e-3 in {c[2] for c in mine}, (opt, m)
            assert (m in ("ema_stale", "replay_skip") and opt == "SGD") or 0.0 in {c[2] for c in mine}, (opt, m)
    assert "ema_stale" not in mutants("SGD", B.CASES[0]) and "ema_stale" in mutants("SGD", B.CASES[1])


# ------------------------------------------------------------------------------------------------ wide and run-length cases
@functools.lru_cache(maxsize=None)
def wide_runs(opt, case):
    """(W0, steps, float64 run, run(dtype, mutant)) of one wide or run-length case: computed once, shared, never modified"""
    n_rows, D, l2, mom = case
    W0, steps = B.make_any_case(case)
    run = lambda dtype, mutant=None: B.dense_loop(opt, W0, steps, B.LR[opt], l2, mom, dtype, mutant=mutant)   # noqa: E731
    return W0, steps, run(np.float64), run


def tol_wide(opt, name, mom):
    t = TOL_WIDE[opt][name]
    return t[mom] if isinstance(t, dict) else t


def test_wide_cases_are_those_of_the_single_table():
    R = B.R
    assert B.WIDE_CASES == ((140003, 64, 1e-3, 0.9), (140003, 20, 0.0, 0.995)) and {c[1] for c in B.RUN_CASES} == {20, 64, 100, 128}
    for cases in (B.WIDE_CASES, B.RUN_CASES):
        assert {c[2] for c in cases} == {0.0, 1e-3} and {c[3] for c in cases} == {0.9, 0.995}
    for case in B.WIDE_CASES + B.RUN_CASES:
        W0, steps = B.make_any_case(case)
        W1, steps1 = R.make_any_case((case[0], case[1], -1, 0.0) if case in B.WIDE_CASES else
                                     [c for c in R.RUN_CASES if c[1] == case[1]][0])
        assert np.array_equal(W0, W1) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(steps, steps1))


def wide_mutants(opt, case):
    """(mutant, the measure that sees it).  The replay mutants lose optimizer steps and target updates of rows without a
    gradient: the online table shows them under Adam and under weight decay; under SGD without decay such a row does not
    move and only its target (which still follows the row) can show them."""
    if case in B.RUN_CASES:
        return [("run_trip", "row")]
    return [(m, "row" if (opt == "Adam" or case[2] != 0) else "t_row") for m in B.WIDE_MUTANTS]


@pytest.mark.parametrize("opt", ["Adam", "SGD"])
def test_wide_tolerances_are_eight_times_the_largest_floor(opt):
    cases = B.WIDE_CASES + B.RUN_CASES
    floors = []
    for case in cases:
        W0, _, ref, run = wide_runs(opt, case)
        fig = figures(W0, ref, run(np.float32))
        print("floor %s %s: update/table %.1e (target %.1e) update_err %.2e row_update_err %.2e t_update_err %.2e t_row_update_err "
              "%.2e state_err %.2e" % (opt, case, fig["update_over_table"], fig["t_update_over_table"], fig["update"], fig["row"],
                                       fig["t_update"], fig["t_row"], fig.get("state", 0.0)))
        floors.append(fig)
    wrong = []
    assert set(TOL_WIDE[opt]) == set(TOL[opt])
    for name, t in TOL_WIDE[opt].items():
        for mom in (sorted(t) if isinstance(t, dict) else [None]):
            worst = max(f[name] for f, c in zip(floors, cases) if mom is None or c[3] == mom)
            print("TOL_WIDE %s %s %s: 8 x %.2e = %.1e -> %.0e" % (opt, name, mom or "", worst, 8 * worst, _round_up_one_digit(8 * worst)))
            if not (math.isclose(tol_wide(opt, name, mom), _round_up_one_digit(8 * worst), rel_tol=1e-9)
                    and 4 * worst < tol_wide(opt, name, mom)):
                wrong.append((opt, name, mom, worst))
    assert not wrong, wrong


@pytest.mark.parametrize("opt", ["Adam", "SGD"])
@pytest.mark.parametrize("case", B.WIDE_CASES + B.RUN_CASES)
def test_wide_wrong_steps_exceed_the_tolerances(opt, case):
    W0, _, ref, run = wide_runs(opt, case)
    weak = []
    for mutant, name in wide_mutants(opt, case):
        fig = figures(W0, ref, run(np.float32, mutant))
        bound = tol_wide(opt, name, case[3])
        print("power %s %s %s: %s %.2e = %.1f x tol %.0e | update %.2e row %.2e t_update %.2e t_row %.2e" % (
            opt, case, mutant, name, fig[name], fig[name] / bound, bound, fig["update"], fig["row"], fig["t_update"], fig["t_row"]))
        if not fig[name] > POWER * bound:
            weak.append((mutant, name, fig[name], bound))
    assert not weak, (opt, case, weak)


def test_every_wide_wrong_step_is_exercised():
    for opt in ("Adam", "SGD"):
        seen = {m for case in B.WIDE_CASES + B.RUN_CASES for m, _ in wide_mutants(opt, case)}
        assert seen == set(B.WIDE_MUTANTS) | {"run_trip"}, opt
        for case in B.WIDE_CASES:                                 # a pair is always stateful: every wide case shows every one
            assert [m for m, _ in wide_mutants(opt, case)] == list(B.WIDE_MUTANTS)


# ------------------------------------------------------------------------------------------------ the interface, without a GPU
def _cpu_model(extra):
    from whisprrec_amd import host, main as launcher
    args, model_class, _, _ = launcher.build_args(["--model_name", "BUIR", "--runner_name", "HipRunner"] + extra)
    args.device = "cpu"
    return model_class(args, host.Corpus(7, 50, {}))


def test_model_installs_the_lazy_optimizer_or_says_why_not(caplog):
    import logging
    import torch
    from whisprrec_amd.buir import BuirLazyOptimizer
    off = _cpu_model(["--buir_native", "1"])
    assert off.optimizer is None and off.emb_lazy is False
    on = _cpu_model(["--buir_native", "1", "--emb_lazy", "1", "--optimizer", "SGD", "--l2", "1e-4"])
    assert isinstance(on.optimizer, BuirLazyOptimizer) and on.emb_lazy
    assert isinstance(on.optimizer.inner, torch.optim.SGD) and on.optimizer.l2 == 1e-4
    inner = [p for g in on.optimizer.param_groups for p in g["params"]]
    assert len(inner) == 2 and inner[0] is on.predictor.weight and inner[1] is on.predictor.bias
    assert set(on.state_dict()) == set(off.state_dict())                # checkpoints are unchanged (and nothing to flush yet)
    on.optimizer.zero_grad()
    with pytest.raises(RuntimeError, match="without a preceding training predict"):
        on.optimizer.step()
    torch_opt = torch.optim.SGD(off.parameters(), lr=0.1)
    off.optimizer = torch_opt                                            # the setter still hooks a torch optimizer ...
    assert "_optimizer_hook" in off.__dict__
    on.optimizer = on.optimizer                                          # ... and takes an object without hooks
    assert "_optimizer_hook" not in on.__dict__
    with caplog.at_level(logging.WARNING):
        a = _cpu_model(["--emb_lazy", "1"])
        b = _cpu_model(["--buir_native", "1", "--emb_lazy", "1", "--optimizer", "Adagrad"])
        c = _cpu_model(["--buir_native", "1", "--emb_lazy", "1", "--embedding_size", "20"])
    assert all(m.optimizer is None and not m.emb_lazy for m in (a, b, c))
    said = [r.getMessage() for r in caplog.records if "--emb_lazy 1" in r.getMessage()]
    assert len(said) == 3 and "buir_native" in said[0] and "Adagrad" in said[1] and "embedding_size=20" in said[2]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes
    import torch
    from whisprrec_amd import abi, hip_ops
    L = abi.lib()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    A = (0.0, 0.9, 0.999, 1e-8, 0.9, 0.1)
    assert L.wr_gather_rows_ema(p, None, p, p, p, 4, 4, p, 1, 0, p, 8, *A, p, p, None, None) == -1                  # no target
    assert L.wr_gather_rows_ema(p, p, p, p, p, 4, 6, p, 1, 0, p, 8, *A, p, p, None, None) == -2                     # D % 4
    assert L.wr_gather_rows_ema(p, p + 4, p, p, p, 4, 4, p, 1, 0, p, 8, *A, p, p, None, None) == -4                 # alignment
    assert L.wr_gather_rows_ema(p, p, p, p, p, 4, 4, p, 1, 8, p, 8, *A, p, p, None, None) != 0                      # step >= n_consts
    assert L.wr_gather_rows_ema(p, p, p, p, p, 4, 4, p, 1, 0, p, 8, 0.0, 0.9, 0.999, 1e-8, 1.5, 0.1, p, p, None, None) != 0
    assert L.wr_gather_rows_ema_sgd(p, p, None, 4, 4, p, 1, 0, 0.1, 0.0, 0.9, 0.1, p, p, None, None) == -1          # always stateful
    assert L.wr_adam_rows_sparse_ema(p, p, p, p, p, 4, 4, p, p, 1, p, 0, p, 8, *A, None, None) != 0                 # step 0
    assert L.wr_adam_rows_sparse_ema(p, p, p, p, p, 4, 4, p, p, 1, p, 8, p, 8, *A, None, None) != 0
    assert L.wr_sgd_rows_sparse_ema(p, p, None, 4, 4, p, p, 1, p, 1, 0.1, 0.0, 0.9, 0.1, None, None) == -1
    assert L.wr_sgd_rows_sparse_ema(p, p, p, 4, 4, p, p, -1, p, 1, 0.1, 0.0, 0.9, 0.1, None, None) != 0
    assert L.wr_adam_catchup_ema(p, p, p, None, p, 4, 4, 1, p, 8, *A, None) == -1
    assert L.wr_sgd_catchup_ema(p, p, p, 0, 4, 1, 0.1, 0.0, 0.9, 0.1, None) == -2                                   # no rows
    # nothing to do is not an error
    assert L.wr_adam_rows_sparse_ema(p, p, p, p, p, 4, 4, None, None, 0, None, 1, p, 8, *A, None, None) == 0
    assert L.wr_gather_rows_ema_sgd(p, p, p, 4, 4, None, 0, 0, 0.1, 0.0, 0.9, 0.1, None, None, None, None) == 0
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.RowLazyEmaTable(torch.zeros(4, 64), torch.zeros(4, 64), "Adam", 1e-3, 0.0, 0.9)
    with pytest.raises(ValueError):
        hip_ops.RowLazyEmaTable(torch.zeros(4, 64), torch.zeros(4, 64), "Adagrad", 1e-3, 0.0, 0.9)
