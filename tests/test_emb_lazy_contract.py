"""CPU checks for the row-lazy item table (--emb_lazy; include/whisprrec_hip.h K22): the flag, the tolerances of the float64
parity check of tests/test_hip_emb_lazy.py against the fp32 floor, and the wrong steps against those tolerances.  No GPU.

Floor: tests/rowopt_ref.py's dense loop in fp32 against the same loop in float64 — the reference against itself in lower
precision, never the code under test — on every case of rowopt_ref.CASES, the cases of the GPU tests.  TOL = 8 x the largest
floor, rounded up to one significant digit (8 x: oracle/parity.py's argument — the kernels contract multiply-adds and use
v_rcp_f32 / v_sqrt_f32, each worth a small multiple of one rounding), and every floor leaves a factor 4.

Measured floors (12 steps, tables ~ N(0, 0.1^2), gradient rows ~ N(0, 0.01^2); Adam lr 1e-3, SGD lr 0.5):

    Adam  (n_rows, D, padding_idx, l2)   update/table  update_err  row_update_err  state_err
    (1000, 64, 0, 0)                     2.3e-2        1.36e-5     1.69e-5         1.38e-5
    (1000, 20, -1, 1e-3)                 3.1e-2        1.16e-5     1.57e-5         1.26e-5
    (1000, 128, 0, 1e-3)                 2.5e-2        2.50e-5     3.61e-5         1.34e-5
    (1000, 64, -1, 0)                    2.4e-2        1.29e-5     1.52e-5         1.31e-5
    (20000, 64, 0, 0)                    1.7e-2        1.48e-5     2.75e-5         1.27e-5
    (20000, 20, 0, 1e-3)                 2.6e-2        1.65e-5     1.66e-5         1.33e-5
    (20000, 128, -1, 0)                  1.7e-2        1.64e-5     2.73e-5         1.32e-5
    (20000, 64, -1, 1e-3)                2.6e-2        1.76e-5     1.79e-5         1.29e-5
      TOL update 8 x 2.50e-5 = 2.0e-4 -> 2e-4   row 8 x 3.61e-5 = 2.9e-4 -> 3e-4   state 8 x 1.38e-5 = 1.1e-4 -> 2e-4
      (the state floor is 1 - beta2 formed in fp32, 1.3e-5, as tests/test_optim_power.py records for the BPRMF tables)
    SGD: update_err 2.4e-7 .. 6.5e-7, row_update_err 1.1e-6 .. 2.7e-6 without weight decay and 1.9e-6 / 2.7e-6 / 1.3e-5 / 7.8e-5 with
      it (rows that only decay move by 12 lr l2 |w|: twelve roundings of w are 1e-4 of that)
      TOL update 8 x 6.53e-7 = 5.2e-6 -> 6e-6   row 8 x 7.81e-5 = 6.3e-4 -> 7e-4

Power (row_update_err of the wrong fp32 loops, smallest over the cases that can show them; all are asserted on every case):
    Adam: one missed replay step 5.4e-2; padding row's gradient kept 1.0; a run's last position dropped 1.4e-2; bias
    corrections of step t + 1 5.6e-2; window sweep marking without replaying 3.3e-1.
    SGD: missed replay (l2 != 0) 2.2e-3; padding kept 2.0e+1; run's last position 3.0e-2; sweep (l2 != 0) 3.4e-2.

Wide and run-length cases (rowopt_ref.WIDE_CASES: 140,003 rows, 6 steps of up to 40,003 positions — the sizes from which the
kernels hold four rows per wave and stride over a table, tests/test_hip_rowopt_wide.py; RUN_CASES: 1,000 rows, two steps of runs
of exactly 1 .. 300 positions).  TOL_WIDE by the same rule over these cases, a key of its own; TOL above is unchanged.  Floors:

    Adam  (n_rows, D, padding_idx, l2)   update/table  update_err  row_update_err  state_err
    (140003, 64, 0, 0)                   9.3e-3        1.99e-5     3.15e-5         1.25e-5
    (140003, 20, -1, 1e-3)               1.2e-2        2.11e-5     2.14e-5         1.31e-5
    (1000, 20, -1, 1e-3)                 4.6e-3        2.04e-5     2.04e-5         1.21e-5
    (1000, 64, -1, 0)                    4.8e-3        2.02e-5     2.02e-5         1.32e-5
    (1000, 100, -1, 1e-3)                5.0e-3        3.96e-5     3.96e-5         1.32e-5
    (1000, 128, -1, 0)                   3.9e-3        2.10e-5     2.10e-5         1.28e-5
      TOL_WIDE update 8 x 3.96e-5 = 3.2e-4 -> 4e-4   row 8 x 3.96e-5 -> 4e-4   state 8 x 1.32e-5 = 1.1e-4 -> 2e-4
    SGD   (140003, 64, 0, 0)             4.3e-1        5.04e-7     2.07e-6
    (140003, 20, -1, 1e-3)               4.7e-1        3.68e-7     9.64e-6
    (1000, 20 / 64 / 100 / 128)          6.5e-1 .. 8.4e-1   3.30e-7 .. 4.50e-7   1.48e-6 .. 1.88e-6
      TOL_WIDE update 8 x 5.04e-7 = 4.0e-6 -> 5e-6   row 8 x 9.64e-6 = 7.7e-5 -> 8e-5
Power of the wide cases (row_update_err of the wrong fp32 loops, smallest over the cases that can show them; asserted on each):
    Adam: a wave's fourth row marked without replay at the flush 7.1e-1; rows above 131,072 marked without replay 7.1e-1; the
    max_lag = 4 window replaying one row too low 4.4e-1; a run of a multiple of 64 positions without its last 64: 1.8.
    SGD (the replay mutants with l2 != 0 only: without decay one table keeps no state and replays nothing): fourth row 1.7e-1;
    rows above 131,072 1.6e-1; window one row too low 4.7e-2; run without its last 64 positions 7.0e-1.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowopt_ref as R  # noqa: E402
from oracle import parity  # noqa: E402

# the tolerances tests/test_hip_emb_lazy.py imports
TOL = {"Adam": {"update": 2e-4, "row": 3e-4, "state": 2e-4}, "SGD": {"update": 6e-6, "row": 7e-4}}
# ... and tests/test_hip_rowopt_wide.py: the wide and run-length cases (rowopt_ref.WIDE_CASES, RUN_CASES)
TOL_WIDE = {"Adam": {"update": 4e-4, "row": 4e-4, "state": 2e-4}, "SGD": {"update": 5e-6, "row": 8e-5}}


def figures(W0, ref, got):
    """update_err / row_update_err / state_err of a run (W, state) against the float64 run ref = (W64, state64)"""
    fig = {"update": parity.update_err(got[0], ref[0], W0), "row": parity.row_update_err(got[0], ref[0], W0),
           "update_over_table": float(np.abs(ref[0] - W0).max() / np.abs(ref[0]).max())}
    if ref[1]:
        fig["state"] = max(parity.table_err(got[1][k], ref[1][k]) for k in ref[1])
    return fig


@functools.lru_cache(maxsize=None)
def case_runs(opt, case):
    """(W0, steps, float64 run, fp32 run) of one case: computed once, shared, never modified"""
    n_rows, D, pad, l2 = case
    W0, steps = R.make_case(n_rows, D, pad)
    run = lambda dtype, mutant=None: R.dense_loop(opt, W0, steps, R.LR[opt], l2, pad, dtype, mutant=mutant)   # noqa: E731
    return W0, steps, run(np.float64), run(np.float32), run


def _round_up_one_digit(x):
    e = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / e - 1e-9) * e


# ------------------------------------------------------------------------------------------------ the flag
@pytest.mark.parametrize("model_name", ["SASRec", "ContraRec", "IF4Rec"])
def test_flag_parses_on_the_three_models(model_name):
    from whisprrec_amd import main as launcher
    base = ["--model_name", model_name, "--runner_name", "HipRunner"]
    args, model_class, _, _ = launcher.build_args(base)
    assert args.emb_lazy == 0 and model_class.__name__ == model_name
    args, _, _, _ = launcher.build_args(base + ["--emb_lazy", "1"])
    assert args.emb_lazy == 1
    with pytest.raises(SystemExit):
        launcher.build_args(base + ["--emb_lazy", "2"])


def test_cases_hold_what_the_kernels_can_get_wrong():
    assert {c[0] for c in R.CASES} == {1000, 20000} and {c[1] for c in R.CASES} == {64, 20, 128}
    assert {c[2] for c in R.CASES} == {0, -1} and {c[3] for c in R.CASES} == {0.0, 1e-3}
    for n_rows, D, pad, _ in R.CASES:
        W0, steps = R.make_case(n_rows, D, pad)
        assert len(steps) == 12 and {i.size for i, _ in steps} == {0, 1, 333, 4099}
        used = [set(i.tolist()) for i, _ in steps]
        for k, (a, b) in R.GAP_USES.items():                     # absent exactly k steps between its two uses
            assert [t for t in range(1, 13) if R.GAP_ROW0 + k in used[t - 1]] == [a, b] and b - a - 1 == k
        assert sorted(R.GAP_USES) == [0, 1, 2, 3, 4, 5, 7]
        for t in R.HOT_STEPS:
            assert int((steps[t - 1][0] == R.HOT_ROW).sum()) == R.HOT_COUNT > 256
        every = np.concatenate([i for i, _ in steps])
        for r in range(R.ONCE_ROW0, R.ONCE_ROW0 + R.N_ONCE):
            assert int((every == r).sum()) == 1
        assert not np.isin(np.arange(n_rows - R.N_NEVER, n_rows), every).any() and every.min() >= 0 and every.max() < n_rows
        frac0 = float((every == 0).mean())
        assert (0.3 < frac0 < 0.45) if pad == 0 else frac0 == 0.0


def test_float64_loop_is_optim_f64_on_one_table():
    """the loop the tolerances hang on, against oracle/optim_parity.py's element formulas: one Adam step with l2 by hand"""
    W0 = np.asarray([[0.1, -0.2, 0.3, 0.4]], np.float32)
    src = np.asarray([[0.01, 0.02, -0.03, 0.0], [0.01, 0.0, 0.0, 0.0]], np.float32)
    W, S = R.dense_loop("Adam", W0, [(np.asarray([0, 0]), src)], 1e-3, 1e-3, -1, np.float64)
    f = lambda x: float(np.float32(x))   # noqa: E731
    g = src.astype(np.float64).sum(0) + f(1e-3) * W0[0].astype(np.float64)
    m, v = f(1 - 0.9) * g, f(1 - 0.999) * g * g
    w = W0[0] - (f(1e-3) / (1 - 0.9)) * (m / (np.sqrt(v) / math.sqrt(1 - 0.999) + f(1e-8)))
    assert np.allclose(W[0], w, rtol=1e-13, atol=0) and np.allclose(S["m"][0], m, rtol=1e-13) and np.allclose(S["v"][0], v, rtol=1e-13)


# ------------------------------------------------------------------------------------------------ floors and tolerances
@pytest.mark.parametrize("opt", ["Adam", "SGD"])
def test_tolerances_are_eight_times_the_largest_floor(opt):
    floors = []
    for case in R.CASES:
        W0, _, ref, f32, _ = case_runs(opt, case)
        fig = figures(W0, ref, f32)
        print("floor %s %s: update/table %.1e update_err %.2e row_update_err %.2e state_err %.2e" % (
            opt, case, fig["update_over_table"], fig["update"], fig["row"], fig.get("state", 0.0)))
        floors.append(fig)
    for name in TOL[opt]:
        worst = max(f[name] for f in floors)
        assert math.isclose(TOL[opt][name], _round_up_one_digit(8 * worst), rel_tol=1e-9), (opt, name, worst)
        assert 4 * worst < TOL[opt][name]


# ------------------------------------------------------------------------------------------------ wrong steps
def _mutants(opt, case):
    _, _, pad, l2 = case
    out = ["run_short"]
    if pad == 0:
        out.append("padding_kept")
    if opt == "Adam":
        out += ["replay_skip", "bias_next", "sweep_unreplayed"]
    elif l2 != 0:
        out += ["replay_skip", "sweep_unreplayed"]            # without decay an SGD row without a gradient does not move
    return out


@pytest.mark.parametrize("opt", ["Adam", "SGD"])
@pytest.mark.parametrize("case", R.CASES)
def test_wrong_steps_exceed_the_tolerances(opt, case):
    W0, _, ref, _, run = case_runs(opt, case)
    for mutant in _mutants(opt, case):
        fig = figures(W0, ref, run(np.float32, mutant))
        print("%s %s %s: update_err %.2e row_update_err %.2e (tol %.0e) state_err %.2e" % (
            opt, case, mutant, fig["update"], fig["row"], TOL[opt]["row"], fig.get("state", 0.0)))
        assert fig["row"] > TOL[opt]["row"] and fig["update"] > TOL[opt]["update"], (opt, case, mutant, fig)


def test_every_wrong_step_of_the_issue_is_exercised():
    seen = {m for opt in ("Adam", "SGD") for case in R.CASES for m in _mutants(opt, case)}
    assert seen == {"replay_skip", "padding_kept", "run_short", "bias_next", "sweep_unreplayed"}


# ------------------------------------------------------------------------------------------------ wide and run-length cases
@functools.lru_cache(maxsize=None)
def wide_runs(opt, case):
    """(W0, steps, float64 run, run(dtype, mutant)) of one wide or run-length case: computed once, shared, never modified"""
    n_rows, D, pad, l2 = case
    W0, steps = R.make_any_case(case)
    run = lambda dtype, mutant=None: R.dense_loop(opt, W0, steps, R.LR[opt], l2, pad, dtype, mutant=mutant)   # noqa: E731
    return W0, steps, run(np.float64), run


def test_wide_cases_hold_what_the_kernels_can_get_wrong():
    n_rows = R.WIDE_ROWS
    assert R.WIDE_CASES == ((140003, 64, 0, 0.0), (140003, 20, -1, 1e-3)) and n_rows % 4 == 3 and n_rows > R.WIDE_STRIDE == 131072
    assert [(n_rows + lag - 1) // lag for lag in R.WIDE_LAGS[1:]] == [35001, 70002]
    assert any(lo % 4 for _, lo, _ in R.window_pieces(n_rows, 4, R.WIDE_N_STEPS))
    for _, D, pad, _ in R.WIDE_CASES:
        W0, steps = R.make_wide_case(n_rows, D, pad)
        assert W0.shape == (n_rows, D) and [i.size for i, _ in steps] == [40003, 333, 40003, 0, 40003, 1]
        used = [set(i.tolist()) for i, _ in steps]
        uses_of = lambda r: tuple(t for t in range(1, 7) if r in used[t - 1])   # noqa: E731
        for row, u in R.wide_uses(n_rows).items():
            assert uses_of(row) == u, (row, u)
        for table in (R.WIDE_GAP_ROWS, R.WIDE_HIGH_GAP_ROWS):                    # absent exactly k steps between two uses
            assert sorted(table) == [0, 1, 2, 3, 4]
            for k, (row, u) in table.items():
                assert len(u) == 1 or u[1] - u[0] - 1 == k, (k, row, u)
        assert all(len(u) == 2 for _, u in R.WIDE_GAP_ROWS.values())
        assert all(row > R.WIDE_STRIDE for row, _ in R.WIDE_HIGH_GAP_ROWS.values()) and max(R.WIDE_ONCE_ROWS) > R.WIDE_STRIDE
        for t in R.WIDE_HOT_STEPS:
            assert int((steps[t - 1][0] == R.HOT_ROW).sum()) == R.HOT_COUNT > 256
        every = np.concatenate([i for i, _ in steps])
        for r in R.WIDE_ONCE_ROWS:
            assert int((every == r).sum()) == 1
        last = R.last_use(steps, n_rows)
        assert not np.isin(np.arange(n_rows - R.N_NEVER, n_rows), every).any() and every.min() >= 0 and every.max() < n_rows
        high = last[R.WIDE_STRIDE:]
        assert (high == 0).sum() > 1000 and (high > 0).sum() > 1000            # the second stride trip: replays and idle rows
        # groups of four: at the flush current / behind by one / by three / never used; after three steps (the gather test) and
        # before the last window current, behind by one or two, behind by three, never used
        assert [int(last[r]) for r in (12, 13, 14, 15)] == [6, 5, 3, 0] and tuple(steps[5][0]) == (12,)
        h = R.WIDE_STRIDE + 8
        assert [int(last[r]) for r in range(h, h + 4)] == [5, 5, 3, 0]
        for base in R.WIDE_MIX_ROW0:
            assert base % 4 == 0
            for g in range(R.WIDE_N_MIX):
                assert [uses_of(base + 4 * g + j) for j in range(4)] == [(1, 3, 5), (2,), (3,), ()]
        edges = R.wide_edge_rows(n_rows)
        assert edges == {70001: (1,), 105002: (1,), 35001: (3,)}
        frac0 = float((every == 0).mean())
        assert (0.3 < frac0 < 0.45) if pad == 0 else frac0 == 0.0
    q = R.make_wide_query(n_rows)
    assert q.size == 32771 and q.size % 4 == 3 and q.min() >= 0 and q.max() < n_rows
    assert q[0] == q[2] and q[1] == R.HOT_ROW and int(last[q[0]]) >= 3 and int(last[q[3]]) == 0
    assert int((q[4:8] > R.WIDE_STRIDE).sum()) == 2
    # the run-length case
    assert {c[1] for c in R.RUN_CASES} == {20, 64, 100, 128}
    for case in R.RUN_CASES:
        _, steps = R.make_any_case(case)
        for k, (idx, _) in enumerate(steps):
            rows, counts = np.unique(idx, return_counts=True)
            assert rows.size == R.RUN_ROWS and sorted(counts[counts > 1].tolist()) == [15, 16, 17, 63, 64, 65, 128, 129, 300]
            assert R.RUN_LENGTHS == (1, 15, 16, 17, 63, 64, 65, 128, 129, 300) and counts[rows == R.RUN_ROW_OF[k][1]] == 1
            assert int(counts[-1]) == (128, 64)[k] and rows[-1] == idx.max()     # the run that ends at the last position


def _wide_mutants(opt, case):
    """Stateless SGD (l2 = 0, one table) keeps no step numbers and replays nothing: a row without a gradient does not move, so
    the replay mutants have nothing to lose there — that case shows none of them."""
    if case in R.RUN_CASES:
        return ["run_trip"]
    return list(R.WIDE_MUTANTS) if (opt == "Adam" or case[3] != 0) else []


@pytest.mark.parametrize("opt", ["Adam", "SGD"])
def test_wide_tolerances_are_eight_times_the_largest_floor(opt):
    floors = []
    for case in R.WIDE_CASES + R.RUN_CASES:
        W0, _, ref, run = wide_runs(opt, case)
        fig = figures(W0, ref, run(np.float32))
        print("floor %s %s: update/table %.1e update_err %.2e row_update_err %.2e state_err %.2e" % (
            opt, case, fig["update_over_table"], fig["update"], fig["row"], fig.get("state", 0.0)))
        floors.append(fig)
    assert set(TOL_WIDE[opt]) == set(TOL[opt])
    for name in TOL_WIDE[opt]:
        worst = max(f[name] for f in floors)
        assert math.isclose(TOL_WIDE[opt][name], _round_up_one_digit(8 * worst), rel_tol=1e-9), (opt, name, worst)
        assert 4 * worst < TOL_WIDE[opt][name]


@pytest.mark.parametrize("opt", ["Adam", "SGD"])
@pytest.mark.parametrize("case", R.WIDE_CASES + R.RUN_CASES)
def test_wide_wrong_steps_exceed_the_tolerances(opt, case):
    W0, _, ref, run = wide_runs(opt, case)
    for mutant in _wide_mutants(opt, case):
        fig = figures(W0, ref, run(np.float32, mutant))
        print("%s %s %s: update_err %.2e row_update_err %.2e (tol %.0e) state_err %.2e" % (
            opt, case, mutant, fig["update"], fig["row"], TOL_WIDE[opt]["row"], fig.get("state", 0.0)))
        assert fig["row"] > TOL_WIDE[opt]["row"], (opt, case, mutant, fig)


def test_every_wide_wrong_step_is_exercised():
    for opt in ("Adam", "SGD"):
        seen = {m for case in R.WIDE_CASES + R.RUN_CASES for m in _wide_mutants(opt, case)}
        assert seen == set(R.WIDE_MUTANTS) | {"run_trip"}, opt
    assert _wide_mutants("SGD", R.WIDE_CASES[0]) == [] and R.WIDE_CASES[0][3] == 0.0


def source_constants():
    """the sizes at which wr_rowopt.hip and wr_lazy.hip change their kernel form, read out of the sources"""
    import re
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "whisprrec_amd", "csrc")
    text = {n: open(os.path.join(src, n)).read() for n in ("wr_rowopt.hip", "wr_lazy.hip", "wr_common.h")}

    def const(name, where):
        found = re.findall(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text[where])
        assert len(found) == 1, (name, where, found)
        return int(found[0])

    out = {"kSmallGather": const("kSmallGather", "wr_rowopt.hip"), "kGatherRowsPerWave": const("kGatherRowsPerWave", "wr_rowopt.hip"),
           "kSmallBatchKeys": const("kSmallBatchKeys", "wr_lazy.hip"), "kRowsPerWave": const("kRowsPerWave", "wr_lazy.hip"),
           "kBlock": const("kBlock", "wr_common.h")}
    for name, fn in (("wr_rowopt.hip", "catchup_grid"), ("wr_lazy.hip", "all_grid")):
        body = text[name].split("static inline unsigned %s(" % fn)[1].split("\n}")[0]
        cap = re.findall(r"cap\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", body)
        assert len(cap) == 1, (name, fn, cap)
        out["cap_" + fn] = int(cap[0][0]) * int(cap[0][1])
    return out


def test_wide_cases_cross_the_thresholds_of_the_sources():
    """a later change of a threshold, of the rows per wave or of the grid cap fails here instead of silently moving the wide
    cases back into the one-row-per-wave forms"""
    from oracle import optim_parity as op
    k = source_constants()
    print("source constants:", k)
    waves = k["kBlock"] // 64
    n_rows = R.WIDE_ROWS
    for small, per_wave, cap in ((k["kSmallGather"], k["kGatherRowsPerWave"], k["cap_catchup_grid"]),
                                 (k["kSmallBatchKeys"], k["kRowsPerWave"], k["cap_all_grid"])):
        assert per_wave > 1 and R.WIDE_STRIDE == cap * waves * per_wave
        assert n_rows > cap * waves * per_wave and n_rows % per_wave != 0                   # a second stride trip, a partial group
        assert cap * waves >= small                                                         # one row per wave never strides
        for lag in R.WIDE_LAGS[1:]:
            win = (n_rows + lag - 1) // lag
            assert win >= small, lag                                                        # both windows: several rows per wave
        assert any(lo % per_wave for _, lo, _ in R.window_pieces(n_rows, 4, R.WIDE_N_STEPS))
        assert R.WIDE_GATHER_N >= small and R.WIDE_GATHER_N % per_wave != 0
        assert (R.WIDE_GATHER_N - 4) < small                                                # [:32767] is the one-row form
        assert max(R.WIDE_STEP_SIZES) >= small and max(R.WIDE_STEP_SIZES) % per_wave != 0
    assert k["kSmallGather"] == 32768 and R.WIDE_GATHER_N - 4 == k["kSmallGather"] - 1
    c = op.case("F")
    assert c["B"] >= k["kSmallBatchKeys"] and 2 * c["B"] >= k["kSmallBatchKeys"]            # user keys and item keys of a batch
    assert c["nI"] == n_rows and c["nI"] > k["cap_all_grid"] * waves * k["kRowsPerWave"]
    assert [(c["nU"] + 1) // 2, (c["nI"] + 1) // 2] == [35001, 70002] and (c["nU"] + 1) // 2 >= k["kSmallBatchKeys"]


# ------------------------------------------------------------------------------------------------ the interface, without a GPU
def _cpu_model(model_name, extra):
    from whisprrec_amd import host, main as launcher
    args, model_class, _, _ = launcher.build_args(["--model_name", model_name, "--runner_name", "HipRunner", "--history_max", "8"] + extra)
    args.device = "cpu"
    return model_class(args, host.Corpus(7, 50, {}))


def test_models_install_the_lazy_optimizer_or_say_why_not(caplog):
    import logging
    import torch
    from whisprrec_amd.sasrec import HipEmbedding, RowLazyOptimizer
    for name in ("SASRec", "ContraRec", "IF4Rec"):
        off = _cpu_model(name, [])
        assert off.optimizer is None and off.emb_lazy is False
        on = _cpu_model(name, ["--emb_lazy", "1", "--optimizer", "SGD", "--l2", "1e-4"])
        emb, = [m for m in on.modules() if isinstance(m, HipEmbedding)]
        assert isinstance(on.optimizer, RowLazyOptimizer) and on.emb_lazy and emb._lazy is on.optimizer
        assert isinstance(on.optimizer.inner, torch.optim.SGD) and on.optimizer.l2 == 1e-4
        inner = [p for g in on.optimizer.param_groups for p in g["params"]]
        assert all(p is not emb.weight for p in inner) and len(inner) == len(list(on.parameters())) - 1
        assert set(on.state_dict()) == set(off.state_dict())            # checkpoints are unchanged (and nothing to flush yet)
        on.optimizer.zero_grad()
        with pytest.raises(RuntimeError, match="without a preceding training predict"):
            on.optimizer.step()
    with caplog.at_level(logging.WARNING):
        a = _cpu_model("SASRec", ["--emb_lazy", "1", "--optimizer", "Adagrad"])
        b = _cpu_model("IF4Rec", ["--emb_lazy", "1", "--interest_native", "1"])
    assert a.optimizer is None and b.optimizer is None and not a.emb_lazy and not b.emb_lazy
    said = [r.getMessage() for r in caplog.records if "--emb_lazy 1" in r.getMessage()]
    assert len(said) == 2 and "Adagrad" in said[0] and "interest_native" in said[1]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes
    import torch
    from whisprrec_amd import abi, hip_ops
    L = abi.lib()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    assert L.wr_gather_rows_lazy(None, p, p, p, 4, 4, p, 1, 0, p, 8, 0.0, 0.9, 0.999, 1e-8, p, None, None) == -1
    assert L.wr_gather_rows_lazy(p, p, p, p, 4, 6, p, 1, 0, p, 8, 0.0, 0.9, 0.999, 1e-8, p, None, None) == -2      # D % 4
    assert L.wr_gather_rows_lazy(p, p, p, p, 4, 4, p, 1, 8, p, 8, 0.0, 0.9, 0.999, 1e-8, p, None, None) != 0       # step >= n_consts
    assert L.wr_adam_rows_sparse(p, p, p, p, 4, 4, p, p, 1, p, -1, 0, p, 8, 0.0, 0.9, 0.999, 1e-8, None, None) != 0  # step 0
    assert L.wr_adam_rows_sparse(p, p, p, p, 4, 4, p, p, 1, p, -1, 8, p, 8, 0.0, 0.9, 0.999, 1e-8, None, None) != 0
    assert L.wr_sgd_rows_sparse(p, None, 4, 4, p, p, 1, p, -1, 1, 0.1, 1e-3, None, None) == -1                     # decay needs last
    assert L.wr_rows_sparse_keys(p, -1, 4, p, None, None) != 0
    assert L.wr_gather_rows_lazy_sgd(p, None, 4, 4, p, 1, 0, 0.1, 1e-3, p, None, None) == -1
    # nothing to do is not an error
    assert L.wr_adam_rows_sparse(p, p, p, p, 4, 4, None, None, 0, None, -1, 1, p, 8, 0.0, 0.9, 0.999, 1e-8, None, None) == 0
    assert L.wr_rows_sparse_keys(None, 0, 4, None, None, None) == 0
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.RowLazyTable(torch.zeros(4, 64), "Adam", 1e-3, 0.0)
    with pytest.raises(ValueError):
        hip_ops.RowLazyTable(torch.zeros(4, 64), "Adagrad", 1e-3, 0.0)
