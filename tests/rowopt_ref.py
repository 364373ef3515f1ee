"""NumPy restatement of dense torch.optim.Adam / SGD on ONE table fed by given gradient rows — the reference of the row-lazy
optimizer tests (tests/test_emb_lazy_contract.py, tests/test_hip_emb_lazy.py).  A helper, not a test; no BPR in it.

``dense_loop``: torch's single-tensor formulas, every row at every step, as oracle/optim_parity.py::optim_f64 writes them: per
step a zero gradient table, the step's rows ``src[k]`` added at ``idx[k]`` in position order (``padding_idx`` dropped), then
the optimizer over the whole table.  ``dtype=np.float64`` is the reference; ``dtype=np.float32`` is the same loop in the
precision of the kernels — every operation rounded to fp32, 1 - beta formed in fp32 as fp32 code forms it (the project's C
oracle does the same; tests/test_optim_power.py records that this, not rounding, is the floor of the Adam state) — and gives
the floors the tolerances are derived from.  ``mutant`` builds one wrong step into the loop for the power checks.

``make_case``: the inputs of one case of the GPU tests, built so that the kernels' paths are all taken (see its docstring).
"""
import math

import numpy as np

F32 = np.float32
N_STEPS = 12
STEP_SIZES = (4099, 333, 4099, 333, 4099, 1, 333, 0, 4099, 333, 4099, 333)      # positions of steps 1 .. 12
# (first use, next use) of the rows that are absent for 0, 1, 2, 3, 4, 5 and 7 steps in between (steps are 1-based)
GAP_USES = {0: (1, 2), 1: (1, 3), 2: (1, 4), 3: (1, 5), 4: (2, 7), 5: (3, 9), 7: (1, 9)}
GAP_ROW0, HOT_ROW, HOT_COUNT, ONCE_ROW0, N_ONCE, FIRST_FREE_ROW, N_NEVER = 10, 5, 300, 30, 10, 100, 50
HOT_STEPS = (1, 5)
SWEEP_LAG = 4                                       # the window of the "sweep" mutant: max_lag = 4, as in the GPU lag test

# (n_rows, D, padding_idx, l2): every value the issue lists occurs, each table size with each D, both padding variants and
# both l2 with each table size.  20,000 rows: wr_scatter_add_rows' row plan (beyond 16,383 rows) in the dense arm.
CASES = ((1000, 64, 0, 0.0), (1000, 20, -1, 1e-3), (1000, 128, 0, 1e-3), (1000, 64, -1, 0.0),
         (20000, 64, 0, 0.0), (20000, 20, 0, 1e-3), (20000, 128, -1, 0.0), (20000, 64, -1, 1e-3))
LR = {"Adam": 1e-3, "SGD": 0.5}                     # the update of the run is ~1e-1 (Adam) / ~1e-1 (SGD) of the table's scale


def _f(x):
    return float(F32(x))


def make_case(n_rows, D, padding_idx, seed=0):
    """-> (W0 float32 [n_rows, D] ~ N(0, 0.1^2), steps = [(idx int64 [n], src float32 [n, D] ~ N(0, 0.01^2))] * 12).
    n follows STEP_SIZES (0, 1, 333 and 4,099 positions: none, one wave, several workgroups, a size that is no multiple of
    anything).  Row HOT_ROW occurs HOT_COUNT (> 256) times in the steps HOT_STEPS; rows ONCE_ROW0 .. +N_ONCE occur exactly once
    in the whole run (step 3); row GAP_ROW0 + k is used at the two steps GAP_USES[k] and at no other, i.e. is absent k steps in
    between (the replay is unrolled by four: 0 .. 5 and 7 cover every remainder and a second trip); the last N_NEVER rows and
    rows 1 .. 4 are never used.  padding_idx = 0: about 40 % of the other positions are 0.  The rest is uniform over
    [FIRST_FREE_ROW, n_rows - N_NEVER): many repeats at 1,000 rows, mostly single occurrences at 20,000."""
    rng = np.random.RandomState(1234 + seed + 7 * n_rows + D)
    W0 = (rng.standard_normal((n_rows, D)) * 0.1).astype(F32)
    steps = []
    for t, n in enumerate(STEP_SIZES, start=1):
        idx = rng.randint(FIRST_FREE_ROW, n_rows - N_NEVER, size=n).astype(np.int64)
        if padding_idx == 0 and n > 1:
            idx[rng.random_sample(n) < 0.4] = 0
        fixed = []
        if n >= 333:
            fixed += [GAP_ROW0 + k for k, uses in GAP_USES.items() if t in uses]
            if t == 3:
                fixed += list(range(ONCE_ROW0, ONCE_ROW0 + N_ONCE))
            if t in HOT_STEPS:
                fixed += [HOT_ROW] * HOT_COUNT
        if fixed:
            at = rng.choice(n, size=len(fixed), replace=False)
            idx[at] = np.asarray(fixed, dtype=np.int64)
        src = (rng.standard_normal((n, D)) * 0.01).astype(F32)
        steps.append((idx, src))
    return W0, steps


def grad_table(idx, src, n_rows, padding_idx, dtype, drop_last_of=None, keep_padding=False, drop_trip=False):
    """embedding_dense_backward: zero table, src rows added at idx in position order, padding_idx dropped.
    drop_last_of = row: the last position of that row's run is left out (a wrong step); keep_padding: another; drop_trip: a
    run whose length is a multiple of 64 loses its last 64 positions (a third)."""
    G = np.zeros((n_rows, src.shape[1]), dtype=dtype)
    keep = np.ones(idx.size, bool) if keep_padding else idx != padding_idx
    if drop_last_of is not None:
        keep[np.flatnonzero(idx == drop_last_of)[-1]] = False
    if drop_trip:
        rows, counts = np.unique(idx, return_counts=True)
        for row in rows[counts % 64 == 0]:
            keep[np.flatnonzero(idx == row)[-64:]] = False
    np.add.at(G, idx[keep], src[keep].astype(dtype))      # unbuffered: repeated rows accumulate one by one, in order
    return G


def lost_by_unreplayed_sweep(steps, n_rows, lag=SWEEP_LAG):
    """the zero-gradient steps that are lost when the rotating window (ceil(n_rows / lag) rows before every step but the
    first) marks its rows as current without replaying them: {step s: rows whose step s never happens}"""
    last = np.zeros(n_rows, np.int64)
    lost = {}
    pos, win = 0, (n_rows + lag - 1) // lag
    for t, (idx, _) in enumerate(steps, start=1):
        if t > 1:
            rows = (pos + np.arange(win)) % n_rows
            pos = (pos + win) % n_rows
            for s in range(1, t):
                hit = rows[last[rows] < s]
                if hit.size:
                    lost.setdefault(s, []).append(hit)
            last[rows] = np.maximum(last[rows], t - 1)
        last[np.unique(idx)] = t
    return {s: np.unique(np.concatenate(v)) for s, v in lost.items()}


def dense_loop(opt, W0, steps, lr, l2=0.0, padding_idx=-1, dtype=np.float64, betas=(0.9, 0.999), eps=1e-8, mutant=None):
    """-> (W, {"m": m, "v": v}) (Adam) or (W, {}) (SGD) after the steps, in `dtype`.  mutant (one wrong step each):
    "replay_skip"      one zero-gradient step of one row does not happen (the row GAP_ROW0 + 1, the step between its uses);
    "padding_kept"     the padding row's gradient is not dropped;
    "run_short"        the last position of the hot row's run is left out of its sum (its first hot step);
    "bias_next"        the bias corrections of step t + 1;
    "sweep_unreplayed" the window sweep (max_lag = SWEEP_LAG) marks rows current without replaying them;
    "fourth_row", "stride_tail", "window_offset"  the replay mutants of the wide cases (lost_of);
    "run_trip"         a run whose length is a multiple of 64 loses its last 64 positions (the run-length case)."""
    f = dtype
    W = np.array(W0, dtype=f)
    n_rows = W.shape[0]
    lr, l2 = f(_f(lr)), f(_f(l2))
    b1, b2, eps = f(_f(betas[0])), f(_f(betas[1])), f(_f(eps))
    if f is np.float32:
        omb1, omb2 = F32(1) - F32(betas[0]), F32(1) - F32(betas[1])
    else:
        omb1, omb2 = f(_f(1.0 - betas[0])), f(_f(1.0 - betas[1]))
    m, v = np.zeros_like(W), np.zeros_like(W)
    lost = {}
    if mutant == "replay_skip":
        lost = {GAP_USES[1][0] + 1: np.asarray([GAP_ROW0 + 1])}
    elif mutant == "sweep_unreplayed":
        lost = lost_by_unreplayed_sweep(steps, n_rows)
    elif mutant in WIDE_MUTANTS:
        lost = lost_of(mutant, steps, n_rows)
    for t, (idx, src) in enumerate(steps, start=1):
        G = grad_table(idx, src, n_rows, padding_idx, f,
                       drop_last_of=HOT_ROW if (mutant == "run_short" and t == HOT_STEPS[0]) else None,
                       keep_padding=mutant == "padding_kept", drop_trip=mutant == "run_trip")
        rows = lost.get(t)
        keep = None if rows is None else [a[rows].copy() for a in (W, m, v)]
        if l2 != 0:
            G += l2 * W
        if opt == "Adam":
            tb = t + 1 if mutant == "bias_next" else t
            bc1, bc2 = 1.0 - betas[0] ** tb, 1.0 - betas[1] ** tb
            m += omb1 * (G - m)
            v *= b2
            v += omb2 * G * G
            W -= f(_f(lr) / bc1) * (m / (np.sqrt(v) / f(math.sqrt(bc2)) + eps))
        else:
            W -= lr * G
        if keep is not None:
            W[rows], m[rows], v[rows] = keep
    return W, ({"m": m, "v": v} if opt == "Adam" else {})


# ------------------------------------------------------------------------------------------------ wide and run-length cases
# The kernels of whisprrec_amd/csrc/wr_rowopt.hip and wr_lazy.hip hold four rows per wave (R = 4) from 32,768 positions / rows
# of a call on, and their catch-up walks a table in strides of 131,072 rows (grid cap 256 * 32 workgroups x 4 waves x 4 rows).
# The wide cases are the smallest that cross both; tests/test_emb_lazy_contract.py reads the constants from the sources.
WIDE_ROWS = 140003                                  # > 131,072; % 4 = 3: the last group of four is partial
WIDE_STEP_SIZES = (40003, 333, 40003, 0, 40003, 1)  # positions of steps 1 .. 6; 40,003 % 4 = 3
WIDE_N_STEPS = len(WIDE_STEP_SIZES)
WIDE_STRIDE = 131072                                # rows of one stride trip of the R = 4 catch-up
WIDE_LAGS = (0, 4, 2)                               # windows of 35,001 (starts no multiple of 4) and 70,002 rows
WIDE_HOT_STEPS = (1, 5)
WIDE_GATHER_N = 32771                               # positions of the wide gather query; % 4 = 3
# rows below WIDE_FREE_LO and in [WIDE_STRIDE, WIDE_FREE_HI) are used only as listed here; the last N_NEVER rows never
WIDE_FREE_LO, WIDE_FREE_HI = 1000, 133000
# row -> the steps (1-based) that use it.  Gaps of 0 .. 4 missed steps, low and above the stride (there the row of gap 4 has
# its first use only: step 6 has one position, row 12).  Rows 12 .. 15 are a group of four that holds at the flush a current
# row, a row behind by one step, one behind by three and one never used; rows H + 4 .. H + 7 above the stride two rows behind by
# one step, one behind by three and one never used
_H = WIDE_STRIDE + 4
WIDE_GAP_ROWS = {0: (10, (1, 2)), 3: (11, (1, 5)), 4: (12, (1, 6)), 2: (13, (2, 5)), 1: (14, (1, 3))}       # gap -> (row, uses)
WIDE_HIGH_GAP_ROWS = {0: (_H, (1, 2)), 3: (_H + 1, (1, 5)), 4: (_H + 2, (1,)), 2: (_H + 5, (2, 5)), 1: (_H + 6, (1, 3))}
WIDE_HIGH_FOUR = {_H + 4: (3, 5)}                   # with _H + 5 (behind one), _H + 6 (behind three), _H + 7 (never)
WIDE_ONCE_ROWS = tuple(range(ONCE_ROW0, ONCE_ROW0 + N_ONCE)) + tuple(range(132500, 132500 + N_ONCE))      # step 3, once
# groups of four 4k .. 4k + 3: used at (1, 3, 5) / (2,) / (3,) / never — at step 3 (the state of the gather test) current, behind
# by one, current, behind by three; before step 6 (the last window) current, behind by three, behind by two, never used
WIDE_MIX_ROW0 = (200, 132000)
WIDE_N_MIX = 8
WIDE_MIX_USES = ((1, 3, 5), (2,), (3,), ())


def window_pieces(n_rows, lag, n_steps):
    """the (step t, first row, rows) pieces of the rotating window of RowLazyTable (ceil(n_rows / lag) rows before every step
    t > 1, brought to step t - 1, in up to two pieces across the wrap-around)"""
    out, lo = [], 0
    for t in range(2, n_steps + 1):
        left = min((n_rows + lag - 1) // lag, n_rows)
        while left > 0:
            c = min(left, n_rows - lo)
            out.append((t, lo, c))
            lo, left = (lo + c) % n_rows, left - c
    return out


def wide_edge_rows(n_rows=WIDE_ROWS, lag=SWEEP_LAG, n_steps=WIDE_N_STEPS):
    """{last row of a window piece that is brought to a step >= 2: (the one step that uses it,)}: these rows have moments when
    their window comes, so a window that leaves its last row out ("window_offset") loses real steps"""
    out = {}
    for t, lo, c in window_pieces(n_rows, lag, n_steps):
        r = lo + c - 1
        if t - 1 >= 2 and WIDE_FREE_LO <= r < n_rows - N_NEVER and r not in out:
            out[r] = (1,) if t - 1 < 4 else (3,)
    return out


def wide_uses(n_rows=WIDE_ROWS):
    """row -> steps, every hand-placed row of a wide case but the hot row"""
    uses = {}
    for table in (WIDE_GAP_ROWS, WIDE_HIGH_GAP_ROWS):
        uses.update({row: u for row, u in table.values()})
    uses.update(WIDE_HIGH_FOUR)
    uses.update({r: (3,) for r in WIDE_ONCE_ROWS})
    for base in WIDE_MIX_ROW0:
        for g in range(WIDE_N_MIX):
            uses.update({base + 4 * g + j: u for j, u in enumerate(WIDE_MIX_USES) if u})
    uses.update(wide_edge_rows(n_rows))
    return uses


def _wide_free_rows(rng, n_rows, n, avoid):
    """uniform over [WIDE_FREE_LO, WIDE_STRIDE) and [WIDE_FREE_HI, n_rows - N_NEVER), never a row of `avoid` (sorted)"""
    low = WIDE_STRIDE - WIDE_FREE_LO
    r = rng.randint(0, low + (n_rows - N_NEVER - WIDE_FREE_HI), size=n).astype(np.int64)
    r = np.where(r < low, r + WIDE_FREE_LO, r - low + WIDE_FREE_HI)
    hit = np.isin(r, avoid)
    r[hit] += 2                                      # the edge rows are isolated: row + 2 is an ordinary row
    return r


def make_wide_case(n_rows, D, padding_idx, seed=0):
    """-> (W0 float32 [n_rows, D] ~ N(0, 0.1^2), steps = [(idx int64 [n], src float32 [n, D] ~ N(0, 0.01^2))] * 6), n as
    WIDE_STEP_SIZES.  As make_case: the hot row (HOT_COUNT times in the steps WIDE_HOT_STEPS), rows with gaps of 0 .. 4 missed
    steps, rows used once, rows never used (1 .. 4, the last N_NEVER, most of [WIDE_STRIDE, WIDE_FREE_HI)), 40 % padding
    positions with padding_idx = 0 — and, for the forms with four rows per wave and the stride loop: gap and once rows above
    row WIDE_STRIDE, groups of four that mix current, late and never-used rows below and above it, and the last row of every
    window piece (max_lag = SWEEP_LAG) used before its window comes.  The rest is uniform over the free rows."""
    assert n_rows > WIDE_FREE_HI + N_NEVER
    rng = np.random.RandomState(4321 + seed + 7 * n_rows + D)
    W0 = (rng.standard_normal((n_rows, D)) * 0.1).astype(F32)
    uses = wide_uses(n_rows)
    avoid = np.asarray(sorted(wide_edge_rows(n_rows)), dtype=np.int64)
    steps = []
    for t, n in enumerate(WIDE_STEP_SIZES, start=1):
        idx = _wide_free_rows(rng, n_rows, n, avoid)
        if padding_idx == 0 and n > 1:
            idx[rng.random_sample(n) < 0.4] = 0
        fixed = [row for row, u in sorted(uses.items()) if t in u]
        if t in WIDE_HOT_STEPS:
            fixed += [HOT_ROW] * HOT_COUNT
        assert len(fixed) <= n, (t, len(fixed), n)
        if fixed:
            at = rng.choice(n, size=len(fixed), replace=False)
            idx[at] = np.asarray(fixed, dtype=np.int64)
        src = (rng.standard_normal((n, D)) * 0.01).astype(F32)
        steps.append((idx, src))
    return W0, steps


def make_wide_query(n_rows, seed=0):
    """the gather query of the wide tests, WIDE_GATHER_N positions (R = 4, n % 4 = 3).  Group 0: a duplicate, the hot row, a row
    that is current after three steps and a never-used row; group 1: two rows above the stride; then the groups of four of
    make_wide_case, the gap and once rows; the rest uniform over the table."""
    rng = np.random.RandomState(77 + seed)
    cur = WIDE_MIX_ROW0[0]                           # used at step 3
    head = [cur, HOT_ROW, cur, 1,
            WIDE_HIGH_GAP_ROWS[1][0], 7, WIDE_ONCE_ROWS[-1], 8,
            12, 13, 14, 15, _H + 4, _H + 5, _H + 6, _H + 7, n_rows - 1, n_rows - 2, 0, 0]
    head += [b + j for b in WIDE_MIX_ROW0 for j in range(4 * WIDE_N_MIX)]
    head += [row for row, _ in WIDE_GAP_ROWS.values()] + [row for row, _ in WIDE_HIGH_GAP_ROWS.values()] + list(WIDE_ONCE_ROWS)
    q = np.concatenate([np.asarray(head, np.int64), rng.randint(0, n_rows, WIDE_GATHER_N - len(head)).astype(np.int64)])
    assert q.size == WIDE_GATHER_N
    return q


# one table: (n_rows, D, padding_idx, l2)
WIDE_CASES = ((WIDE_ROWS, 64, 0, 0.0), (WIDE_ROWS, 20, -1, 1e-3))

# run-length case: the sparse step (rows_sparse_kernel / run_sum: 64 entries of a run per trip, kRunFly = 16 gradient rows in
# flight).  D = 100: above 64 and no multiple of it — the second element trip has lanes without an element.
RUN_ROWS = 1000
RUN_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 128, 129, 300)
# run length -> row, per step.  Step 1: the largest id has the run of 128, which so ends at the step's last position; step 2:
# the run of 64 is the last
RUN_ROW_OF = ({1: 10, 15: 20, 16: 30, 17: 40, 63: 50, 64: 60, 65: 61, 129: 80, 300: 90, 128: RUN_ROWS - 1},
              {1: 10, 15: 20, 16: 30, 17: 40, 63: 50, 128: 60, 65: 61, 129: 80, 300: 90, 64: RUN_ROWS - 1})
RUN_CASES = ((RUN_ROWS, 20, -1, 1e-3), (RUN_ROWS, 64, -1, 0.0), (RUN_ROWS, 100, -1, 1e-3), (RUN_ROWS, 128, -1, 0.0))


def make_run_case(n_rows, D, padding_idx=-1, seed=0):
    """-> (W0, steps): two steps whose positions are runs of exactly RUN_LENGTHS positions on the rows RUN_ROW_OF and one
    position on every other row (every row moves at every step: the per-row measure has no row that only rounds), in a
    random order of the positions (the order within a run is the order of the sum)"""
    assert n_rows == RUN_ROWS and padding_idx == -1
    rng = np.random.RandomState(999 + seed + D)
    W0 = (rng.standard_normal((n_rows, D)) * 0.1).astype(F32)
    steps = []
    for rows in RUN_ROW_OF:
        idx = np.concatenate([np.full(length, row, np.int64) for length, row in rows.items()]
                             + [np.setdiff1d(np.arange(n_rows), list(rows.values()))])
        rng.shuffle(idx)
        steps.append((idx, (rng.standard_normal((idx.size, D)) * 0.01).astype(F32)))
    return W0, steps


def make_any_case(case, seed=0):
    """make_case / make_wide_case / make_run_case by the case tuple (n_rows, D, padding_idx, ...)"""
    n_rows, D, pad = case[:3]
    if case in RUN_CASES:
        return make_run_case(n_rows, D, pad, seed)
    return (make_wide_case if n_rows == WIDE_ROWS else make_case)(n_rows, D, pad, seed)


def last_use(steps, n_rows):
    """per row the last step that has it (0: none)"""
    last = np.zeros(n_rows, np.int64)
    for t, (idx, _) in enumerate(steps, start=1):
        last[idx] = t
    return last


def lost_at_flush(steps, n_rows, rows):
    """the steps lost when the flush marks `rows` (a mask) current without replaying them: {step s: rows that are behind s}"""
    last, n = last_use(steps, n_rows), len(steps)
    return {s: np.flatnonzero(rows & (last < s)) for s in range(1, n + 1) if (rows & (last < s)).any()}


def lost_by_window_offset(steps, n_rows, lag=SWEEP_LAG):
    """the steps lost when every piece of the rotating window replays rows lo - 1 .. lo + c - 2 and marks lo .. lo + c - 1: the
    piece's last row is marked without its replay (row lo - 1 was the last row of the piece before, marked current already)"""
    last = np.zeros(n_rows, np.int64)
    lost = {}
    pieces = window_pieces(n_rows, lag, len(steps))
    for t, (idx, _) in enumerate(steps, start=1):
        for _, lo, c in [p for p in pieces if p[0] == t]:
            r = lo + c - 1
            for s in range(last[r] + 1, t):
                lost.setdefault(s, []).append(r)
            last[lo:lo + c] = np.maximum(last[lo:lo + c], t - 1)
        last[np.unique(idx)] = t
    return {s: np.unique(np.asarray(v, np.int64)) for s, v in lost.items()}


def lost_of(mutant, steps, n_rows):
    """the lost (step, rows) of the replay mutants of the wide cases, None for any other mutant:
    "fourth_row"     at the flush, rows with r % 4 == 3 are marked current without replay (a stale fourth row of a wave);
    "stride_tail"    the same for rows >= WIDE_STRIDE (no second trip of the stride loop);
    "window_offset"  see lost_by_window_offset (max_lag = SWEEP_LAG)."""
    r = np.arange(n_rows)
    if mutant == "fourth_row":
        return lost_at_flush(steps, n_rows, r % 4 == 3)
    if mutant == "stride_tail":
        return lost_at_flush(steps, n_rows, r >= WIDE_STRIDE)
    if mutant == "window_offset":
        return lost_by_window_offset(steps, n_rows)
    return None


WIDE_MUTANTS = ("fourth_row", "stride_tail", "window_offset")
