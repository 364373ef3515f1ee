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


def grad_table(idx, src, n_rows, padding_idx, dtype, drop_last_of=None, keep_padding=False):
    """embedding_dense_backward: zero table, src rows added at idx in position order, padding_idx dropped.
    drop_last_of = row: the last position of that row's run is left out (a wrong step); keep_padding: another."""
    G = np.zeros((n_rows, src.shape[1]), dtype=dtype)
    keep = np.ones(idx.size, bool) if keep_padding else idx != padding_idx
    if drop_last_of is not None:
        keep[np.flatnonzero(idx == drop_last_of)[-1]] = False
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
    "sweep_unreplayed" the window sweep (max_lag = SWEEP_LAG) marks rows current without replaying them."""
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
    for t, (idx, src) in enumerate(steps, start=1):
        G = grad_table(idx, src, n_rows, padding_idx, f,
                       drop_last_of=HOT_ROW if (mutant == "run_short" and t == HOT_STEPS[0]) else None,
                       keep_padding=mutant == "padding_kept")
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
