"""Float64 reference of the batch-synchronous SGD step and update-normalised parity metrics — TEST INFRASTRUCTURE ONLY
(tests/ and scripts/stress_parity.py; ``whisprrec_amd`` never imports it).

Why.  ``conftest.rel_err`` is max|a-b| / max|b| on the TABLE.  At the full-size shapes (1M x 1M, B = 65,536, lr = 0.05) one
step moves a row by ~1e-7 of the table's largest element, so a table that was never updated passes a 1e-5 bound, and fp32
rounding alone is 10 % of the update: no metric separates a right kernel from a wrong one there.  The probe run therefore
(a) uses a learning rate proportional to the batch (``probe_lr``), which puts the update at ~1e-2 of the table whatever B is,
and (b) measures the error against the UPDATE, per table (``update_err``) and per row (``row_update_err``), with a float64
reference whose own rounding is invisible at that scale.

Tolerances are derived, not chosen: tests/test_parity_power.py runs the fp32 C oracle (``oracle.bprmf_step_sgd``) at
``probe_lr`` against ``bprmf_sgd_f64`` at the shapes of the GPU tests — "the reference against itself in lower precision" —
and TOL = 8 x the largest such floor, rounded up to one significant digit (8 x: the kernels sum in another order, contract
multiply-adds and use another exp; each is worth a small multiple of one rounding, not an order of magnitude).  The same
test asserts floor x 4 < TOL, TOL_ROW <= 1e-3, and that five wrong steps (never updated, update x 1.01, one row dropped,
one occurrence missing from a shared row's sum, one stale read of a row handed over by the step before) exceed TOL_ROW.

Measured floors (fp32 C oracle against float64 at probe_lr(B); ids, seeds and table scales of the GPU tests they stand for):

    users x items, D, B, steps                                update/table  update_err  row_update_err
    1M x 1M, 64, 65,536, 6 (headline)                         1.5e-2        6.8e-6      1.7e-5
    70K x 200K, 64, 8,192, 7, short last batch                2.4e-2        5.8e-6      1.7e-5
    3K x 2.5K, 64, 256, 7, short last batch                   2.2e-2        4.8e-6      1.4e-5
    40K x 50K, 64, 2,048, 3, rows with 150 / 200 occurrences  6.5e-2        1.3e-6      1.4e-5
    120K x 150K, 64, 8,192, 9, a row with 600 occurrences     3.2e-1        4.2e-6      1.7e-5
    120K x 150K, 64, 8,192, 9, a row with 100 occurrences     1.1e-1        4.7e-6      1.5e-5
  the stratified (rotating item blocks) schedule on its GLOBAL batches, B = the ranks' batches together, at probe_lr(B)
  (tests/test_rotating_power.py):
    6K x 4,002, 64, 2 x 2,048, 24 (2 ranks, 2 parts, 2 epochs)   6.0e-2        4.0e-6      8.3e-6
    6K x 4,003, 64, 3 x 2,048, 36 (3 ranks, 2 parts, 2 epochs)   9.7e-2        5.2e-6      8.9e-6
    6K x 4,004, 64, 4 x 2,048, 72 (4 ranks, 3 parts, 2 epochs)   1.9e-1        2.9e-6      6.1e-6
    6K x 4,002, 64, 2 x 2,048, 12 (2 real ranks, 1 epoch)        4.6e-2        4.4e-6      9.3e-6
    6K x 4,003, 64, 3 x 2,048, 18 (3 real ranks, 1 epoch)        6.5e-2        4.1e-6      9.2e-6
    3K x 2,001, 64, 4,096, 15 (1 rank, 3 sub-epochs)             7.6e-2        3.6e-6      7.4e-6
    40K x 196,610, 64, 2 x 8,192, 8 (2 ranks, chained launch)    3.9e-2        4.8e-6      1.9e-5

    TOL_UPDATE = 8 x 6.8e-6 = 5.4e-5 -> 6e-5          TOL_ROW = 8 x 1.74e-5 = 1.4e-4 -> 2e-4
    (from the first three rows, as test_parity_power asserts; the largest row floor of the whole table, 1.88e-5 on the chained
    launch's shape, gives 8 x 1.88e-5 = 1.5e-4 -> 2e-4 as well, and every row leaves the factor 4)

Hot rows run at the same probe_lr(B).  A row with c occurrences does not move c times as far as a row with one: its
gradient is a sum of c nearly independent rows (~sqrt(c)), and the row with 600 occurrences per batch moves by 0.3 of the
table in nine steps — large, but the floor stays where it is.  Shrinking lr by the occurrence count (ratio 0.015 / c) was
measured as well and is what NOT to do: the rows with one occurrence, which are most rows and decide the per-row metric,
then move by ~1e-5 of the table, a few ulps, and the floor of row_update_err is 4e-3 .. 1e-2 — above the stale read
(5.5e-3) the probe run exists to see.
"""
import numpy as np

GAMMA = float(np.float32(1e-10))            # BPRLoss(gamma=1e-10), as WR_GAMMA in wr_oracle.c

TOL_UPDATE = 6e-5
TOL_ROW = 2e-4
TOL_TABLE = 1e-5                            # the north-star bound on the table and the losses, unchanged


def probe_lr(batch, ratio=0.015):
    """Learning rate of a probe run.  The loss is a batch MEAN, so lr / B is the step per triplet: a row that occurs once
    in the batch moves by (lr / B) * s(1 - s) / (gamma + s) * |other row| ~ 0.5 * (lr / B) of the table.  With lr =
    ratio * B the update of a run of a few steps is ~1e-2 of the table's largest element for every batch size — the regime
    of the small-batch goldens, where fp32 rounding is ~1e-5 of the update instead of ~1e-1 at lr = 0.05, B = 65,536.  lr
    is one scalar argument of the kernels: nothing else about the launch changes."""
    return float(ratio) * int(batch)


def table_err(a, b):
    """conftest.rel_err: max|a - b| / max|b|"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-30)


def touched_rows(u, p, n):
    """sorted ids of the rows a run touches: (user rows, item rows) — the rows of the compact tables"""
    return np.unique(np.asarray(u)), np.unique(np.concatenate([np.asarray(p), np.asarray(n)]))


def _row_sums(idx, vals):
    """sum of vals' rows per distinct idx: (distinct idx, sums), in float64, one pass in sorted order"""
    o = np.argsort(idx, kind="stable")
    s = idx[o]
    starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    return s[starts], np.add.reduceat(vals[o], starts, axis=0)


def bpr_row_grads_f64(U, I, ub, pb, nbk):
    """float64 BPR loss of one batch (the mean over its triplets) and its gradient by row: (user rows, their gradient sums,
    item rows, their gradient sums, loss) — rows outside the batch have zero gradient and are not listed"""
    ue, pe, ne = U[ub], I[pb], I[nbk]
    x = np.einsum("bd,bd->b", ue, pe) - np.einsum("bd,bd->b", ue, ne)
    s = 1.0 / (1.0 + np.exp(-x))
    c = -(s * (1.0 - s) / (GAMMA + s)) / ub.size
    ru, gu = _row_sums(ub, c[:, None] * (pe - ne))
    cu = c[:, None] * ue
    ri, gi = _row_sums(np.concatenate([pb, nbk]), np.concatenate([cu, -cu]))
    return ru, gu, ri, gi, float(np.mean(-np.log(GAMMA + s)))


def bprmf_sgd_f64(U, I, u, p, n, batch, lr, n_steps=None, keep_steps=False, l2=0.0):
    """The reference loop's step (src/helpers/BaseRunner.py:194-200 with BPRMF.py:69-80 and loss.py:38; the semantics of
    oracle.bprmf_step_sgd, l2 = 0): strictly sequential batch-synchronous SGD steps, every gradient of a step from the tables
    before it, a short last batch allowed — in plain NumPy float64.  U, I: the tables the ids index (compact tables of the
    touched rows for the large shapes; rows outside a batch have zero gradient and are not visited).  l2 != 0 (torch.optim.SGD's
    weight_decay): dense, g += l2 * w on EVERY row of the tables handed in, so these must be the whole tables.  Returns (U64,
    I64, losses[n_steps]) and, with keep_steps, a fourth value: the list of (U64, I64) copies after every step."""
    U, I = np.array(U, dtype=np.float64), np.array(I, dtype=np.float64)
    u, p, n = (np.asarray(a, dtype=np.int64) for a in (u, p, n))
    batch = int(batch)
    nb = (u.size + batch - 1) // batch if n_steps is None else int(n_steps)
    lr, l2 = float(np.float32(lr)), float(np.float32(l2))      # the kernels and the C oracle take lr and l2 as floats
    losses, kept = np.zeros(nb, np.float64), []
    for k in range(nb):
        ub, pb, nbk = u[k * batch:(k + 1) * batch], p[k * batch:(k + 1) * batch], n[k * batch:(k + 1) * batch]
        ru, gu, ri, gi, losses[k] = bpr_row_grads_f64(U, I, ub, pb, nbk)
        if l2 != 0.0:                                # w -= lr * (g + l2 * w), the decay from the tables before the step
            decay_u, decay_i = (lr * l2) * U, (lr * l2) * I
        U[ru] -= lr * gu
        I[ri] -= lr * gi
        if l2 != 0.0:
            U -= decay_u
            I -= decay_i
        if keep_steps:
            kept.append((U.copy(), I.copy()))
    return (U, I, losses, kept) if keep_steps else (U, I, losses)


def _row_inf(a):
    return np.max(np.abs(a), axis=1)


def update_err(got, ref64, before):
    """max|got - ref| / max|ref - before|: the error as a fraction of the largest update"""
    got, ref64, before = (np.asarray(a, dtype=np.float64) for a in (got, ref64, before))
    return float(np.max(np.abs(got - ref64))) / max(float(np.max(np.abs(ref64 - before))), 1e-300)


def row_update_err(got, ref64, before, return_row=False):
    """max over rows of |got - ref|_inf / max(|ref - before|_inf of that row, median of that quantity over the rows the run
    moved).  The floor under the denominator keeps a row whose update happens to be tiny from deciding the test; rows the
    reference leaves alone do not enter the median, so whole tables and tables of the touched rows give the same figure."""
    got, ref64, before = (np.asarray(a, dtype=np.float64) for a in (got, ref64, before))
    upd = _row_inf(ref64 - before)
    moved = upd > 0
    ratio = _row_inf(got - ref64) / np.maximum(upd, float(np.median(upd[moved])) if moved.any() else 1e-300)
    worst = int(np.argmax(ratio))
    return (float(ratio[worst]), worst) if return_row else float(ratio[worst])


def sgd_run_errors(U0, I0, ref, got_U, got_I):
    """the figures of one run against its float64 reference ref = (U64, I64, ...): a dict"""
    eu, wu = row_update_err(got_U, ref[0], U0, return_row=True)
    ei, wi = row_update_err(got_I, ref[1], I0, return_row=True)
    return {"update_err": max(update_err(got_U, ref[0], U0), update_err(got_I, ref[1], I0)),
            "row_update_err": max(eu, ei), "worst": ("user", wu) if eu >= ei else ("item", wi),
            "table_err": max(table_err(got_U, ref[0]), table_err(got_I, ref[1])),
            "update_over_table": max(float(np.max(np.abs(ref[0] - U0))) / max(float(np.max(np.abs(ref[0]))), 1e-30),
                                     float(np.max(np.abs(ref[1] - I0))) / max(float(np.max(np.abs(ref[1]))), 1e-30))}


def take_rows(tab, rows):
    """tab[rows] as a NumPy array; tab: a NumPy array or a torch tensor on any device"""
    if isinstance(tab, np.ndarray):
        return tab[rows]
    import torch
    return tab[torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(tab.device)].cpu().numpy()


def check_sgd_run(tag, U0, I0, u, p, n, batch, lr, got_U, got_I, got_losses, rows=None, n_steps=None,
                  tol_update=TOL_UPDATE, tol_row=TOL_ROW, per_step=None):
    """One probe run against the float64 reference, with the four assertions every SGD parity test makes:
    update_err < tol_update, row_update_err < tol_row, table_err < 1e-5 and losses within 1e-5 of the float64 losses.

    U0, I0: the tables before the run; got_U, got_I: after it — whole tables (NumPy arrays or torch tensors; the rows the run
    touches are taken out here, the others are not this check's business), or, with rows = (user ids, item ids) as from
    touched_rows, tables already restricted to those rows.  Prints the figures once (pytest -s / -rP).  On a failure the
    message names the worst row (global id, user or item, its occurrences per step) and, when per_step is given — a
    callable k -> (got_U, got_I) after k steps run as one-step calls, in the layout of got_U / got_I — the first step at which
    the per-step comparison leaves the tolerance.  Returns the figures."""
    u, p, n = (np.asarray(a.cpu() if hasattr(a, "cpu") else a, dtype=np.int64) for a in (u, p, n))
    batch = int(batch)
    whole = rows is None
    rows_u, rows_i = touched_rows(u, p, n) if whole else rows
    cut = (lambda U, I: (take_rows(U, rows_u), take_rows(I, rows_i))) if whole else (lambda U, I: (np.asarray(U), np.asarray(I)))
    cu, cp, cn = np.searchsorted(rows_u, u), np.searchsorted(rows_i, p), np.searchsorted(rows_i, n)
    (U0, I0), (got_U, got_I) = cut(U0, I0), cut(got_U, got_I)
    if hasattr(got_losses, "cpu"):
        got_losses = got_losses.cpu().numpy()
    assert got_U.shape == U0.shape == (rows_u.size, U0.shape[1]) and got_I.shape == I0.shape == (rows_i.size, I0.shape[1])
    ref = bprmf_sgd_f64(U0, I0, cu, cp, cn, batch, lr, n_steps, keep_steps=per_step is not None)
    fig = sgd_run_errors(U0, I0, ref, got_U, got_I)
    fig["loss_err"] = table_err(np.asarray(got_losses, dtype=np.float64).reshape(-1), ref[2])
    print("parity %s: lr %.4g update/table %.1e | update_err %.2e (tol %.0e) row_update_err %.2e (tol %.0e) table_err %.2e "
          "loss_err %.2e" % (tag, lr, fig["update_over_table"], fig["update_err"], tol_update, fig["row_update_err"], tol_row,
                             fig["table_err"], fig["loss_err"]), flush=True)
    ok = (fig["update_err"] < tol_update and fig["row_update_err"] < tol_row and fig["table_err"] < TOL_TABLE
          and fig["loss_err"] < TOL_TABLE)
    if not ok:
        kind, row = fig["worst"]
        nb = ref[2].size
        cols = (cu,) if kind == "user" else (cp, cn)
        occ = [sum(int(np.sum(c[k * batch:(k + 1) * batch] == row)) for c in cols) for k in range(nb)]
        msg = "%s: %s; worst row: %s %d, occurrences per step %s" % (
            tag, {k: v for k, v in fig.items() if k != "worst"}, kind, int((rows_u if kind == "user" else rows_i)[row]), occ)
        if per_step is not None:
            first, before = None, (U0, I0)
            for k in range(1, nb + 1):
                gU, gI = cut(*per_step(k))
                e = sgd_run_errors(before[0], before[1], ref[3][k - 1], gU, gI)
                if not (e["update_err"] < tol_update and e["row_update_err"] < tol_row):
                    first = (k, e["update_err"], e["row_update_err"], e["worst"])
                    break
                before = ref[3][k - 1]
            msg += "; first step outside the tolerance (one-step calls): %s" % (first,)
        raise AssertionError(msg)
    return fig
