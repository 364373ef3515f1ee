"""Float64 reference of LightGCN's loss that keeps its two terms apart, the inputs of the tests built on it and their derived
tolerances — TEST INFRASTRUCTURE ONLY (tests/ and tests/golden/make_golden.py; ``whisprrec_amd`` never imports it).

Why.  loss = mean BPR + reg_weight * EmbLoss, EmbLoss = (|U0[u]|_F + |I0[p]|_F + |I0[n]|_F) / B on the ego rows (reference
src/utils/loss.py:94-98, src/models/general/LightGCN.py:169-175).  At the reference's default reg_weight (1e-5) the whole
term is worth 2e-6 of the gradient on the g4 golden and 1.5e-5 on an ml-1m-shaped batch, and every test that reached the
kernels of the term (wr_rows.hip: lightgcn_tail_*, embloss_sumsq / finish / grad) asked for conftest.rel_err < 1e-5: a kernel
that adds nothing, or half the right thing, passed.  So (a) the term is tested on its own (tests/test_hip_embloss.py), (b) the
whole step runs at a reg_weight where the term is 0.3 .. 0.8 of the gradient (``reg_weight_for_share``; the g11 golden and the
synthetic cases of tests/test_lightgcn.py), and (c) errors are measured per row (``row_err``) against a float64 reference whose
own rounding is invisible at that scale.

Tolerances are derived as in oracle/parity.py: tests/test_lightgcn_power.py compares an fp32 restatement with the float64
reference on the exact inputs of the GPU cases (the C oracle for the whole step; NumPy fp32 for the isolated term: sums of
squares in fp32, rob / sqrt, count * coef * row, one multiply-add into the buffer) and each TOL is 8 x the largest floor,
rounded up to one significant digit (the 8: see parity.py).  The same test asserts 4 x floor < TOL for every case, that seven
wrong versions of the term are rejected with a factor 5 to spare, and that the old bound at reg_weight 1e-5 accepts them all.

Measured floors, largest over the cases (fp32 restatement against float64):

    quantity; cases                                                                            floor     8 x       TOL
    three sums of squares, relative (np.sum in fp32); the 34 embloss cases                     1.55e-7   1.24e-6   2e-6
    reg_weight * EmbLoss taken as loss(rw) - loss(0), relative to the term; the same           2.47e-7   1.98e-6   2e-6
    EmbLoss gradient per row; the same                                                         3.18e-7   2.54e-6   3e-6
      (into zeros: users 2.22e-7, items 1.74e-7; into a non-zero buffer of the term's own size: 3.18e-7, 2.29e-7)
    whole gradient per row, C oracle; STEP_CASES and g4's inputs at g11's reg_weight           3.56e-7   2.85e-6   3e-6
      (16,1,64,8) 2.7e-7  (20,3,100,32) 1.9e-7  (32,2,257,8) 1.8e-7  (128,2,256,64) 1.9e-7  (8,2,33,8) 3.6e-7
      (96,2,192,32) 1.9e-7  (16,2,64,4) 2.0e-7  g4 at reg_weight 4.2: 1.3e-7
    the same cases under the project's own bounds, which stay at 1e-5: conftest.rel_err of the gradient 1.25e-7, loss 1.27e-7;
    loss at reg_weight 0 of the embloss cases against the float64 BPR mean 8.6e-8 (parity.TOL_TABLE)
"""
import functools

import numpy as np

from .parity import GAMMA, _row_sums

TOL_SQ = 2e-6           # the three sums of squares, relative
TOL_REG_LOSS = 2e-6     # loss(rw) - loss(0) against rw * EmbLoss, relative to the term
TOL_REG_ROW = 3e-6      # the isolated EmbLoss gradient, per row (row_err)
TOL_LGCN_ROW = 3e-6     # the whole LightGCN gradient, per row (row_err)

SHARE = (0.3, 0.8)      # max|g_reg| / max|g_bpr + g_reg| of a run in which the term counts


# ------------------------------------------------------------------------------------------------ the reference, float64
def bpr_terms_f64(x):
    """-log(GAMMA + sigmoid(x)) and its derivative in x, per triplet (reference src/utils/loss.py:38)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
    return -np.log(GAMMA + s), -(s * (1.0 - s) / (GAMMA + s))


def spmm_f64(row_ptr, col, val, X, block=1 << 18):
    """CSR product A @ X in float64: row sums with np.add.reduceat over slabs of ~block non-zeros; empty rows stay zero"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    col, val, X = np.asarray(col, dtype=np.int64), np.asarray(val, dtype=np.float64), np.asarray(X, dtype=np.float64)
    Y = np.zeros_like(X)
    n_rows, r0 = rp.size - 1, 0
    while r0 < n_rows:
        r1 = max(r0 + 1, int(np.searchsorted(rp, rp[r0] + block, side="right")) - 1)
        r1 = min(r1, n_rows)
        lo, hi = int(rp[r0]), int(rp[r1])
        if hi > lo:
            starts = rp[r0:r1] - lo
            full = np.flatnonzero(rp[r0 + 1:r1 + 1] > rp[r0:r1])
            Y[r0 + full] = np.add.reduceat(val[lo:hi, None] * X[col[lo:hi]], starts[full], axis=0)
        r0 = r1
    return Y


def propagate_f64(row_ptr, col, val, X, L):
    """mean over l = 0..L of A^l X (LightGCN.py:134-143)"""
    X = np.asarray(X, dtype=np.float64)
    acc, cur = X.copy(), X
    for _ in range(int(L)):
        cur = spmm_f64(row_ptr, col, val, cur)
        acc += cur
    return acc / (int(L) + 1)


def embloss_terms_f64(U0, I0, u, p, n, reg_weight):
    """-> (reg_loss, sq3, gU, gI): EmbLoss of the batch (un-weighted), the three sums of squares, and the gradient of
    reg_weight * EmbLoss as whole tables.  Closed form: every occurrence of row r in block k adds reg_weight / (B |block_k|_F) *
    row; a block of zero norm adds nothing (torch.norm's backward gives zero there)."""
    U0, I0 = np.asarray(U0, dtype=np.float64), np.asarray(I0, dtype=np.float64)
    u, p, n = (np.asarray(a, dtype=np.int64) for a in (u, p, n))
    B, rw = u.size, float(np.float32(reg_weight))               # the kernels and the C oracle take reg_weight as a float
    blocks = ((U0, u), (I0, p), (I0, n))
    sq3 = np.array([np.sum(tab[idx] ** 2) for tab, idx in blocks])
    nrm = np.sqrt(sq3)
    gU, gI = np.zeros_like(U0), np.zeros_like(I0)
    for (tab, idx), g, nk in zip(blocks, (gU, gI, gI), nrm):
        if nk > 0:
            np.add.at(g, idx, (rw / (B * nk)) * tab[idx])
    return float(nrm.sum() / B), sq3, gU, gI


def lightgcn_terms_f64(n_users, n_items, row_ptr, col, val, E0, L, reg_weight, u, p, n):
    """-> (bpr_loss, reg_loss, g_bpr, g_reg); loss = bpr_loss + reg_weight * reg_loss, gradient = g_bpr + g_reg, both
    [n_users + n_items, D].  g_bpr: the BPR gradient on the propagated rows taken back through the mean of layers (the
    adjacency is symmetric); g_reg: embloss_terms_f64 on the ego rows."""
    E0 = np.asarray(E0, dtype=np.float64)
    u, p, n = (np.asarray(a, dtype=np.int64) for a in (u, p, n))
    nU, B = int(n_users), u.size
    allE = propagate_f64(row_ptr, col, val, E0, L)
    ue, pe, ne = allE[u], allE[nU + p], allE[nU + n]
    term, c = bpr_terms_f64(np.einsum("bd,bd->b", ue, pe) - np.einsum("bd,bd->b", ue, ne))
    c = c / B
    gout = np.zeros_like(E0)
    ru, gu = _row_sums(u, c[:, None] * (pe - ne))
    cu = c[:, None] * ue
    ri, gi = _row_sums(np.concatenate([p, n]), np.concatenate([cu, -cu]))
    gout[ru] = gu
    gout[nU + ri] = gi
    reg_loss, _, gU, gI = embloss_terms_f64(E0[:nU], E0[nU:], u, p, n, reg_weight)
    return float(np.mean(term)), reg_loss, propagate_f64(row_ptr, col, val, gout, L), np.concatenate([gU, gI])


def reg_share(g_bpr, g_reg):
    return float(np.max(np.abs(g_reg))) / max(float(np.max(np.abs(g_bpr + g_reg))), 1e-300)


def reg_weight_for_share(g_bpr, g_reg_at_1, target=0.5):
    """a reg_weight of two significant digits at which max|g_reg| / max|g_bpr + g_reg| is about `target` (bisection on
    log reg_weight: the share grows from 0 to 1 with it); the caller asserts SHARE on what it gets"""
    lo, hi = -12.0, 12.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if reg_share(g_bpr, 10.0 ** mid * g_reg_at_1) < target:
            lo = mid
        else:
            hi = mid
    return float(np.float32(float("%.1e" % 10.0 ** hi)))


# ------------------------------------------------------------------------------------------------ metrics
def _row_inf(a):
    return np.max(np.abs(a), axis=1)


def row_err(got, ref64, scale=None, return_row=False):
    """max over rows of |got - ref|_inf / max(|scale|_inf of that row, median of it over the rows where scale is non-zero);
    scale = ref unless given (a term added into a non-zero buffer G0: got against G0 + term, scale = the term).  The floor
    under the denominator keeps a row that happens to be tiny from deciding the test (parity.row_update_err)."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    size = _row_inf(ref64 if scale is None else np.asarray(scale, dtype=np.float64))
    live = size > 0
    ratio = _row_inf(got - ref64) / np.maximum(size, float(np.median(size[live])) if live.any() else 1e-300)
    worst = int(np.argmax(ratio))
    return (float(ratio[worst]), worst) if return_row else float(ratio[worst])


def describe_row(kind, row, u, p, n, sq3=None):
    """what a failing assertion says about its worst row: occurrences as user / positive / negative, and the block norms its
    EmbLoss coefficient is made of"""
    u, p, n = (np.asarray(a, dtype=np.int64) for a in (u, p, n))
    if kind == "user":
        txt = "user row %d: %d occurrences, norm of block 0 (users)" % (row, int(np.sum(u == row)))
    else:
        cp, cn = int(np.sum(p == row)), int(np.sum(n == row))
        used = [k for k, c in ((1, cp), (2, cn)) if c]
        txt = "item row %d: %d as positive, %d as negative, norm(s) of block(s) %s (1 positives, 2 negatives)" % (row, cp, cn, used)
    if sq3 is not None:
        txt += "; block norms %s" % np.sqrt(np.asarray(sq3, dtype=np.float64)).tolist()
    return txt


def check_rows(tag, got_U, got_I, ref_U, ref_I, tol, u, p, n, scale_U=None, scale_I=None, sq3=None):
    """row_err of both tables below tol; prints the figures (pytest -s / -rP), names the worst row on a failure"""
    eu, wu = row_err(got_U, ref_U, scale_U, return_row=True)
    ei, wi = row_err(got_I, ref_I, scale_I, return_row=True)
    print("%s: row_err users %.2e items %.2e (tol %.0e)" % (tag, eu, ei, tol), flush=True)
    if not (eu < tol and ei < tol):
        kind, row = ("user", wu) if eu / tol >= ei / tol else ("item", wi)
        raise AssertionError("%s: row_err users %.3e items %.3e, tol %.0e; worst %s" % (
            tag, eu, ei, tol, describe_row(kind, row, u, p, n, sq3)))
    return eu, ei


# ------------------------------------------------------------------------------------------------ inputs of the GPU cases
def _skewed_batch(rng, B, n_users, n_items, pos_pool, neg_pool, hot_user, shared_item):
    """one batch in which the term's bookkeeping has something to get wrong: hot_user takes ~30 %, shared_item is m1 times a
    positive and m2 != m1 times a negative, positives come from pos_pool (rows scaled x4 by the callers) and negatives from
    neg_pool, row 0 and the last row of both tables occur; shuffled.  Batches of fewer than 15 keep what fits."""
    u = rng.randint(0, n_users, B).astype(np.int64)
    p = rng.choice(pos_pool[pos_pool != shared_item], B).astype(np.int64)
    n = rng.choice(neg_pool[neg_pool != shared_item], B).astype(np.int64)
    m1 = m2 = 0
    if B >= 15:
        h, m1, m2 = int(round(0.3 * B)), max(3, B // 10), max(2, B // 20)
        u[:h] = hot_user
        u[h], u[h + 1] = 0, n_users - 1
        p[:m1] = shared_item
        n[m1:m1 + m2] = shared_item
    else:
        u[0] = 0 if B == 1 else n_users - 1
    p[-1], n[-1] = n_items - 1, 0
    o = rng.permutation(B)
    return u[o], p[o], n[o], (m1, m2)


EMBLOSS_USERS, EMBLOSS_ITEMS = 300, 400
# (D, B): every branch of WR_DISPATCH_D up to 256 (20, 96, 200: the masked ones) meets a B that is no multiple of its teams
# per workgroup (256 / T: D = 4 -> 256, 8 -> 128, 16 -> 64, 32 -> 32, the others 16), and every B occurs
EMBLOSS_CASES = ((4, 1), (4, 255), (4, 257), (8, 15), (8, 257), (8, 2048), (16, 17), (16, 255), (20, 1), (20, 15), (20, 17),
                 (20, 257), (32, 17), (32, 255), (32, 2048), (64, 1), (64, 15), (64, 257), (64, 2048), (96, 17), (96, 255),
                 (128, 15), (128, 257), (200, 17), (200, 255), (200, 2048), (256, 1), (256, 17), (256, 257))
EMBLOSS_SPECIAL = (("zero_users", 64, 257), ("zero_users", 20, 17), ("saturated", 64, 257), ("saturated", 96, 255),
                   ("saturated", 8, 2048))


@functools.lru_cache(maxsize=None)
def embloss_case(D, B, kind="plain"):
    """Inputs of one case of tests/test_hip_embloss.py, as a dict.  U0, I0: ego tables (300 x D, 400 x D; items 200.. scaled
    x4, so the positives' norm is > 2 x the negatives'); Ua, Ia: other tables standing for the propagated ones;  u, p, n: an
    epoch of two batches of batch_size > B whose last, short batch (k = 1, length B) is the one under test — ub, pb, nb.
    kind "zero_users": every user row of U0 is zero; "saturated": Ua scaled so that scores lie beyond +-40 on both sides.
    reg_weight: makes the term a third of the loss.  G0u, G0i: non-zero buffers of the size of the term's own rows."""
    nU, nI = EMBLOSS_USERS, EMBLOSS_ITEMS
    rng = np.random.RandomState(100003 * D + 7 * B + {"plain": 0, "zero_users": 1, "saturated": 2}[kind])
    U0, I0, Ua, Ia = ((rng.standard_normal((r, D)) * 0.2).astype(np.float32) for r in (nU, nI, nU, nI))
    I0[200:] *= np.float32(4.0)
    if kind == "zero_users":
        U0[:] = 0
    if kind == "saturated":
        Ua *= np.float32(400.0 / np.sqrt(D))
    batch_size = B + B // 4 + 3
    pos_pool, neg_pool = np.arange(200, nI), np.arange(0, 200)
    u0, p0, n0 = (rng.randint(0, r, batch_size).astype(np.int64) for r in (nU, nI, nI))
    ub, pb, nb, (m1, m2) = _skewed_batch(rng, B, nU, nI, pos_pool, neg_pool, hot_user=7, shared_item=250)
    x = np.einsum("bd,bd->b", Ua[ub].astype(np.float64), Ia[pb].astype(np.float64) - Ia[nb].astype(np.float64))
    bpr = float(np.mean(bpr_terms_f64(x)[0]))
    reg_loss, sq3, _, _ = embloss_terms_f64(U0, I0, ub, pb, nb, 1.0)
    rw = float(np.float32(float("%.1e" % (0.5 * bpr / reg_loss))))
    _, _, gU, gI = embloss_terms_f64(U0, I0, ub, pb, nb, rw)
    size = np.concatenate([_row_inf(gU), _row_inf(gI)])
    med = float(np.median(size[size > 0]))
    G0u, G0i = ((rng.standard_normal((r, D)) * med).astype(np.float32) for r in (nU, nI))
    return dict(D=D, B=B, kind=kind, U0=U0, I0=I0, Ua=Ua, Ia=Ia, batch_size=batch_size, u=np.concatenate([u0, ub]),
                p=np.concatenate([p0, pb]), n=np.concatenate([n0, nb]), ub=ub, pb=pb, nb=nb, m=(m1, m2), reg_weight=rw,
                x=x, bpr_loss=bpr, reg_loss=reg_loss, sq3=sq3, gU=gU, gI=gI, G0u=G0u, G0i=G0i)


STEP_USERS, STEP_ITEMS = 300, 200
# (D, L, B, max_nnz of a chunk); the last one cuts user 0's row (200 non-zeros) into 50 chunks: two combine levels
STEP_CASES = ((16, 1, 64, 8), (20, 3, 100, 32), (32, 2, 257, 8), (128, 2, 256, 64), (8, 2, 33, 8), (96, 2, 192, 32),
              (16, 2, 64, 4))


@functools.lru_cache(maxsize=None)
def step_graph():
    """(clicked_ptr, clicked_idx) of a 300 x 200 graph: user 0 linked to every item, user 5 isolated, a power-law rest"""
    nU, nI = STEP_USERS, STEP_ITEMS
    rng = np.random.RandomState(11)
    w = 1.0 / (np.arange(nI) + 3.0) ** 0.9
    w = rng.permutation(w / w.sum())
    ptr, idx = [0], []
    for uu in range(nU):
        if uu == 0:
            items = np.arange(nI)
        elif uu == 5:
            items = np.zeros(0, np.int64)
        else:
            k = int(min(1 + rng.pareto(1.1) * 3, 80))
            items = np.sort(rng.choice(nI, size=k, replace=False, p=w))
        idx += items.tolist()
        ptr.append(len(idx))
    return np.asarray(ptr, dtype=np.int32), np.asarray(idx, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def step_case(D, L, B, max_nnz):
    """Inputs and float64 reference of one whole-step case of tests/test_lightgcn.py, as a dict: the CSR adjacency (row_ptr,
    col, val from oracle.lightgcn_build_adj), E0 (items 100.. scaled x4), one skewed batch, reg_weight by the share rule, and
    bpr_loss, reg_loss, g_bpr, g_reg at that reg_weight."""
    import oracle
    nU, nI = STEP_USERS, STEP_ITEMS
    ptr, idx = step_graph()
    rp, col, val = oracle.lightgcn_build_adj(nU, nI, ptr, idx)
    rng = np.random.RandomState(7919 * D + 31 * B + L)
    E0 = (rng.standard_normal((nU + nI, D)) * 0.1).astype(np.float32)
    E0[nU + 100:] *= np.float32(4.0)
    u, p, n, m = _skewed_batch(rng, B, nU, nI, np.arange(100, nI), np.arange(0, 100), hot_user=9, shared_item=150)
    u[np.flatnonzero(u != 9)[0]] = 5                                     # the isolated user is in the batch
    _, _, g_bpr, g1 = lightgcn_terms_f64(nU, nI, rp, col, val, E0, L, 1.0, u, p, n)
    rw = reg_weight_for_share(g_bpr, g1)
    bpr, reg, g_bpr, g_reg = lightgcn_terms_f64(nU, nI, rp, col, val, E0, L, rw, u, p, n)
    return dict(D=D, L=L, B=B, max_nnz=max_nnz, n_users=nU, n_items=nI, row_ptr=rp, col=col, val=val, E0=E0, u=u, p=p, n=n,
                m=m, reg_weight=rw, bpr_loss=bpr, reg_loss=reg, g_bpr=g_bpr, g_reg=g_reg, share=reg_share(g_bpr, g_reg))


def g4_csr(g4):
    """CSR (row_ptr, col, val) of the adjacency the reference built for g4 (stored there as its non-zeros in row order)"""
    N = g4["U0"].shape[0] + g4["I0"].shape[0]
    row = np.asarray(g4["adj_row"], dtype=np.int64)
    assert np.all(np.diff(row) >= 0)
    rp = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=N), out=rp[1:])
    return rp, np.asarray(g4["adj_col"], dtype=np.int32), np.asarray(g4["adj_val"], dtype=np.float32)


def g4_terms_f64(g4, reg_weight):
    """lightgcn_terms_f64 on g4's graph, tables and batch"""
    nU, nI = g4["U0"].shape[0], g4["I0"].shape[0]
    rp, col, val = g4_csr(g4)
    return lightgcn_terms_f64(nU, nI, rp, col, val, np.concatenate([g4["U0"], g4["I0"]]), int(g4["hp"][0]), reg_weight,
                              g4["u"], g4["p"], g4["n"])
