"""Float64 restatement of one side of SGL's calc_ssl_loss (reference src/models/general/SGL.py:213-220) with its gradients,
the four comparison figures of the InfoNCE tests, and their tolerances.  A helper module, not a conftest.

    q_b = A[idx_b] / max(|A[idx_b]|, eps)      k_j = Bm[j] / max(|Bm[j]|, eps)          (F.normalize, eps = 1e-12)
    loss = weight * sum_b ( log sum_j exp(<q_b, k_j> / tau) - <q_b, k_idx_b> / tau )

Why four figures: the rows of gB named by the batch carry the -q / tau term and are 10 to 5,000 times larger than the
rows outside the batch, so a max-norm over the whole table cannot see an error in the out-of-batch rows.  `gB_out` is
normalised by the out-of-batch rows' own maximum.

Tolerances: DESIGN section 2's rule, TOL = 8 x the largest floor, rounded up to one digit, where the floor is the stock fp32
torch formula (with torch.autograd) against this restatement on the same inputs — the reference against itself in lower
precision.  FLOORS holds the largest floor of each figure over SHAPES, with and without a quarter of the batch on one row,
measured on a CPU; tests/test_infonce_contract.py re-measures them and asserts 4 x floor < TOL.
"""
import numpy as np

EPS = 1e-12

# (rows, batch, D, tau) of the GPU parity test
SHAPES = [(3706, 512, 64, 0.1), (6040, 480, 64, 0.2), (100003, 1024, 64, 0.1), (50000, 256, 32, 0.05), (20000, 512, 128, 0.2)]

# Largest floor over the ten cases.  The large ones come from the case (50,000 rows, B 256, tau 0.05) with 64 positions on one
# row: at that temperature the positive's softmax weight is 0.994, and the row's gradient sum_b (p_b - 1) q_b / tau cancels
# to 1/170 of its terms — in any fp32 evaluation, the reference's included.
FLOORS = {"loss": 2.4e-7, "gA": 4.0e-6, "gB_in": 2.6e-5, "gB_out": 4.0e-6}
TOL = {"loss": 2e-6, "gA": 4e-5, "gB_in": 3e-4, "gB_out": 4e-5}       # 8 x floor, rounded up to one digit


def make_case(n, B, D, seed, dup=False, scale=0.1):
    """tables like propagated embeddings (rows of very different length) and a batch; dup: a quarter of it names one row"""
    rng = np.random.RandomState(seed)
    A = (rng.standard_normal((n, D)) * scale * rng.uniform(0.2, 2.0, (n, 1))).astype(np.float32)
    Bm = (A * 0.7 + rng.standard_normal((n, D)) * scale * 0.5).astype(np.float32)        # the two views correlate
    idx = rng.randint(0, n, B).astype(np.int64)
    if dup:
        idx[rng.permutation(B)[:B // 4]] = idx[0]
    return A, Bm, idx


def _normalize(x):
    nrm = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return x / np.maximum(nrm, EPS), nrm


def _normalize_bwd(g, y, nrm, project=True):
    """d/dx of y = x / max(|x|, eps): (g - y <y, g>) / |x|, and g / eps on the clamped branch (|x| < eps)"""
    proj = (g - y * (y * g).sum(axis=1, keepdims=True)) if project else g
    return np.where(nrm < EPS, g / EPS, proj / np.maximum(nrm, EPS))


def infonce_f64(A, Bm, idx, tau, weight=1.0, *, positive=True, project=True, drop_last=0, block=256):
    """-> (loss, gA [n, D], gB [n, D]) in float64.  The keyword switches build deliberately WRONG results for the power
    checks: positive=False drops the positive term, project=False the projection of the normalisation backward,
    drop_last=m leaves the last m rows of Bm out of sum_j exp."""
    A, Bm = np.asarray(A, np.float64), np.asarray(Bm, np.float64)
    idx = np.asarray(idx, np.int64)
    n, B = A.shape[0], idx.size
    K, nB = _normalize(Bm)
    Q, nA = _normalize(A[idx])
    Kp = K[idx]
    wt = weight / tau
    loss = 0.0
    gq = np.empty_like(Q)
    gK = np.zeros_like(K)
    for lo in range(0, B, block):
        hi = min(B, lo + block)
        S = Q[lo:hi] @ K.T / tau
        if drop_last:
            S[:, n - drop_last:] = -np.inf
        m = S.max(axis=1, keepdims=True)
        E = np.exp(S - m)
        Z = E.sum(axis=1, keepdims=True)
        loss += float((np.log(Z) + m).sum())
        P = E / Z
        gq[lo:hi] = wt * (P @ K)
        gK += wt * (P.T @ Q[lo:hi])
    if positive:
        loss -= float((Q * Kp).sum() / tau)
        gq -= wt * Kp
        np.subtract.at(gK, idx, wt * Q)
    gA = np.zeros_like(A)
    np.add.at(gA, idx, _normalize_bwd(gq, Q, nA, project))
    gB = _normalize_bwd(gK, K, nB, project)
    return weight * loss, gA, gB


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def figures(got, ref, idx, skip_rows=()):
    """the four figures of (loss, gA, gB) against the reference triple; skip_rows are left out of the table figures"""
    (l, gA, gB), (rl, rgA, rgB) = got, ref
    n = rgA.shape[0]
    inb = np.zeros(n, bool)
    inb[np.asarray(idx)] = True
    keep = np.ones(n, bool)
    keep[list(skip_rows)] = False
    gA, gB = np.asarray(gA, np.float64), np.asarray(gB, np.float64)
    assert not np.any(gA[~inb]), "gA must be zero outside the batch rows"
    return {"loss": abs(float(l) - rl) / abs(rl),
            "gA": rel_err(gA[inb & keep], rgA[inb & keep]),
            "gB_in": rel_err(gB[inb & keep], rgB[inb & keep]),
            "gB_out": rel_err(gB[~inb & keep], rgB[~inb & keep])}


def stock_fp32(A, Bm, idx, tau, weight=1.0, device="cpu"):
    """the reference's formula as written (SGL.py:213-220) in fp32 torch with torch.autograd — what --ssl_native 0 runs"""
    import torch
    import torch.nn.functional as F
    A = torch.as_tensor(A, dtype=torch.float32, device=device).clone().requires_grad_(True)
    Bm = torch.as_tensor(Bm, dtype=torch.float32, device=device).clone().requires_grad_(True)
    idx = torch.as_tensor(idx, dtype=torch.int64, device=device)
    e1 = F.normalize(A[idx], dim=1)
    e2 = F.normalize(Bm[idx], dim=1)
    all2 = F.normalize(Bm, dim=1)
    v1 = torch.exp(torch.sum(e1 * e2, dim=1) / tau)
    v2 = torch.sum(torch.exp(e1.matmul(all2.T) / tau), dim=1)
    loss = -torch.sum(torch.log(v1 / v2)) * weight
    gA, gB = torch.autograd.grad(loss, [A, Bm])
    return float(loss.detach()), gA.cpu().numpy(), gB.cpu().numpy()


def fmt(tag, fig):
    return "parity %s: " % tag + " ".join("%s %.2e" % (k, fig[k]) for k in ("loss", "gA", "gB_in", "gB_out"))
