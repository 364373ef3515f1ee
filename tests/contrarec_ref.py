"""Float64 NumPy restatements for the ContraRec tests: the transformer block with a KEY-LENGTH mask (K13's _keys entry points;
BERT4RecEncoder, reference src/models/sequential/ContraRec.py:216-233) and the supervised contrastive loss with its closed-form
gradient (K15; ContraLoss, :141-204), plus the shapes, figures and tolerances of those tests.  A helper module, not a conftest.

The block is sasblock_ref.block_f64's algebra (its LayerNorm helpers and figures are imported) with one change: query i of
sequence b keeps key j iff j < key_len[b], for every i in 0..T-1 — padded queries are ordinary queries.

The loss, as the reference writes it (N = 2B rows, z = normalised rows, label of row r = labels[r mod B]):
    s = z z^T / tau,  m_i = max_j s_ij,  l_ij = s_ij - 2 m_i,  E_i = sum_{j != i} exp(l_ij),  P_i = {j != i: same label}
    loss = weight / N * sum_i (-tau / (|P_i| + 1e-10)) sum_{j in P_i} (l_ij - log(E_i + 1e-10))
and the gradient with m_i held constant:
    G_ij = (-tau / N) ([j in P_i] / c_i - (|P_i| / c_i) exp(l_ij) / (E_i + 1e-10)),  gz = weight (G + G^T) z / tau,
    gF_i = (gz_i - <gz_i, z_i> z_i) / |F_i|

Figures: max |a - b| / max |b|; the loss relatively.  Tolerances by DESIGN section 2's rule: the floor of a figure is the stock
fp32 torch path against the restatement on a CPU, over the shapes below; TOL = 8 x the largest floor, rounded up to one digit.
tests/test_contrarec_contract.py re-measures the floors and asserts 4 x floor < TOL.  BLOCK_WALK_SHAPES / BLOCK_FORM_SHAPES
(sasblock_ref's walk and form lists through the _keys entry points, with and without dropout) carry floors and tolerances of their own.
"""
import numpy as np

import sasblock_ref as R
from sasblock_ref import PARAMS, _ln_bwd, _ln_fwd, figures, fmt, group_of, rel_err, worst  # noqa: F401

# ------------------------------------------------------------------------------------------------ shapes and tolerances
# (B, T, D, heads); the first is g12's batch with the state of encoder.transformer_block.0
BLOCK_SHAPES = [(96, 20, 64, 2), (3, 1, 64, 2), (5, 7, 32, 2), (2, 33, 64, 2), (130, 64, 64, 1), (37, 20, 32, 4)]
# (B, D, tau, distinct labels); a quarter of the rows are identical in both views.  The last three give every column chunk of the
# kernel two tiles and the last chunk one full tile and a ragged one (the second tile, the buffer swap): 2B rows above 2048 at
# D <= 64, above 1448 at D = 128
LOSS_SHAPES = [(3, 32, 0.2, 2), (64, 64, 0.2, 10), (65, 64, 0.2, 20), (200, 32, 0.05, 30), (256, 64, 0.2, 40), (64, 128, 0.05, 500),
               (1140, 64, 0.2, 100), (760, 128, 0.05, 500), (1130, 32, 0.2, 60)]

# Largest floor of each figure over the shapes: stock fp32 torch (sasrec._Block with the [B, 1, 1, T] mask; contrarec.contra_loss
# over F.normalize) against float64, on a CPU.
BLOCK_FLOORS = {"out": 3.0e-7, "gx": 2.8e-7, "gqk": 1.2e-6, "gparam": 8.8e-7, "gkb": 6.1e-6}
BLOCK_TOL = {"out": 3e-6, "gx": 3e-6, "gqk": 1e-5, "gparam": 8e-6, "gkb": 5e-5}        # 8 x floor, rounded up to one digit
# Several visits per workgroup and the <D, TM> forms at their border: sasblock_ref's two lists, through the _keys entry points, at
# p = 0 and p = 0.1.  Floors measured as BLOCK_FLOORS is (tests/test_contrarec_contract.py prints them).
BLOCK_WALK_SHAPES, BLOCK_FORM_SHAPES = R.WALK_SHAPES, R.FORM_SHAPES
BLOCK_WALK_SEED, BLOCK_FORM_SEED = 17300, 27300           # make_block_case's seed bases of the two lists (BLOCK_SHAPES: 7300)
# WALK: gqk and gkb peak at (515, 20, 64, 4) p = 0, gparam at (515, 33, 32, 2) p = 0.1.  FORM: gx at (4, 64, 32, 1) p = 0.
BLOCK_WALK_FLOORS = {"out": 2.71e-7, "gx": 2.60e-7, "gqk": 2.79e-6, "gparam": 1.71e-6, "gkb": 1.11e-5}
BLOCK_FORM_FLOORS = {"out": 2.26e-7, "gx": 4.10e-7, "gqk": 1.59e-6, "gparam": 5.90e-7, "gkb": 7.69e-6}
# 8 x floor, rounded up to one digit (sasblock_ref.rule_of); BLOCK_TOL's own value where the rule lands on it
BLOCK_WALK_TOL = {"out": BLOCK_TOL["out"], "gx": BLOCK_TOL["gx"], "gqk": 3e-5, "gparam": 2e-5, "gkb": 9e-5}
BLOCK_FORM_TOL = {"out": 2e-6, "gx": 4e-6, "gqk": 2e-5, "gparam": 5e-6, "gkb": 7e-5}
# The wrong results of a walk (tests/test_contrarec_contract.py), smallest largest-figure / BLOCK_WALK_TOL over the walk shapes at
# p = 0.1: later_visits_dropped 5.7e3, later_visits_stale 2.9e5, mask_of_first_visit 1.6e5, length_of_first_visit 1.2e5;
# max_of_first_visit misses the stored maximum (13.14 at x[2049] x 100) by 13.13.
LOSS_FLOORS = {"loss": 1.5e-7, "gF": 8.3e-7}
LOSS_TOL = {"loss": 2e-6, "gF": 7e-6}

BLOCK_WRONG = ["causal", "pad_keys_attended", "pad_queries_skipped"]
LOSS_WRONG = ["single_shift", "no_eps", "diag_in_denominator", "labels_ignored", "no_transpose_term", "no_projection"]


# ------------------------------------------------------------------------------------------------ inputs
def make_lengths(B, T, rng):
    """random lengths in [1, T] with 1 and T forced in (as far as B allows)"""
    n = rng.randint(1, T + 1, size=B).astype(np.int64)
    n[0] = T
    if B > 1:
        n[1] = 1
    return n


def make_block_case(i, g12=None, shapes=None, seed=7300):
    """-> (x [B, T, D] fp32, params, upstream gradient, heads, key_len int64 [B]) of BLOCK_SHAPES[i]; case 0 needs g12.
    shapes / seed: another list (BLOCK_WALK_SHAPES, BLOCK_FORM_SHAPES) with its own seed base.  One draw gives every length, so
    the lengths of the sequences b >= 512 are independent of those of b - 512."""
    B, T, D, heads = (BLOCK_SHAPES if shapes is None else shapes)[i]
    rng = np.random.RandomState(seed + i)
    if i == 0 and shapes is None:
        pre = "sd__encoder.transformer_block.0."
        sd = {n: np.asarray(g12[pre + n], np.float32) for n in PARAMS}
        lengths = np.asarray(g12["lengths"], np.int64)
        pos = np.arange(T)[None, :] * (np.arange(T)[None, :] < lengths[:, None])
        x = (g12["sd__item_embeddings.weight"][g12["hist"]] + g12["sd__encoder.p_embeddings.weight"][pos]).astype(np.float32)
    else:
        sd = R.xavier_params(D, heads, rng)
        x = (rng.standard_normal((B, T, D)) * np.sqrt(2.0 / (3706 + D)) * np.sqrt(2.0)).astype(np.float32)
        lengths = make_lengths(B, T, rng)
    rp = np.random.RandomState(seed + 100 + i)   # parameters away from their initial 0 / 1: every gradient path carries weight
    for n in PARAMS:
        if n.endswith("bias"):
            sd[n] = (sd[n] + 0.05 * rp.standard_normal(sd[n].shape)).astype(np.float32)
        elif "layer_norm" in n:
            sd[n] = (sd[n] + 0.1 * rp.standard_normal(sd[n].shape)).astype(np.float32)
    g = rng.standard_normal((B, T, D)).astype(np.float32)
    return x, sd, g, heads, lengths


def make_loss_case(i):
    """-> (F [2B, D] fp32, labels int64 [B], tau) of LOSS_SHAPES[i]: encoder-like rows (not unit length), labels with many
    duplicates, a quarter of the rows identical in both views"""
    B, D, tau, n_lab = LOSS_SHAPES[i]
    rng = np.random.RandomState(7500 + i)
    F = (rng.standard_normal((2 * B, D)) * (0.5 + rng.rand(2 * B, 1))).astype(np.float32)
    same = rng.permutation(B)[:max(B // 4, 1)]
    F[B + same] = F[same]
    labels = rng.randint(1, n_lab + 1, size=B).astype(np.int64)
    return F, labels, tau


# ------------------------------------------------------------------------------------------------ the block in float64
def block_keys_f64(x, sd, heads, key_len, gout=None, wrong=None, m1=None, m2=None, first=None):
    """-> dict(out and, with gout, gx and g[name] for every parameter).  `wrong` builds deliberately WRONG blocks: 'causal' (the
    SASRec mask), 'pad_keys_attended' (no mask at all), 'pad_queries_skipped' (queries at padded positions get no attention),
    'later_visits_dropped' (only the sequences b < first enter the parameter-gradient sums).
    m1 / m2: multiplicative dropout masks (keep * scale) of sasblock_ref.masks_for, or None."""
    f = np.float64
    x = np.asarray(x, f)
    W = {n: np.asarray(sd[n], f) for n in PARAMS}
    pq, pk, pv = (["masked_attn_head.%s_linear.%s" % (c, s) for s in ("weight", "bias")] for c in "qkv")
    B, T, D = x.shape
    dk = D // heads
    key_len = np.asarray(key_len, np.int64)
    one = np.ones((), f)
    m1 = one if m1 is None else np.asarray(m1, f)
    m2 = one if m2 is None else np.asarray(m2, f)

    def split(z):
        return z.reshape(B, T, heads, dk).transpose(0, 2, 1, 3)

    def merge(z):
        return z.transpose(0, 2, 1, 3).reshape(B, T, D)

    q, k, v = (split(x @ W[w].T + W[b]) for w, b in (pq, pk, pv))
    sc = 1.0 / np.sqrt(f(dk))
    S = np.einsum("bhid,bhjd->bhij", q, k) * sc
    keep = np.broadcast_to((np.arange(T)[None, :] < key_len[:, None])[:, None, None, :], S.shape)      # [B, 1, 1, T]
    if wrong == "causal":
        keep = np.broadcast_to(np.tril(np.ones((T, T), bool))[None, None], S.shape)
    elif wrong == "pad_keys_attended":
        keep = np.ones(S.shape, bool)
    S = np.where(keep, S, -np.inf)
    gmax = S.max()
    with np.errstate(under="ignore"):
        E = np.exp(S - gmax)
    if wrong == "pad_queries_skipped":
        E = np.where((np.arange(T)[None, :] < key_len[:, None])[:, None, :, None], E, 0.0)
    Z = E.sum(-1, keepdims=True)
    zero = Z == 0
    P = np.where(zero, 0.0, E / np.where(zero, 1.0, Z))
    A = merge(P @ v)
    C, xh1, rstd1 = _ln_fwd(A * m1 + x, W["layer_norm1.weight"], W["layer_norm1.bias"], R.LN_EPS)
    pre = C @ W["linear1.weight"].T + W["linear1.bias"]
    H = np.maximum(pre, 0.0)
    O2 = H @ W["linear2.weight"].T + W["linear2.bias"]
    out, xh2, rstd2 = _ln_fwd(O2 * m2 + C, W["layer_norm2.weight"], W["layer_norm2.bias"], R.LN_EPS)
    res = {"out": out, "gmax": float(gmax), "seq_max": S.max((1, 2, 3))}
    if gout is None:
        return res
    G = np.asarray(gout, f)
    g = {}
    n_sum = B if wrong != "later_visits_dropped" else first

    def wsum(a, b):
        return np.einsum("btj,btd->jd", a[:n_sum], b[:n_sum])

    def bsum(a):
        return a[:n_sum].sum((0, 1))

    g["layer_norm2.weight"], g["layer_norm2.bias"] = bsum(G * xh2), bsum(G)
    dY2 = _ln_bwd(G, xh2, rstd2, W["layer_norm2.weight"])
    dO2 = dY2 * m2
    g["linear2.weight"], g["linear2.bias"] = wsum(dO2, H), bsum(dO2)
    dpre = (dO2 @ W["linear2.weight"]) * (pre > 0)
    g["linear1.weight"], g["linear1.bias"] = wsum(dpre, C), bsum(dpre)
    dC = dY2 + dpre @ W["linear1.weight"]
    g["layer_norm1.weight"], g["layer_norm1.bias"] = bsum(dC * xh1), bsum(dC)
    dY1 = _ln_bwd(dC, xh1, rstd1, W["layer_norm1.weight"])
    dA = split(dY1 * m1)
    dP = np.einsum("bhid,bhjd->bhij", dA, v)
    dS = P * (dP - (P * dP).sum(-1, keepdims=True))
    dq = merge(dS @ k) * sc
    dkk = merge(dS.transpose(0, 1, 3, 2) @ q) * sc
    dv = merge(P.transpose(0, 1, 3, 2) @ dA)
    gx = dY1.copy()
    for (w, b), d in ((pq, dq), (pk, dkk), (pv, dv)):
        g[w], g[b] = wsum(d, x), bsum(d)
        gx += d @ W[w]
    res["gx"], res["g"] = gx, g
    return res


def stock_block_fp32(x, sd, heads, gout, key_len, device="cpu", dtype=None, m1=None, m2=None):
    """the stock `_Block` under torch.autograd with BERT4RecEncoder's [B, 1, 1, T] mask -> (out, gx, {name: grad});
    m1 / m2: explicit dropout masks in place of its two dropout layers"""
    import torch
    from whisprrec_amd.sasrec import _Block
    dtype = dtype or torch.float32
    B, T, D = x.shape
    blk = _Block(D, D, heads, 0.0).to(dtype)
    blk.load_state_dict({n: torch.as_tensor(sd[n]).to(dtype) for n in PARAMS})
    blk = blk.to(device)
    if m1 is not None:
        class _Mul(torch.nn.Module):
            def __init__(self, m):
                super().__init__()
                self.m = torch.as_tensor(np.asarray(m), dtype=dtype, device=device)

            def forward(self, a):
                return a * self.m

        blk.dropout1, blk.dropout2 = _Mul(m1), _Mul(m2)
    xt = torch.as_tensor(x, dtype=dtype, device=device).clone().requires_grad_(True)
    lens = torch.as_tensor(np.asarray(key_len), device=device)
    mask = (torch.arange(T, device=device)[None, :] < lens[:, None]).view(B, 1, 1, T)
    out = blk(xt, mask)
    out.backward(torch.as_tensor(gout, dtype=dtype, device=device))
    return (out.detach().cpu().numpy(), xt.grad.cpu().numpy(), {n: p.grad.cpu().numpy() for n, p in blk.named_parameters()})


def block_fmt(tag, fig, tol=None):
    w, tol = worst(fig), BLOCK_TOL if tol is None else tol
    return "parity sasblock_keys %s: " % tag + " ".join("%s %.2e (tol %.0e)" % (k, w[k], tol[k]) for k in R.GROUPS)


# ------------------------------------------------------------------------------------------------ the loss in float64
def supcon_f64(F, labels, tau, weight=1.0, wrong=None):
    """-> (loss, gF [2B, D]) in float64.  `wrong` builds deliberately WRONG losses: 'single_shift' (the row maximum subtracted
    once), 'no_eps' (neither + 1e-10), 'diag_in_denominator' (E_i includes j = i), 'labels_ignored' (only the other view of the
    same row is a positive), 'no_transpose_term' (gz = G z / tau), 'no_projection' (gF_i = gz_i / |F_i|)."""
    f = np.float64
    F = np.asarray(F, f)
    N, B = F.shape[0], F.shape[0] // 2
    lab = np.arange(B) if wrong == "labels_ignored" else np.asarray(labels).reshape(-1)
    lab = np.concatenate([lab, lab])
    nrm = np.sqrt((F * F).sum(1, keepdims=True))
    den = np.maximum(nrm, 1e-12)
    z = F / den
    s = (z @ z.T) / tau
    m = s.max(1, keepdims=True)
    l = s - (1.0 if wrong == "single_shift" else 2.0) * m
    eye = np.eye(N, dtype=bool)
    off = np.ones((N, N), bool) if wrong == "diag_in_denominator" else ~eye
    eps = 0.0 if wrong == "no_eps" else 1e-10
    pos = (lab[:, None] == lab[None, :]) & ~eye
    with np.errstate(under="ignore"):
        ex = np.exp(l) * off
    E = ex.sum(1, keepdims=True)
    cnt = pos.sum(1, keepdims=True).astype(f)
    c = cnt + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        inner = np.where(pos, l - np.log(E + eps), 0.0).sum(1, keepdims=True)
        per_row = np.where(cnt > 0, -tau / np.where(c > 0, c, 1.0) * inner, 0.0)
        loss = weight * per_row.sum() / N
        G = (-tau / N) * (np.where(cnt > 0, pos / np.where(c > 0, c, 1.0), 0.0)
                          - np.where(cnt > 0, cnt / np.where(c > 0, c, 1.0), 0.0) * ex / (E + eps))
    G = np.where(eye, 0.0, G) if wrong != "diag_in_denominator" else G * ~eye
    M = G if wrong == "no_transpose_term" else G + G.T
    gz = weight * (M @ z) / tau
    clamped = nrm < 1e-12
    proj = 0.0 if wrong == "no_projection" else (gz * z).sum(1, keepdims=True) * z
    gF = np.where(clamped, gz / 1e-12, (gz - proj) / den)
    return float(loss), gF


def stock_loss_fp32(F, labels, tau, dtype=None, device="cpu"):
    """the torch path of the model: contra_loss over F.normalize of the stacked views, under autograd -> (loss, gF)"""
    import torch
    from whisprrec_amd.contrarec import contra_loss
    dtype = dtype or torch.float32
    Ft = torch.as_tensor(F, dtype=dtype, device=device).clone().requires_grad_(True)
    B = Ft.shape[0] // 2
    feats = torch.nn.functional.normalize(torch.stack([Ft[:B], Ft[B:]], dim=1), dim=-1)
    loss = contra_loss(feats, torch.as_tensor(np.asarray(labels), device=device), tau)
    loss.backward()
    return float(loss.detach()), Ft.grad.cpu().numpy()


def loss_figures(loss, gF, ref):
    return {"loss": abs(loss - ref[0]) / abs(ref[0]), "gF": rel_err(gF, ref[1])}


def loss_fmt(tag, fig):
    return "parity supcon %s: " % tag + " ".join("%s %.2e (tol %.0e)" % (k, fig[k], LOSS_TOL[k]) for k in ("loss", "gF"))
