"""Float64 restatement of the full-catalogue softmax loss of --train_loss softmax (whisprrec_amd/softmax_loss.py) with its
gradients, the four comparison figures of the softmax-loss tests, and their tolerances.  A helper module, not a conftest.

    s_bj = <Q[b], E[j]>      loss = weight * sum_b ( log sum_{j >= first_class} exp(s_bj) - s_b,target_b )

Why four figures (the reason tests/infonce_ref.py gives): the rows of gE named by a target carry the -Q[b] term and are orders of
magnitude larger than the other rows, so a max-norm over the whole table cannot see an error in the rows no target names.
`gE_out` is normalised by those rows' own maximum.

Tolerances: DESIGN section 2's rule, TOL = 8 x the largest floor, rounded up to one digit, where the floor is the stock fp32
torch lines (matmul, logits[:, 0] = -inf, F.cross_entropy, with torch.autograd) against this restatement on the same inputs — the
feature's definition against itself in lower precision.  FLOORS holds the largest floor of each figure over SHAPES x VARIANTS,
measured on a CPU; tests/test_softmax_loss_contract.py re-measures them and asserts 4 x floor < TOL <= 16 x FLOORS.
"""
import numpy as np

# (n_items, B, D) of the GPU parity test: the smallest shapes at which the split of the K26 passes can still go wrong (128
# resident rows per workgroup, streamed tiles of 64 rows — 32 at D = 128 — and a split that aims at 1024 workgroups)
SHAPES = [(3706, 200, 64),      # one-tile chunks, ragged last tile, B below two resident blocks
          (20000, 520, 64),     # several tiles per chunk in both passes, ragged tails on both sides
          (5000, 130, 32),
          (4099, 257, 128),
          (70, 1, 64)]          # a single query, two tiles
VARIANTS = ("random", "dup", "large")      # random targets; a quarter of the batch on one target; max |s| > 150
LARGE_SCORE = 160.0

# Largest floor over the fifteen cases.  The gradient floors come from the large-score variant: there the softmax is close to a
# one-hot row, p - [j == target] cancels for a row whose target holds the maximum, and what is left is the rounding of the fp32
# scores themselves (|s| ~ 160, ulp 1.5e-5) — in any fp32 evaluation, the stock lines included.
FLOORS = {"loss": 1.5e-7, "gQ": 7.8e-6, "gE_in": 4.7e-6, "gE_out": 4.0e-6}
TOL = {"loss": 2e-6, "gQ": 7e-5, "gE_in": 4e-5, "gE_out": 4e-5}            # 8 x floor, rounded up to one digit
FIGURES = ("loss", "gQ", "gE_in", "gE_out")


def make_case(n, B, D, seed, variant="random"):
    """an item table like a trained one (rows of very different length, a padding row 0 that is NOT zero: xavier overwrites it),
    queries like layer-norm outputs, targets in [1, n) -> (Q [B, D], E [n, D], target [B])"""
    assert variant in VARIANTS
    rng = np.random.RandomState(seed)
    E = (rng.standard_normal((n, D)) * 0.1 * rng.uniform(0.2, 2.0, (n, 1))).astype(np.float32)
    E[0] *= 4.0
    Q = rng.standard_normal((B, D)).astype(np.float32)
    target = rng.randint(1, n, B).astype(np.int64)
    if variant == "dup":
        target[rng.permutation(B)[:max(B // 4, 1)]] = target[0]
    if variant == "large":
        top = np.abs(Q.astype(np.float64) @ E[1:].astype(np.float64).T).max()
        Q = (Q * (LARGE_SCORE / top)).astype(np.float32)
    return Q, E, target


def softmax_ce_f64(Q, E, target, first_class=1, weight=None, *, keep_excluded=False, target_term=True, drop_last=0,
                   out_scale=1.0, miss_one_dup=False, block=256):
    """-> (loss, gQ [B, D], gE [n, D]) in float64; weight None = 1 / B.  The keyword switches build deliberately WRONG results
    for the power checks: keep_excluded leaves the columns below first_class in the softmax, target_term=False drops the target
    term, drop_last=m leaves the last m items out of the softmax, out_scale scales the rows of gE no target names,
    miss_one_dup leaves one occurrence of the most repeated target out of its row of gE."""
    Q, E = np.asarray(Q, np.float64), np.asarray(E, np.float64)
    target = np.asarray(target, np.int64)
    n, B = E.shape[0], Q.shape[0]
    w = 1.0 / B if weight is None else float(weight)
    loss = 0.0
    gQ = np.empty_like(Q)
    gE = np.zeros_like(E)
    for lo in range(0, B, block):
        hi = min(B, lo + block)
        S = Q[lo:hi] @ E.T
        if not keep_excluded:
            S[:, :first_class] = -np.inf
        if drop_last:
            S[:, n - drop_last:] = -np.inf
        m = S.max(axis=1, keepdims=True)
        X = np.exp(S - m)
        Z = X.sum(axis=1, keepdims=True)
        loss += float((np.log(Z) + m).sum())
        P = X / Z
        gQ[lo:hi] = w * (P @ E)
        gE += w * (P.T @ Q[lo:hi])
    named = np.zeros(n, bool)
    named[target] = True
    gE[~named] *= out_scale
    if target_term:
        loss -= float((Q * E[target]).sum())
        gQ -= w * E[target]
        keep = np.ones(B, bool)
        if miss_one_dup:
            ids, counts = np.unique(target, return_counts=True)
            assert counts.max() > 1, "miss_one_dup needs a repeated target"
            keep[np.flatnonzero(target == ids[counts.argmax()])[-1]] = False
        np.subtract.at(gE, target[keep], w * Q[keep])
    return w * loss, gQ, gE


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def figures(got, ref, target):
    """the four figures of (loss, gQ, gE) against the reference triple"""
    (l, gQ, gE), (rl, rgQ, rgE) = got, ref
    named = np.zeros(rgE.shape[0], bool)
    named[np.asarray(target)] = True
    gE = np.asarray(gE, np.float64)
    return {"loss": abs(float(l) - rl) / abs(rl),
            "gQ": rel_err(gQ, rgQ),
            "gE_in": rel_err(gE[named], rgE[named]),
            "gE_out": rel_err(gE[~named], rgE[~named])}


def stock_lines(user_e, weight, pos_item, first_class=1):
    """the three stock lines of --softmax_native 0 on torch tensors of any dtype and device, under autograd"""
    import torch.nn.functional as F
    logits = user_e @ weight.t()
    logits[:, :first_class] = -float("inf")
    return F.cross_entropy(logits, pos_item)


def stock_fp32(Q, E, target, first_class=1, device="cpu"):
    """stock_lines in fp32 torch with torch.autograd -> (loss, gQ, gE) as numpy"""
    import torch
    Q = torch.as_tensor(Q, dtype=torch.float32, device=device).clone().requires_grad_(True)
    E = torch.as_tensor(E, dtype=torch.float32, device=device).clone().requires_grad_(True)
    target = torch.as_tensor(target, dtype=torch.int64, device=device)
    loss = stock_lines(Q, E, target, first_class)
    gQ, gE = torch.autograd.grad(loss, [Q, E])
    return float(loss.detach()), gQ.cpu().numpy(), gE.cpu().numpy()


def cases():
    """(tag, shape index, variant, seed) of every parity case"""
    return [("%dx%dx%d-%s" % (SHAPES[i] + (v,)), i, v, 100 + 10 * i + k) for i in range(len(SHAPES)) for k, v in enumerate(VARIANTS)]


def measure_floors():
    """largest stock-fp32-against-float64 figure over cases(), on the CPU"""
    worst = dict.fromkeys(FIGURES, 0.0)
    for _, i, v, seed in cases():
        Q, E, t = make_case(*SHAPES[i], seed, v)
        fig = figures(stock_fp32(Q, E, t), softmax_ce_f64(Q, E, t), t)
        for k in FIGURES:
            worst[k] = max(worst[k], fig[k])
    return worst


def fmt(tag, fig):
    return "parity %s: " % tag + " ".join("%s %.2e (tol %.0e)" % (k, fig[k], TOL[k]) for k in FIGURES)
