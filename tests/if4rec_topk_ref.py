"""Float64 NumPy restatement of the top-K of a multi-interest model (K23): a row's score against an item is the maximum over
its interests (IF4Rec.py:117-118), the row's masked items are left out, the rest is sorted by score descending, then item id
ascending (the reference's save_rec_results over full_predict, src/main.py:83-102), and cut at k; a row with fewer than k items
left ends with -1 / -inf.  No GPU, no library: tests/test_if4rec_topk_contract.py checks that the wrong variants below change
the lists, tests/test_hip_if4rec_topk.py checks the kernels against this file.

A case is the dict of tests/if4rec_ref.make_rank_case: queries [n, KQ, D], items [n_items, D], mask_ptr / mask_idx (CSR lists),
mask_row [n] (the list of row e; None or absent: no mask)."""
import numpy as np

GAP = 1e-4               # a row is judged when its reference scores at positions 1..k+1 lie at least this far apart
WRONG_TOPK = ("sum_over_k", "mean_over_k", "interest_0_only", "mask_of_own_row_number")


def scores_ref(c, variant=None):
    """float64 [n, n_items] scores with the masked items at -inf, and [n, n_items] the first interest that attains each score"""
    q, it = c["queries"].astype(np.float64), c["items"].astype(np.float64)
    n = q.shape[0]
    per = np.einsum("ekd,jd->ekj", q, it)
    if variant == "sum_over_k":
        S = per.sum(axis=1)
    elif variant == "mean_over_k":
        S = per.mean(axis=1)
    elif variant == "interest_0_only":
        S = per[:, 0, :].copy()
    else:
        S = per.max(axis=1)
    win = per.argmax(axis=1)                            # the first on ties
    if c.get("mask_row") is not None:
        n_lists = len(c["mask_ptr"]) - 1
        for e in range(n):
            r = e % n_lists if variant == "mask_of_own_row_number" else c["mask_row"][e]
            S[e, c["mask_idx"][c["mask_ptr"][r]:c["mask_ptr"][r + 1]]] = -np.inf
    return S, win


def topk_ref(c, k, variant=None):
    """-> items int64 [n, k] (-1 at padding), scores float64 [n, k] (-inf at padding), interest int64 [n, k] (-1 at padding),
    judged bool [n]: the row's scores at positions 1..k+1 lie at least GAP apart (its list does not hang on fp32 rounding)"""
    S, win = scores_ref(c, variant)
    n, n_items = S.shape
    order = np.argsort(-S, axis=1, kind="stable")
    kk = min(k + 1, n_items)
    top = np.take_along_axis(S, order[:, :kk], axis=1)
    if kk > 1:
        gaps = -np.diff(np.where(np.isfinite(top), top, -1e30), axis=1)
        judged = gaps.min(axis=1) >= GAP
    else:
        judged = np.ones(n, bool)
    order = order[:, :k]
    sc = np.take_along_axis(S, order, axis=1)
    fin = np.isfinite(sc)
    items = np.where(fin, order, -1)
    interest = np.where(fin, np.take_along_axis(win, order, axis=1), -1)
    if k > n_items:
        pad = k - n_items
        items = np.concatenate([items, -np.ones((n, pad), np.int64)], axis=1)
        interest = np.concatenate([interest, -np.ones((n, pad), np.int64)], axis=1)
        sc = np.concatenate([sc, np.full((n, pad), -np.inf)], axis=1)
    return items.astype(np.int64), sc, interest.astype(np.int64), judged
