"""Float64 NumPy restatements for IF4Rec's kernels: the interest pooling (K18, IF4Rec.py:87-103) with its gradients, and the
ranks of a multi-interest model (K19, :117-118) with their margins; the case list, the figures, the floors and tolerances, and the
wrong variants the figures must be able to see.  No GPU, no library: tests/test_if4rec_contract.py checks this file against the
reference formula under autograd, tests/test_hip_if4rec.py checks the kernels against this file.

Tolerances (DESIGN.md section 2's rule).  FLOORS[k] is the largest figure k of the STOCK fp32 torch path — the reference's own
operations, global-maximum shift included — against float64 on a CPU over CASES (all-zero rows left out: autograd gives them
NaN); TOL = 8 x the largest floor, rounded up to one digit.  tests/test_if4rec_contract.py re-measures the floors and asserts
4 x floor < TOL.  WALK_CASES (B above the kernels' workgroup caps: a workgroup visits several sequences) has WALK_FLOORS /
WALK_TOL of its own, by the same rule.
"""
import numpy as np

LEAKY = 0.01

# (B, T, D, A, K)
CASES = [(96, 20, 64, 8, 2), (3, 1, 64, 8, 2), (5, 7, 32, 8, 1), (2, 33, 64, 8, 4), (130, 64, 64, 8, 2), (37, 20, 128, 16, 3),
         (1, 20, 64, 8, 8)]
SPREAD_CASE = 4        # W2 scaled: the scores of this case span about +-60 across its sequences
N_ITEMS = 211

FIGURES = ("out", "g_hp", "g_item", "g_pos", "gW1", "gb1", "gW2", "gb2")

# measured by tests/test_if4rec_contract.py::test_floors_and_tolerance (stock fp32 torch on a CPU against float64)
FLOORS = {"out": 7.40e-7, "g_hp": 9.33e-7, "g_item": 5.78e-7, "g_pos": 4.58e-7, "gW1": 9.94e-7, "gb1": 4.23e-7, "gW2": 5.46e-7,
          "gb2": 2.44e-7}
TOL = 8e-6             # 8 x 9.94e-7 = 7.95e-6, rounded up to one digit

# The caps of wr_if4rec.hip restated: a workgroup takes the sequences b, b + cap, b + 2 cap, ... once B exceeds the cap.
FWD_WG = 4096          # kIpFwdWg: workgroups of the forward
BWD_WG = 512           # kIpBwdWg: workgroups of the backward, which carry the partials of gW1, gb1, gW2, gb2 and g_pos across visits

# Cases at which a workgroup visits several sequences (backward: 2 - 3 visits, the last one ragged; (4099, 2, 64, 8, 1) walks the
# forward too and gives the backward 8 - 9 visits).  make_case's row kinds, and among the later visits a row of length 1 (row
# BWD_WG + 1) and all-zero rows (the last row and, where that is another one, row BWD_WG + 2).
WALK_CASES = [(1027, 5, 32, 8, 2), (4099, 2, 64, 8, 1), (1030, 3, 128, 16, 3), (515, 20, 64, 8, 4)]
WALK_SEED = 11400      # make_case's seed base of this list (CASES: 1400)
# measured by tests/test_if4rec_contract.py::test_walk_floors_and_tolerance, as FLOORS is
# (one thread; all-zero rows left out).  g_pos and gW2 peak at (4099, 2, 64, 8, 1): sums over 4,099 sequences of K = 1, T = 2.
WALK_FLOORS = {"out": 1.89e-7, "g_hp": 2.16e-7, "g_item": 3.72e-7, "g_pos": 1.80e-6, "gW1": 4.21e-7, "gb1": 2.37e-7, "gW2": 1.67e-6,
               "gb2": 3.03e-7}
WALK_TOL = 2e-5        # 8 x 1.80e-6 = 1.44e-5, rounded up to one digit
# The wrong results of a walk (walk_wrong below), smallest largest-figure / WALK_TOL over WALK_CASES: later_visits_dropped 7.8e3,
# later_visits_stale 3.8e4, length_of_first_visit 4.9e4.


# The model on the reference's batch (g14): the loss and every gradient are held to TOL, except the gradients that arrive through
# the attention scores of the blocks (q_linear, k_linear).  Over K = 2 interest tokens those are sums that cancel almost entirely
# (max |g| ~ 2e-6 against ~1e-2 elsewhere; the k bias is zero on paper and is measured on the scale of the k weight), and the
# STOCK fp32 path itself misses TOL on them: MODEL_QK_FLOOR is its largest such figure against float64 on a CPU, 8 and 4 heads
# (tests/test_if4rec_contract.py::test_model_floors re-measures it); MODEL_QK_TOL = 8 x floor, rounded up to one digit.
SCORE_PATH = ("masked_attn_head.q_linear.weight", "masked_attn_head.q_linear.bias", "masked_attn_head.k_linear.weight",
              "masked_attn_head.k_linear.bias")
MODEL_QK_FLOOR = 1.25e-4
MODEL_QK_TOL = 1e-3    # 8 x 1.25e-4 = 1.0e-3
KB, KW = "masked_attn_head.k_linear.bias", "masked_attn_head.k_linear.weight"


def model_grad_figures(got, ref):
    """{parameter: max |got - ref| / max |scale|} over a model's gradients; the gradients that are zero on paper (k_linear.bias,
    W2.bias) on the scale of their weight's gradient"""
    fig = {}
    for n, r in ref.items():
        scale = ref[n.replace(KB, KW)] if n.endswith(KB) else ref["W2.weight"] if n == "W2.bias" else r
        fig[n] = figure(got[n], r, scale)
    return fig


def model_tol(name):
    return MODEL_QK_TOL if name.endswith(SCORE_PATH) else TOL


def make_case(i, cases=None, seed=1400):
    """inputs of case i as float32 / int64 arrays.  Every case with B >= 3 holds a row of length 1 (row 0), a full row (row 1),
    an all-zero row (the last) and, when B >= 4 and T >= 3, a row with an interior zero (row 2).
    cases / seed: another list (WALK_CASES) with its own seed base; its cases also hold a row of length 1 and an all-zero row
    among the sequences a workgroup of the backward meets on a later visit."""
    B, T, D, A, K = (CASES if cases is None else cases)[i]
    rng = np.random.RandomState(seed + i)
    item = (rng.standard_normal((N_ITEMS, D)) * 0.5).astype(np.float32)
    pos = (rng.standard_normal((T + 1, D)) * 0.5).astype(np.float32)
    W1 = (rng.standard_normal((A, D)) / np.sqrt(D)).astype(np.float32)
    b1 = (rng.standard_normal(A) * 0.1).astype(np.float32)
    W2 = (rng.standard_normal((K, A)) / np.sqrt(A)).astype(np.float32)
    b2 = (rng.standard_normal(K) * 0.1).astype(np.float32)
    lengths = rng.randint(1, T + 1, size=B).astype(np.int64)
    if B >= 3:
        lengths[0], lengths[1] = 1, T
    hist = np.zeros((B, T), np.int64)
    for r in range(B):
        hist[r, :lengths[r]] = rng.randint(1, N_ITEMS, size=lengths[r])
    if B >= 4 and T >= 3:
        lengths[2] = max(lengths[2], 3)
        hist[2, :lengths[2]] = rng.randint(1, N_ITEMS, size=lengths[2])
        hist[2, 1] = 0
    if B >= 3:
        hist[B - 1] = 0
    if cases is not None:
        lengths[BWD_WG + 1] = 1
        hist[BWD_WG + 1, 1:] = 0
        if BWD_WG + 2 < B - 1:
            hist[BWD_WG + 2] = 0
    if i == SPREAD_CASE and cases is None:
        c = dict(item=item, pos=pos, hist=hist, W1=W1, b1=b1, W2=W2, b2=b2)
        s = pool_ref(c)["s"]
        W2 = (W2 * (60.0 / np.abs(s[np.isfinite(s)]).max())).astype(np.float32)
        b2 = np.zeros_like(b2)
    g_out = rng.standard_normal((B, K, D)).astype(np.float32)
    return dict(item=item, pos=pos, hist=hist, lengths=lengths, W1=W1, b1=b1, W2=W2, b2=b2, g_out=g_out)


def drop_zero_rows(c):
    """the case without its all-zero rows (autograd passes NaN through them)"""
    keep = (c["hist"] > 0).any(axis=1)
    out = dict(c)
    for k in ("hist", "lengths", "g_out"):
        out[k] = c[k][keep]
    return out


def pool_ref(c, variant=None, g_out=None, valid=None):
    """float64 pooling of case dict c and, with g_out, every gradient.  variant: one of WRONG_POOL (a deliberately wrong
    formula), or None.  valid: bool [B, T], a history mask other than hist > 0 (walk_wrong's 'length_of_first_visit' only)."""
    f = np.float64
    item, pos, W1, b1, W2, b2 = (c[k].astype(f) for k in ("item", "pos", "W1", "b1", "W2", "b2"))
    hist = c["hist"]
    B, T = hist.shape
    valid = hist > 0 if valid is None else np.asarray(valid, bool)
    if variant == "mask_by_lengths":
        valid = np.arange(T)[None, :] < c["lengths"][:, None]
    pidx = np.arange(T)[None, :] * valid
    hp = item[hist] + (0.0 if variant == "no_position" else pos[pidx])
    h = hp @ W1.T + b1
    act = np.where(h > 0, h, 0.0 if variant == "relu" else LEAKY * h)
    s = np.transpose(act @ W2.T + b2, (0, 2, 1))                     # [B, K, T]
    s = np.where(valid[:, None, :], s, -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        if variant == "softmax_over_k":
            e = np.exp(s - s.max(axis=1, keepdims=True))
            p = e / e.sum(axis=1, keepdims=True)
        else:
            e = np.exp(s - s.max())                                  # the reference's shift by the global maximum
            p = e / e.sum(axis=2, keepdims=True)
    if variant != "zero_row_nan":
        p = np.where(np.isnan(p), 0.0, p)
    out = np.einsum("bkt,btd->bkd", p, hp)
    res = dict(out=out, s=s, p=p)
    if g_out is None:
        return res
    g = g_out.astype(f)
    dp = np.einsum("bkd,btd->bkt", g, hp)
    ds = p * (dp - (p * dp).sum(axis=2, keepdims=True))
    g_hp = np.einsum("bkt,bkd->btd", p, g)
    dh = np.einsum("bkt,ka->bta", ds, W2) * np.where(h > 0, 1.0, LEAKY)
    g_hp = (g_hp + dh @ W1) * valid[:, :, None]
    g_item = np.zeros_like(item)
    np.add.at(g_item, hist.reshape(-1), g_hp.reshape(B * T, -1))
    g_pos = np.zeros_like(pos)
    np.add.at(g_pos, pidx.reshape(-1), g_hp.reshape(B * T, -1))
    res.update(g_hp=g_hp, g_item=g_item, g_pos=g_pos, gW1=np.einsum("bta,btd->ad", dh, hp), gb1=dh.sum(axis=(0, 1)),
               gW2=np.einsum("bkt,bta->ka", ds, act), gb2=ds.sum(axis=(0, 2)))
    return res


WRONG_POOL = ("mask_by_lengths", "relu", "softmax_over_k", "no_position", "zero_row_nan")


# ------------------------------------------------------------------------------------------------ several visits per workgroup
PER_SEQUENCE = ("out", "g_hp")
WALK_WRONG = ("later_visits_dropped", "later_visits_stale", "length_of_first_visit")


def first_visit_of(B, cap):
    """int64 [B]: b for b < cap, b - cap after it — the sequence a workgroup saw one visit earlier"""
    src = np.arange(B)
    src[cap:] -= cap
    return src


def visit_figures(got, ref, cap):
    """{name: (first, later)}: the figure of out and g_hp apart for the sequences of a workgroup's first visit (b < cap) and of
    its later ones, both against the whole array's max |ref|"""
    fig = {}
    for n in PER_SEQUENCE:
        a, b = np.asarray(got[n], np.float64), np.asarray(ref[n], np.float64)
        den = max(float(np.abs(b).max()), 1e-300)
        fig[n] = (float(np.abs(a[:cap] - b[:cap]).max()) / den, float(np.abs(a[cap:] - b[cap:]).max()) / den if len(b) > cap else 0.0)
    return fig


def visit_fmt(fig):
    return " ".join("%s first %.2e later %.2e" % (n, *v) for n, v in fig.items())


def walk_wrong(c, ref, wrong, cap):
    """deliberately WRONG results of a walk: 'later_visits_dropped' (gW1, gb1, gW2, gb2 and g_pos summed over the sequences
    b < cap only), 'later_visits_stale' (out and g_hp of sequence b >= cap those of b - cap), 'length_of_first_visit' (sequence
    b >= cap under the history mask of b - cap)"""
    src = first_visit_of(c["hist"].shape[0], cap)
    if wrong == "later_visits_dropped":
        cut = dict(c, hist=c["hist"][:cap], lengths=c["lengths"][:cap])
        part = pool_ref(cut, g_out=c["g_out"][:cap])
        return dict(ref, **{k: part[k] for k in ("gW1", "gb1", "gW2", "gb2", "g_pos")})
    if wrong == "later_visits_stale":
        return dict(ref, **{k: ref[k][src] for k in PER_SEQUENCE})
    if wrong == "length_of_first_visit":
        return pool_ref(c, g_out=c["g_out"], valid=(c["hist"] > 0)[src])
    raise ValueError(wrong)


def figure(x, ref, scale=None):
    """max |x - ref| / max |scale| (scale: ref itself unless given); anything not finite counts as infinitely wrong"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(x).all():
        return float("inf")
    return float(np.abs(x - ref).max() / max(np.abs(ref if scale is None else scale).max(), 1e-300))


# d out / d b2 is zero on paper (a softmax row's gradient sums to zero over t): its figure is taken on the scale of gW2
SCALE_OF = {"gb2": "gW2"}


def figures(got, ref):
    return {k: figure(got[k], ref[k], ref[SCALE_OF[k]] if k in SCALE_OF else None) for k in FIGURES if k in got and k in ref}


# ------------------------------------------------------------------------------------------------ ranks of K interests
RANK_MARGIN = 1e-4       # a row is judged when its target's nearest other score is further than this x max |score|
WRONG_RANK = ("sum_over_k", "mean_over_k", "target_from_interest_0")


def make_rank_case(D, n_items, n, KQ, seed=0):
    """queries [n, KQ, D], items [n_items, D], targets [n], 50 shared mask rows (CSR) with mask_row[e] != e"""
    rng = np.random.RandomState(1900 + seed + 7 * KQ + D)
    queries = rng.standard_normal((n, KQ, D)).astype(np.float32)
    items = rng.standard_normal((n_items, D)).astype(np.float32)
    # targets as a trained model meets them: 19 rows in 20 among the best 1 % of their row (8 at least), where the scores lie
    # apart, the others anywhere.  A uniformly drawn target among 2,100 normal scores has a neighbour within RANK_MARGIN in every
    # second row, and such rows say nothing about the kernel.
    S = np.einsum("ekd,jd->ekj", queries.astype(np.float64), items.astype(np.float64)).max(axis=1)
    top = rng.randint(0, max(8, n_items // 100), size=n)
    place = np.where(rng.random_sample(n) < 0.95, top, rng.randint(0, n_items, size=n))
    target = np.argsort(-S, axis=1)[np.arange(n), place].astype(np.int64)
    n_mask = 50
    # lists of up to 30 % of the items (one of them empty): items above a target are masked in many rows
    lists = [np.sort(rng.choice(n_items, size=rng.randint(0, 3 * n_items // 10) if r else 0, replace=False)).astype(np.int32)
             for r in range(n_mask)]
    mask_ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    mask_idx = np.concatenate(lists).astype(np.int32)
    mask_row = ((np.arange(n) * 7 + 3) % n_mask).astype(np.int64)
    for e in range(n):                        # never row e's own number, and never a list that holds the row's target
        while mask_row[e] == e or target[e] in lists[mask_row[e]]:
            mask_row[e] = (mask_row[e] + 1) % n_mask
    return dict(queries=queries, items=items, target=target, mask_ptr=mask_ptr, mask_idx=mask_idx, mask_row=mask_row)


def rank_ref(c, variant=None):
    """float64 ranks [n] (1 + unmasked items scoring above the target) and margins [n]: the distance of the target's score to the
    nearest other unmasked score, relative to max |score|"""
    q, it = c["queries"].astype(np.float64), c["items"].astype(np.float64)
    n = q.shape[0]
    per = np.einsum("ekd,jd->ekj", q, it)
    if variant == "sum_over_k":
        S = per.sum(axis=1)
    elif variant == "mean_over_k":
        S = per.mean(axis=1)
    else:
        S = per.max(axis=1)
    tsc = S[np.arange(n), c["target"]]
    if variant == "target_from_interest_0":
        tsc = per[np.arange(n), 0, c["target"]]
    keep = np.ones(S.shape, bool)
    for e in range(n):
        r = c["mask_row"][e]
        keep[e, c["mask_idx"][c["mask_ptr"][r]:c["mask_ptr"][r + 1]]] = False
    rank = 1 + (keep & (S > tsc[:, None])).sum(axis=1)
    other = keep.copy()
    other[np.arange(n), c["target"]] = False
    gap = np.where(other, np.abs(S - tsc[:, None]), np.inf).min(axis=1)
    return rank.astype(np.int64), gap / np.abs(S).max()
