"""Float64 restatement of the time-interval attention (whisprrec_amd/tisasrec.py::ti_attention_torch, reference
src/utils/layers.py:116-146) with its five gradients, of the block around it and of TiSASRec's forward, with the shapes, time
patterns, figures and tolerances of the K25 tests.  A helper module, not a conftest.

    r_ij = min(|t_i - t_j| // m_b, time_max)           s_ij = <q_i, k_j + time_k[r_ij]> / sqrt(d_k), j <= i, per head
    p_i. = softmax_j s_i.                               out_i = sum_j p_ij (v_j + time_v[r_ij])
    d time_k[r] += ds_ij q_i      d time_v[r] += p_ij d out_i      over every (b, h, i, j) with r_ij = r

The softmax here subtracts each row's own maximum; in float64 that equals the reference's shift by the call's maximum wherever the
latter is finite.

Figures: max |a - b| / max |b| per array (0 where both are exactly zero).  Groups: `out`; `gv` (d v, d time_v: sums of
probabilities times the upstream gradient); `gqk` (d q, d k: sums of ds = p (dp - sum p dp), terms that cancel — the group
sasblock_ref.py calls by the same name); `gtk` (d time_k).  A row of d time_k that collects whole softmax rows is
MATHEMATICALLY ZERO (sum_j ds_ij = 0: with equal timestamps every pair lands on row 0 and the whole gradient is rounding noise),
so d time_k is measured absolutely, against the largest sum of the MAGNITUDES of a row's contributions sum |ds_ij q_i|
(`gtk_mag`) — as sasblock_ref.py measures the k_linear.bias gradient against its weight's.

Tolerances: DESIGN section 2's rule.  The floor of a group is the stock fp32 torch path (ti_attention_torch under autograd, what
--ti_native 0 runs) against this restatement on a CPU; FLOORS holds the largest floor over SHAPES x PATTERNS; TOL = 8 x that,
rounded up to one digit.  tests/test_tisasrec_contract.py re-measures the floors and asserts 4 x floor < TOL.  WALK_SHAPES
(B above the kernels' workgroup caps: a workgroup visits several sequences) has WALK_FLOORS / WALK_TOL of its own, by the same rule.
"""
import numpy as np

LN_EPS = 1e-5
PARAMS = ["masked_attn_head.v_linear.weight", "masked_attn_head.v_linear.bias", "masked_attn_head.k_linear.weight",
          "masked_attn_head.k_linear.bias", "masked_attn_head.q_linear.weight", "masked_attn_head.q_linear.bias",
          "layer_norm1.weight", "layer_norm1.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
          "layer_norm2.weight", "layer_norm2.bias"]                     # _TiBlock.state_dict() order (the reference layer's)

# (B, T, D, heads, time_max): T = 1; odd T; d_k = 8; T just above 32; T maximum; the model's own shape
SHAPES = [(3, 1, 64, 4, 1), (5, 7, 32, 2, 8), (37, 20, 32, 4, 16), (2, 33, 64, 2, 512), (130, 64, 64, 1, 512), (96, 20, 64, 4, 512)]
PATTERNS = ("spread", "equal", "far")      # spread timestamps; all equal (every pair on row 0); every gap above time_max * m

GROUPS = ("out", "gv", "gqk", "gtk")
GROUP_OF = {"out": "out", "gv": "gv", "gtv": "gv", "gq": "gqk", "gk": "gqk", "gtk": "gtk"}

# Largest floor of each group over SHAPES x PATTERNS, stock fp32 ti_attention_torch against float64 on a CPU (measure_floors()
# below; `python tests/tisas_ref.py` prints every case).  torch's CPU backward of the two table gathers adds in thread order, so
# the figures move by up to 1.4x from run to run; these are the largest seen over three runs.  gv and gqk peak at
# (130, 64, 64, 1, 512) and (96, 20, 64, 4, 512) with the "far" and "equal" patterns: one table row collects every
# off-diagonal pair of the call.
FLOORS = {"out": 1.5e-7, "gv": 1.6e-5, "gqk": 1.2e-5, "gtk": 2.5e-7}
TOL = {"out": 2e-6, "gv": 2e-4, "gqk": 1e-4, "gtk": 2e-6}                  # 8 x floor, rounded up to one digit

# The caps of wr_tiattn.hip restated: a workgroup takes the sequences b, b + cap, b + 2 cap, ... once B exceeds the cap.
FWD_WG = 4096      # kTiFwdWg: workgroups of the forward
BWD_WG = 256       # kTiBwdWg: workgroups of the backward = slabs of table-gradient partials, added into on every visit

# Shapes at which a workgroup visits several sequences (backward: 2 - 3 visits, the last one ragged; (4099, 2, 32, 1, 4) walks the
# forward too, and gives the backward 16 - 17 visits).  Every pattern runs: with "equal" every pair of every visit adds into row 0
# of the workgroup's slab.
WALK_SHAPES = [(259, 7, 32, 2, 8), (515, 20, 64, 4, 512), (4099, 2, 32, 1, 4)]
WALK_SEED = 19000                             # make_case's seed base of this list (SHAPES: 9000)
# Largest floor of each group over WALK_SHAPES x PATTERNS, measured as FLOORS is (measure_floors(shapes=WALK_SHAPES, seed=WALK_SEED))
# — the largest seen over three runs (the thread order of torch's CPU gather backward moves gv between 6.4e-6 and 1.04e-5, gtk
# between 1.2e-7 and 1.4e-7).  out and gv peak at (515, 20, 64, 4, 512) "spread" / "far", gqk at (4099, 2, 32, 1, 4) "spread".
WALK_FLOORS = {"out": 1.65e-7, "gv": 1.04e-5, "gqk": 5.98e-6, "gtk": 1.41e-7}
WALK_TOL = {"out": TOL["out"], "gv": 9e-5, "gqk": 5e-5, "gtk": TOL["gtk"]}  # 8 x floor, rounded up to one digit; TOL's where equal
# The wrong results of a walk (walk_wrong below), smallest largest-figure / WALK_TOL over WALK_SHAPES x PATTERNS: later_visits_dropped
# 6.4e2 (at (259, 7, 32, 2, 8) "equal": 3 of 259 sequences missing), later_visits_stale 3.5e5.


# ------------------------------------------------------------------------------------------------ intervals
def intervals(times, min_interval, time_max):
    """[B, T, T] int64 min(|t_i - t_j| // max(m_b, 1), time_max) — integer floor division"""
    t = np.asarray(times, np.int64)
    m = np.maximum(np.asarray(min_interval, np.int64), 1)
    return np.minimum(np.abs(t[:, :, None] - t[:, None, :]) // m[:, None, None], int(time_max))


def min_intervals(user_his, n_users, cap=65535):
    """the model's per-user scale restated: the smallest positive difference between any two timestamps of a user, at most
    `cap`; `cap` without one"""
    out = np.full(n_users, cap, np.int64)
    for u, his in user_his.items():
        ts = sorted({int(x[1]) for x in his})
        gaps = [b - a for a, b in zip(ts, ts[1:])]
        if gaps:
            out[u] = min(min(gaps), cap)
    return out


# ------------------------------------------------------------------------------------------------ inputs
def make_times(pattern, B, T, time_max, rng):
    """-> (times int64 [B, T], min_interval int64 [B])"""
    m = np.asarray([1, 7, 60, 86400, 3, 65535])[rng.randint(0, 6, B)].astype(np.int64)
    if pattern == "equal":
        gaps = np.zeros((B, T), np.int64)
    elif pattern == "far":
        gaps = (time_max + 1 + rng.randint(0, 4, (B, T))) * m[:, None]
    else:                                                   # quotients on both sides of the clamp, with remainders
        gaps = (rng.randint(0, 2 * time_max + 2, (B, T)) * m[:, None]) // np.maximum(T // 2, 1) + rng.randint(0, 2, (B, T))
    return 1_000_000_000 + np.cumsum(gaps, axis=1), m


def make_case(i, pattern, shapes=None, seed=9000):
    """-> dict(q, k, v, gout [B, T, D] fp32, tk, tv [time_max + 1, D] fp32, times, min_interval, heads, time_max) of SHAPES[i];
    shapes / seed: another list (WALK_SHAPES) with its own seed base"""
    B, T, D, heads, time_max = (SHAPES if shapes is None else shapes)[i]
    rng = np.random.RandomState(seed + 10 * i + PATTERNS.index(pattern))
    f = lambda *s: rng.standard_normal(s)                   # noqa: E731
    c = {"q": f(B, T, D) * 0.7, "k": f(B, T, D) * 0.7, "v": f(B, T, D) * 0.5, "gout": f(B, T, D),
         "tk": f(time_max + 1, D) * 0.4, "tv": f(time_max + 1, D) * 0.4}
    c = {n: a.astype(np.float32) for n, a in c.items()}
    c["times"], c["min_interval"] = make_times(pattern, B, T, time_max, rng)
    c["heads"], c["time_max"] = heads, time_max
    return c


# ------------------------------------------------------------------------------------------------ the attention in float64
def attn_f64(q, k, v, interval, tk, tv, heads, gout=None, wrong=None):
    """-> dict(out, P [B, h, T, T] and, with gout, gq, gk, gv, gtk, gtv).  `wrong` builds deliberately WRONG results for the
    power checks: 'no_time_k', 'no_time_v', 'mask_shift', 'no_scale'."""
    f = np.float64
    q, k, v, tk, tv = (np.asarray(a, f) for a in (q, k, v, tk, tv))
    B, T, D = q.shape
    dk = D // heads
    R = np.asarray(interval, np.int64)

    def split(z):                                           # [B, T, D] -> [B, h, T, dk]
        return z.reshape(B, T, heads, dk).transpose(0, 2, 1, 3)

    def merge(z):
        return z.transpose(0, 2, 1, 3).reshape(B, T, D)

    def split_pair(z):                                      # [B, T, T, D] -> [B, h, T, T, dk]
        return z.reshape(B, T, T, heads, dk).transpose(0, 3, 1, 2, 4)

    qh, kh, vh = split(q), split(k), split(v)
    ik = split_pair(tk[R]) * (0.0 if wrong == "no_time_k" else 1.0)
    iv = split_pair(tv[R]) * (0.0 if wrong == "no_time_v" else 1.0)
    sc = 1.0 if wrong == "no_scale" else 1.0 / np.sqrt(f(dk))
    S = (np.einsum("bhid,bhjd->bhij", qh, kh) + np.einsum("bhid,bhijd->bhij", qh, ik)) * sc
    causal = np.tril(np.ones((T, T), bool), -1 if (wrong == "mask_shift" and T > 1) else 0)
    if wrong == "mask_shift" and T > 1:
        causal[0, 0] = True
    S = np.where(causal, S, -np.inf)
    E = np.exp(S - S.max(-1, keepdims=True))
    P = E / E.sum(-1, keepdims=True)
    out = merge(P @ vh + np.einsum("bhij,bhijd->bhid", P, iv))
    res = {"out": out, "P": P}
    if gout is None:
        return res
    dO = split(np.asarray(gout, f))
    dP = np.einsum("bhid,bhjd->bhij", dO, vh) + np.einsum("bhid,bhijd->bhij", dO, iv)
    dS = P * (dP - (P * dP).sum(-1, keepdims=True)) * sc    # w.r.t. the plain products
    res["gq"] = merge(dS @ kh + np.einsum("bhij,bhijd->bhid", dS, ik))
    res["gk"] = merge(dS.transpose(0, 1, 3, 2) @ qh)
    res["gv"] = merge(P.transpose(0, 1, 3, 2) @ dO)
    # per pair and column: d inter_k[b, i, j, h dk + d] = dS[b, h, i, j] q[b, h, i, d]; scattered by r
    dik = np.einsum("bhij,bhid->bijhd", dS, qh).reshape(B, T, T, D)
    div = np.einsum("bhij,bhid->bijhd", P, dO).reshape(B, T, T, D)
    order = np.argsort(R.reshape(-1), kind="stable")
    rows, first = np.unique(R.reshape(-1)[order], return_index=True)
    gtk, gtv = np.zeros_like(tk), np.zeros_like(tv)
    gtk[rows] = np.add.reduceat(dik.reshape(-1, D)[order], first, axis=0)
    mag = np.zeros_like(tk)                                 # the sum of the magnitudes of d time_k's contributions
    mag[rows] = np.add.reduceat(np.abs(dik).reshape(-1, D)[order], first, axis=0)
    res["gtk_mag"] = mag
    gtv[rows] = np.add.reduceat(div.reshape(-1, D)[order], first, axis=0)
    res["gtk"], res["gtv"] = gtk, gtv
    return res


def case_f64(c, wrong=None):
    R = intervals(c["times"], c["min_interval"], c["time_max"])
    return attn_f64(c["q"], c["k"], c["v"], R, c["tk"], c["tv"], c["heads"], c["gout"], wrong=wrong)


# ------------------------------------------------------------------------------------------------ the block and the model
def _ln_fwd(y, g, b):
    mu = y.mean(-1, keepdims=True)
    var = ((y - mu) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    xh = (y - mu) * rstd
    return xh * g + b, xh, rstd


def _ln_bwd(dy, xh, rstd, g):
    dxh = dy * g
    return rstd * (dxh - dxh.mean(-1, keepdims=True) - xh * (dxh * xh).mean(-1, keepdims=True))


def block_f64(x, pos_k, pos_v, interval, tk, tv, sd, heads, gout=None):
    """one TimeIntervalTransformerLayer (dropout 0) -> dict(out and, with gout, gx, gpos_k, gpos_v, gtk, gtv, g[name])"""
    f = np.float64
    x, pos_k, pos_v = (np.asarray(a, f) for a in (x, pos_k, pos_v))
    W = {n: np.asarray(sd[n], f) for n in PARAMS}
    pq, pk, pv = (["masked_attn_head.%s_linear.%s" % (c, s) for s in ("weight", "bias")] for c in "qkv")
    q = x @ W[pq[0]].T + W[pq[1]]
    k = x @ W[pk[0]].T + W[pk[1]] + pos_k
    v = x @ W[pv[0]].T + W[pv[1]] + pos_v

    def attend(go=None):
        return attn_f64(q, k, v, interval, tk, tv, heads, go)

    att = attend()
    C, xh1, rstd1 = _ln_fwd(att["out"] + x, W["layer_norm1.weight"], W["layer_norm1.bias"])
    pre = C @ W["linear1.weight"].T + W["linear1.bias"]
    H = np.maximum(pre, 0.0)
    O2 = H @ W["linear2.weight"].T + W["linear2.bias"]
    out, xh2, rstd2 = _ln_fwd(O2 + C, W["layer_norm2.weight"], W["layer_norm2.bias"])
    res = {"out": out}
    if gout is None:
        return res
    G = np.asarray(gout, f)
    g = {}

    def wsum(a, b):
        return np.einsum("btj,btd->jd", a, b)

    g["layer_norm2.weight"], g["layer_norm2.bias"] = (G * xh2).sum((0, 1)), G.sum((0, 1))
    dY2 = _ln_bwd(G, xh2, rstd2, W["layer_norm2.weight"])
    g["linear2.weight"], g["linear2.bias"] = wsum(dY2, H), dY2.sum((0, 1))
    dpre = (dY2 @ W["linear2.weight"]) * (pre > 0)
    g["linear1.weight"], g["linear1.bias"] = wsum(dpre, C), dpre.sum((0, 1))
    dC = dY2 + dpre @ W["linear1.weight"]
    g["layer_norm1.weight"], g["layer_norm1.bias"] = (dC * xh1).sum((0, 1)), dC.sum((0, 1))
    dY1 = _ln_bwd(dC, xh1, rstd1, W["layer_norm1.weight"])
    att = attend(dY1)
    gx = dY1.copy()
    for (w, b), d in ((pq, att["gq"]), (pk, att["gk"]), (pv, att["gv"])):
        g[w], g[b] = wsum(d, x), d.sum((0, 1))
        gx += d @ W[w]
    res.update(gx=gx, gpos_k=att["gk"], gpos_v=att["gv"], gtk=att["gtk"], gtv=att["gtv"], g=g)
    return res


def model_forward_f64(sd, hist, lengths, times, min_interval, heads, time_max):
    """TiSASRec.forward in float64 from a model state dict (names of whisprrec_amd/tisasrec.py) -> [B, D] user vectors"""
    f = np.float64
    hist, lengths = np.asarray(hist, np.int64), np.asarray(lengths, np.int64)
    B, T = hist.shape
    valid = hist > 0
    position = (lengths[:, None] - np.arange(T)[None, :]) * valid
    x = np.asarray(sd["item_embedding.weight"], f)[hist]
    pos_k = np.asarray(sd["position_k_embedding.weight"], f)[position]
    pos_v = np.asarray(sd["position_v_embedding.weight"], f)[position]
    R = intervals(times, min_interval, time_max)
    n_layers = 1 + max(int(n.split(".")[1]) for n in sd if n.startswith("transformer_block."))
    for layer in range(n_layers):
        pre = "transformer_block.%d." % layer
        x = block_f64(x, pos_k, pos_v, R, sd["time_k_embedding.weight"], sd["time_v_embedding.weight"],
                      {n: sd[pre + n] for n in PARAMS}, heads)["out"]
    x = x * valid[:, :, None]
    return x[np.arange(B), lengths - 1]


# ------------------------------------------------------------------------------------------------ figures
def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    diff, den = float(np.max(np.abs(a - b))), float(np.max(np.abs(b)))
    return diff / den if den > 0 else (0.0 if diff == 0 else float("inf"))


def figures(got, ref):
    """got: dict(out, gq, gk, gv, gtk, gtv) -> relative error of each against attn_f64's result; gtk absolutely, against the
    largest entry of gtk_mag"""
    fig = {n: rel_err(got[n], ref[n]) for n in GROUP_OF if n != "gtk"}
    diff, den = float(np.max(np.abs(np.asarray(got["gtk"], np.float64) - ref["gtk"]))), float(np.max(ref["gtk_mag"]))
    fig["gtk"] = diff / den if den > 0 else (0.0 if diff == 0 else float("inf"))
    return fig


def worst(fig):
    w = {g: 0.0 for g in GROUPS}
    for n, v in fig.items():
        w[GROUP_OF[n]] = max(w[GROUP_OF[n]], v)
    return w


def fmt(tag, fig, tol=None):
    w, tol = worst(fig), TOL if tol is None else tol
    return "parity ti_attention %s: " % tag + " ".join("%s %.2e (tol %.0e)" % (g, w[g], tol[g]) for g in GROUPS)


# ------------------------------------------------------------------------------------------------ several visits per workgroup
PER_SEQUENCE = ("out", "gq", "gk", "gv")


def first_sequences(c, n):
    """the case cut to its first n sequences (the tables stay)"""
    cut = dict(c)
    for k in ("q", "k", "v", "gout", "times", "min_interval"):
        cut[k] = c[k][:n]
    return cut


def first_visit_of(B, cap):
    """int64 [B]: b for b < cap, b - cap after it — the sequence a workgroup saw one visit earlier"""
    src = np.arange(B)
    src[cap:] -= cap
    return src


def visit_figures(got, ref, cap):
    """{name: (first, later)}: the figure of each per-sequence array apart for the sequences of a workgroup's first visit
    (b < cap) and of its later ones, both against the whole array's max |ref|"""
    fig = {}
    for n in PER_SEQUENCE:
        a, b = np.asarray(got[n], np.float64), np.asarray(ref[n], np.float64)
        den = max(float(np.max(np.abs(b))), 1e-300)
        fig[n] = (float(np.max(np.abs(a[:cap] - b[:cap]))) / den, float(np.max(np.abs(a[cap:] - b[cap:]))) / den if len(b) > cap else 0.0)
    return fig


def visit_fmt(fig):
    return " ".join("%s first %.2e later %.2e" % (n, *v) for n, v in fig.items())


def walk_wrong(c, ref, wrong, cap):
    """deliberately WRONG results of a walk: 'later_visits_dropped' (the two table gradients summed over the sequences b < cap
    only), 'later_visits_stale' (out, gq, gk, gv of sequence b >= cap replaced by those of b - cap)"""
    bad = dict(ref)
    if wrong == "later_visits_dropped":
        part = case_f64(first_sequences(c, cap))
        bad["gtk"], bad["gtv"] = part["gtk"], part["gtv"]
    elif wrong == "later_visits_stale":
        src = first_visit_of(len(ref["out"]), cap)
        for n in PER_SEQUENCE:
            bad[n] = ref[n][src]
    else:
        raise ValueError(wrong)
    return bad


def stock_fp32(c, device="cpu"):
    """the stock path under torch.autograd (what --ti_native 0 runs after the projections) -> dict(out, gq, gk, gv, gtk, gtv)"""
    import torch
    from whisprrec_amd.tisasrec import interval_matrix, ti_attention_torch
    leaves = {n: torch.as_tensor(c[n], dtype=torch.float32, device=device).clone().requires_grad_(True)
              for n in ("q", "k", "v", "tk", "tv")}
    T = c["q"].shape[1]
    R = interval_matrix(torch.as_tensor(c["times"], device=device), torch.as_tensor(c["min_interval"], device=device), c["time_max"])
    mask = torch.tril(torch.ones(1, 1, T, T, dtype=torch.int32, device=device))
    out = ti_attention_torch(leaves["q"], leaves["k"], leaves["v"], leaves["tk"][R], leaves["tv"][R], mask, c["heads"])
    out.backward(torch.as_tensor(c["gout"], dtype=torch.float32, device=device))
    res = {"out": out.detach().cpu().numpy()}
    for n in ("q", "k", "v", "tk", "tv"):
        res["g" + n] = leaves[n].grad.cpu().numpy()
    return res


def measure_floors(shapes=None, patterns=PATTERNS, walk=False):
    """-> {group: largest figure of the stock fp32 path against float64 on a CPU}, and the per-case figures; `shapes`: indices
    into SHAPES, or into WALK_SHAPES with walk=True"""
    floors, cases = {g: 0.0 for g in GROUPS}, {}
    lst = (WALK_SHAPES, WALK_SEED) if walk else (None, 9000)
    for i in (range(len(WALK_SHAPES if walk else SHAPES)) if shapes is None else shapes):
        for pat in patterns:
            c = make_case(i, pat, *lst)
            w = worst(figures(stock_fp32(c), case_f64(c)))
            cases[(i, pat)] = w
            for g in GROUPS:
                floors[g] = max(floors[g], w[g])
    return floors, cases


if __name__ == "__main__":
    import time
    t0 = time.time()
    fl, per = measure_floors()
    for key, w in per.items():
        print(SHAPES[key[0]], key[1], " ".join("%s %.2e" % (g, w[g]) for g in GROUPS))
    print("floors", fl, "%.1f s" % (time.time() - t0))
