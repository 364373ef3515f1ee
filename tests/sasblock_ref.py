"""Float64 restatement of one SASRec transformer block (whisprrec_amd/sasrec.py::_Block, reference src/utils/layers.py:8-86)
with its backward, the counter-based dropout mask of wr_sasblock.hip restated bit for bit, and the shapes, figures and
tolerances of the K13 tests.  A helper module, not a conftest.

    q, k, v = x Wq^T + bq, ...                       S = q k^T / sqrt(d_k), causal          P = softmax(S - max over the call)
    A = P v (rows with sum exp == 0 are 0)           C = LN1(drop1(A) + x)
    H = relu(C W1^T + b1)                            out = LN2(drop2(H W2^T + b2) + C)

The backward ignores the path through the global maximum (softmax is shift-invariant: it sums to zero) and passes nothing
through the scores of a zeroed row.

Figures: max |a - b| / max |b| for the output, gx and every parameter gradient — except `k_linear.bias`, whose gradient is
mathematically zero (q . b_k is constant along a softmax row): it is measured absolutely, against max |g(k_linear.weight)|.

Tolerances: DESIGN section 2's rule.  The floor of a figure is the stock fp32 `_Block` (torch.autograd) against this
restatement on a CPU; FLOORS holds the largest floor over SHAPES at p = 0 and at p = 0.1 (explicit mask); TOL = 8 x that,
rounded up to one digit.  tests/test_sasblock_contract.py re-measures the floors and asserts 4 x floor < TOL.

WALK_SHAPES (a workgroup visits several sequences: B above the kernels' workgroup caps) and FORM_SHAPES (every <D, TM> form of the
kernels at its border) have floors and tolerances of their own, by the same rule, and the same test re-measures them; the deliberately
WRONG results of a walk (`later_visits_dropped`, stale(), a mask or a maximum taken at the first visit) stand 5 x WALK_TOL out.
"""
import numpy as np

LN_EPS = 1e-5
PARAMS = ["masked_attn_head.q_linear.weight", "masked_attn_head.q_linear.bias", "masked_attn_head.k_linear.weight",
          "masked_attn_head.k_linear.bias", "masked_attn_head.v_linear.weight", "masked_attn_head.v_linear.bias",
          "layer_norm1.weight", "layer_norm1.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
          "layer_norm2.weight", "layer_norm2.bias"]                     # _Block.state_dict() order: the order of the C-ABI
KB, KW = "masked_attn_head.k_linear.bias", "masked_attn_head.k_linear.weight"

# (B, T, D, heads); the first is g5's batch and state dict
SHAPES = [(96, 20, 64, 4), (3, 1, 64, 4), (5, 7, 32, 2), (2, 33, 64, 2), (130, 64, 64, 1), (37, 20, 32, 4)]

# Largest floor of each figure over SHAPES x {p = 0, p = 0.1}, stock fp32 _Block against float64 on a CPU.
# The largest ones come from (37, 20, 32, 4): d_k = 8, and the q / k gradients are sums of cancelling softmax terms.
FLOORS = {"out": 3.3e-7, "gx": 3.4e-7, "gqk": 5.2e-6, "gparam": 1.3e-6, "gkb": 9.6e-6}
TOL = {"out": 3e-6, "gx": 3e-6, "gqk": 5e-5, "gparam": 2e-5, "gkb": 8e-5}          # 8 x floor, rounded up to one digit

# The caps of wr_sasblock.hip restated: a workgroup takes the sequences b, b + cap, b + 2 cap, ... once B exceeds the cap.
FWD_WG = 2048      # kSasFwdWg: workgroups of forward launch 1, the partial maxima (launch 2 runs one workgroup per sequence)
BWD_WG = 512       # kSasBwdWg: workgroups of the backward, which carry the parameter-gradient partials across their visits

# Shapes at which a workgroup visits several sequences: most workgroups of the backward visit two, a few three, the last
# visit is ragged; (2051, 2, 64, 4) also walks forward launch 1 (2,048 + 3) and gives the backward 4 - 5 visits;
# (515, 20, 64, 4) is the production form; (515, 33, 32, 2) is the <32, 64> form, which walks as well.  Each runs at p = 0
# and p = 0.1: the mask index is (b T + t) D + d, so dropout parity on a later visit checks the true b.
WALK_SHAPES = [(1027, 5, 32, 2), (2051, 2, 64, 4), (515, 20, 64, 4), (515, 33, 32, 2)]
# The <D, TM> forms of WR_SAS_DISPATCH ({32, 64} x {24, 64}) at their border: T = 24 fills a TM = 24 tile, T = 25 is the first
# T of the TM = 64 form; (4, 64, 32, 1) fills the <32, 64> tile.
FORM_SHAPES = [(3, 25, 32, 4), (4, 64, 32, 1), (3, 24, 64, 2), (3, 24, 32, 2), (3, 25, 64, 2)]
WALK_SEED, FORM_SEED = 17000, 27000           # make_case's seed bases of the two lists (SHAPES: 7000)

# Largest floor of each figure over the list x {p = 0, p = 0.1}, measured as FLOORS is (test_sasblock_contract.py prints them).
# WALK: gqk and gkb peak at (2051, 2, 64, 4) p = 0 (T = 2: the score gradients are differences of two nearly equal terms), gparam
# at (515, 33, 32, 2) p = 0.1.  FORM: gqk at (3, 25, 32, 4) p = 0.1, gkb at (3, 24, 64, 2) p = 0.
WALK_FLOORS = {"out": 2.74e-7, "gx": 3.16e-7, "gqk": 4.27e-6, "gparam": 1.63e-6, "gkb": 1.50e-5}
FORM_FLOORS = {"out": 2.69e-7, "gx": 2.70e-7, "gqk": 2.12e-6, "gparam": 5.48e-7, "gkb": 9.08e-6}
# 8 x floor, rounded up to one digit (rule_of below); TOL's own value where the rule lands on it
WALK_TOL = {"out": TOL["out"], "gx": TOL["gx"], "gqk": 4e-5, "gparam": TOL["gparam"], "gkb": 2e-4}
FORM_TOL = {"out": TOL["out"], "gx": TOL["gx"], "gqk": 2e-5, "gparam": 5e-6, "gkb": TOL["gkb"]}
# The wrong results of a walk (tests/test_sasblock_contract.py), smallest largest-figure / WALK_TOL over WALK_SHAPES at p = 0.1:
# later_visits_dropped 4.6e3 (at (515, 20, 64, 4): 3 of 515 sequences missing), later_visits_stale 2.9e5, mask_of_first_visit 1.8e5;
# max_of_first_visit misses the stored maximum (21.92 at x[2049] x 100) by 21.91, against the 1e-5 relative it is held to.


def rule_of(floor):
    """DESIGN section 2's rule: 8 x floor, rounded up to one digit"""
    v = 8.0 * floor
    e = int(np.floor(np.log10(v)))
    return float("%de%d" % (int(np.ceil(v / 10.0 ** e - 1e-9)), e))


# ------------------------------------------------------------------------------------------------ dropout mask
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(x):
    """splitmix64 finaliser (wr_sampler.hip's mix64)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def drop_threshold(p):
    """24-bit threshold of the fp32 probability p: an element is kept iff its 24-bit draw is >= it"""
    return int(float(np.float32(p)) * 16777216.0)


def keep_mask(seed, site, B, T, D, p):
    """bool [B, T, D]: the keep mask of dropout site 0 (after attention) / 1 (after the feed-forward)"""
    with np.errstate(over="ignore"):
        key = _mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ (np.uint64(site + 1) * np.uint64(0x9E3779B97F4A7C15)))
        e = np.arange(B * T * D, dtype=np.uint64)
        r = _mix64(key ^ (e * np.uint64(0xD1B54A32D192ED03) + np.uint64(1))) >> np.uint64(40)
    return (r >= np.uint64(drop_threshold(p))).reshape(B, T, D)


def drop_scale(p):
    """the fp32 scale 1 / (1 - p) the kernel multiplies kept elements with"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def masks_for(seed, B, T, D, p):
    """the two multiplicative masks (keep * scale) as float64, or None for p == 0"""
    if p == 0:
        return None, None
    s = drop_scale(p)
    return keep_mask(seed, 0, B, T, D, p) * s, keep_mask(seed, 1, B, T, D, p) * s


# ------------------------------------------------------------------------------------------------ inputs
def xavier_params(D, heads, rng):
    """_xavier_normal_all: linear weights N(0, 2 / (fan_in + fan_out)), biases 0; LayerNorm 1 / 0"""
    sd = {}
    for n in PARAMS:
        if n.endswith("weight") and "layer_norm" not in n:
            sd[n] = (rng.standard_normal((D, D)) * np.sqrt(2.0 / (2 * D))).astype(np.float32)
        elif "layer_norm" in n and n.endswith("weight"):
            sd[n] = np.ones(D, np.float32)
        else:
            sd[n] = np.zeros(D, np.float32)
    return sd


def make_case(i, g5=None, shapes=None, seed=7000):
    """-> (x [B, T, D] fp32, params, upstream gradient [B, T, D] fp32, heads) of SHAPES[i]; case 0 needs the g5 set.
    shapes / seed: another list (WALK_SHAPES, FORM_SHAPES) with its own seed base; SHAPES' data does not depend on them."""
    B, T, D, heads = (SHAPES if shapes is None else shapes)[i]
    rng = np.random.RandomState(seed + i)
    if i == 0 and shapes is None:
        pre = "sd__transformer_block.0."
        sd = {n: np.asarray(g5[pre + n], np.float32) for n in PARAMS}
        x = (g5["sd__item_embedding.weight"][g5["hist"]] + g5["sd__position_embedding.weight"][np.arange(T)][None]).astype(np.float32)
    else:
        sd = xavier_params(D, heads, rng)
        # the scale of xavier-initialised tables (3,706 items): item + position rows
        x = (rng.standard_normal((B, T, D)) * np.sqrt(2.0 / (3706 + D)) * np.sqrt(2.0)).astype(np.float32)
    # parameters away from their initial 0 / 1 so that every gradient path carries weight
    rp = np.random.RandomState(seed + 100 + i)
    for n in PARAMS:
        if n.endswith("bias"):
            sd[n] = (sd[n] + 0.05 * rp.standard_normal(sd[n].shape)).astype(np.float32)
        elif "layer_norm" in n:
            sd[n] = (sd[n] + 0.1 * rp.standard_normal(sd[n].shape)).astype(np.float32)
    g = rng.standard_normal((B, T, D)).astype(np.float32)
    return x, sd, g, heads


# ------------------------------------------------------------------------------------------------ the block in float64
def _ln_fwd(y, g, b, eps):
    mu = y.mean(-1, keepdims=True)
    var = ((y - mu) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (y - mu) * rstd
    return xh * g + b, xh, rstd


def _ln_bwd(dy, xh, rstd, g):
    dxh = dy * g
    return rstd * (dxh - dxh.mean(-1, keepdims=True) - xh * (dxh * xh).mean(-1, keepdims=True))


def block_f64(x, sd, heads, gout=None, m1=None, m2=None, wrong=None, zero_below=None, zero_rows=None, first=None):
    """-> dict(out, gmax, P [B, h, T, T], zero_rows [B, h, T] and, with gout, gx and g[name] for every parameter).
    m1 / m2: multiplicative dropout masks (keep * scale) or None.  `wrong` builds deliberately WRONG blocks for the power
    checks: 'no_scale', 'mask_shift', 'ln_no_eps', 'ln_no_bias_grad', 'drop_no_scale:<scale>', 'v_head', 'relu_gate',
    'skip_seq'.  zero_below: a score row whose own maximum lies more than this far below the call's maximum is zeroed, as
    it is in any fp32 evaluation (exp underflows to 0 at -104, at -88 without denormals; float64 only at -745).
    zero_rows: bool [B, h, T], score rows to zero on top of that.
    first: with wrong = 'later_visits_dropped', the number of sequences whose terms enter the parameter-gradient sums."""
    f = np.float64
    x = np.asarray(x, f)
    W = {n: np.asarray(sd[n], f) for n in PARAMS}
    pq, pk, pv = (["masked_attn_head.%s_linear.%s" % (c, s) for s in ("weight", "bias")] for c in "qkv")
    B, T, D = x.shape
    dk = D // heads
    eps = 0.0 if wrong == "ln_no_eps" else LN_EPS
    if wrong is not None and wrong.startswith("drop_no_scale"):
        s = float(wrong.split(":")[1])
        m1, m2 = m1 / s, m2 / s
    one = np.ones((), f)
    m1 = one if m1 is None else np.asarray(m1, f)
    m2 = one if m2 is None else np.asarray(m2, f)

    def split(z):
        return z.reshape(B, T, heads, dk).transpose(0, 2, 1, 3)

    def merge(z):
        return z.transpose(0, 2, 1, 3).reshape(B, T, D)

    q, k, v = (split(x @ W[w].T + W[b]) for w, b in (pq, pk, pv))
    sc = 1.0 if wrong == "no_scale" else 1.0 / np.sqrt(f(dk))
    S = np.einsum("bhid,bhjd->bhij", q, k) * sc
    causal = np.tril(np.ones((T, T), bool), -1 if (wrong == "mask_shift" and T > 1) else 0)
    if wrong == "mask_shift" and T > 1:
        causal[0, 0] = True
    S = np.where(causal, S, -np.inf)
    gmax = S.max()
    with np.errstate(under="ignore"):
        E = np.exp(S - gmax)
    gap = gmax - S.max(-1)                       # [B, h, T]: how far each row's best score lies below the call's
    if zero_below is not None:
        E = np.where((gap > zero_below)[..., None], 0.0, E)
    if zero_rows is not None:
        E = np.where(np.asarray(zero_rows, bool)[..., None], 0.0, E)
    Z = E.sum(-1, keepdims=True)
    zero = Z == 0
    P = np.where(zero, 0.0, E / np.where(zero, 1.0, Z))
    A = merge(P @ v)
    C, xh1, rstd1 = _ln_fwd(A * m1 + x, W["layer_norm1.weight"], W["layer_norm1.bias"], eps)
    pre = C @ W["linear1.weight"].T + W["linear1.bias"]
    H = np.maximum(pre, 0.0)
    O2 = H @ W["linear2.weight"].T + W["linear2.bias"]
    out, xh2, rstd2 = _ln_fwd(O2 * m2 + C, W["layer_norm2.weight"], W["layer_norm2.bias"], eps)
    res = {"out": out, "gmax": float(gmax), "P": P, "zero_rows": zero[..., 0], "A": A, "gap": gap, "seq_max": S.max((1, 2, 3))}
    if gout is None:
        return res
    G = np.asarray(gout, f)
    g = {}
    keep = np.ones(B, bool)
    if wrong == "skip_seq":
        keep[B - 1] = False                      # one sequence missing from every weight-gradient sum
    if wrong == "later_visits_dropped":
        keep[first:] = False                     # only each workgroup's first visit reaches the weight-gradient sums

    def wsum(a, b):                              # sum over sequences and positions of a^T b
        return np.einsum("btj,btd->jd", a[keep], b[keep])

    def bsum(a):
        return a[keep].sum((0, 1))

    g["layer_norm2.weight"], g["layer_norm2.bias"] = bsum(G * xh2), bsum(G)
    dY2 = _ln_bwd(G, xh2, rstd2, W["layer_norm2.weight"])
    dO2 = dY2 * m2
    g["linear2.weight"], g["linear2.bias"] = wsum(dO2, H), bsum(dO2)
    dH = dO2 @ W["linear2.weight"]
    dpre = dH if wrong == "relu_gate" else dH * (pre > 0)
    g["linear1.weight"], g["linear1.bias"] = wsum(dpre, C), bsum(dpre)
    dC = dY2 + dpre @ W["linear1.weight"]
    g["layer_norm1.weight"], g["layer_norm1.bias"] = bsum(dC * xh1), bsum(dC)
    if wrong == "ln_no_bias_grad":
        g["layer_norm1.bias"] = np.zeros(D)
        g["layer_norm2.bias"] = np.zeros(D)
    dY1 = _ln_bwd(dC, xh1, rstd1, W["layer_norm1.weight"])
    dA = split(dY1 * m1)
    dP = np.einsum("bhid,bhjd->bhij", dA, v)
    dS = P * (dP - (P * dP).sum(-1, keepdims=True))
    dq = merge(dS @ k) * sc
    dkk = merge(dS.transpose(0, 1, 3, 2) @ q) * sc
    dvh = P.transpose(0, 1, 3, 2) @ dA
    if wrong == "v_head":
        dvh[:, heads - 1] = 0.0
    dv = merge(dvh)
    gx = dY1.copy()
    for (w, b), d in ((pq, dq), (pk, dkk), (pv, dv)):
        g[w], g[b] = wsum(d, x), bsum(d)
        gx += d @ W[w]
    res["gx"], res["g"] = gx, g
    return res


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def figures(out, gx, gparams, ref):
    """relative error of the output, of gx and of each parameter gradient against block_f64's result; the k_linear.bias
    gradient absolutely, against max |g(k_linear.weight)|"""
    fig = {"out": rel_err(out, ref["out"]), "gx": rel_err(gx, ref["gx"])}
    for n in PARAMS:
        if n == KB:
            # T = 1: the softmax is the constant 1, g(k_linear.weight) is exactly zero and so must this gradient be
            diff, den = float(np.max(np.abs(np.asarray(gparams[n], np.float64) - ref["g"][n]))), float(np.max(np.abs(ref["g"][KW])))
            fig[n] = diff / den if den > 0 else (0.0 if diff == 0 else float("inf"))
        else:
            fig[n] = rel_err(gparams[n], ref["g"][n])
    return fig


QK = ("masked_attn_head.q_linear.weight", "masked_attn_head.q_linear.bias", KW)
GROUPS = ("out", "gx", "gqk", "gparam", "gkb")


def group_of(name):
    """the tolerance group of a figure.  `gqk`: the gradients that arrive through the scores (q weight and bias, k weight) are
    sums of terms P (dP - sum P dP) that cancel — their fp32 floor is ten times that of the other parameters"""
    return name if name in ("out", "gx") else "gkb" if name == KB else "gqk" if name in QK else "gparam"


def worst(fig):
    """the largest figure of each tolerance group"""
    w = {k: 0.0 for k in GROUPS}
    for n, v in fig.items():
        w[group_of(n)] = max(w[group_of(n)], v)
    return w


def fmt(tag, fig, tol=None):
    w, tol = worst(fig), TOL if tol is None else tol
    return "parity sasblock %s: " % tag + " ".join("%s %.2e (tol %.0e)" % (k, w[k], tol[k]) for k in GROUPS)


# ------------------------------------------------------------------------------------------------ several visits per workgroup
def first_visit_of(B, cap):
    """int64 [B]: b for b < cap, b - cap after it — the sequence a workgroup saw one visit earlier"""
    src = np.arange(B)
    src[cap:] -= cap
    return src


def visit_figures(got, ref, cap, names=("out", "gx")):
    """{name: (first, later)}: the figure of each per-sequence array apart for the sequences of a workgroup's first visit
    (b < cap) and of its later ones, both against the whole array's max |ref| — the larger of the two is figures()'s"""
    fig = {}
    for n in names:
        a, b = np.asarray(got[n], np.float64), np.asarray(ref[n], np.float64)
        den = max(float(np.max(np.abs(b))), 1e-300)
        fig[n] = (float(np.max(np.abs(a[:cap] - b[:cap]))) / den, float(np.max(np.abs(a[cap:] - b[cap:]))) / den if len(b) > cap else 0.0)
    return fig


def visit_fmt(fig):
    return " ".join("%s first %.2e later %.2e" % (n, *v) for n, v in fig.items())


def stale(res, cap, names=("out", "gx")):
    """the WRONG result `later_visits_stale`: what belongs to sequence b >= cap replaced by that of sequence b - cap"""
    bad = dict(res)
    for n in names:
        bad[n] = np.asarray(res[n])[first_visit_of(len(res[n]), cap)]
    return bad


def stock_fp32(x, sd, heads, gout, m1=None, m2=None, device="cpu", dtype=None):
    """the stock `_Block` under torch.autograd (what --block_native 0 runs), with explicit dropout masks
    -> (out, gx, {name: grad})"""
    import torch
    from whisprrec_amd.sasrec import _Block
    dtype = dtype or torch.float32
    B, T, D = x.shape
    blk = _Block(D, D, heads, 0.0).to(dtype)
    blk.load_state_dict({n: torch.as_tensor(sd[n]).to(dtype) for n in PARAMS})
    blk = blk.to(device)
    if m1 is not None:
        t1, t2 = (torch.as_tensor(np.asarray(m), dtype=dtype, device=device) for m in (m1, m2))

        class _Mul(torch.nn.Module):
            def __init__(self, m):
                super().__init__()
                self.m = m

            def forward(self, a):
                return a * self.m

        blk.dropout1, blk.dropout2 = _Mul(t1), _Mul(t2)
    xt = torch.as_tensor(x, dtype=dtype, device=device).clone().requires_grad_(True)
    mask = torch.tril(torch.ones(1, 1, T, T, dtype=torch.int32, device=device))
    out = blk(xt, mask)
    out.backward(torch.as_tensor(gout, dtype=dtype, device=device))
    return (out.detach().cpu().numpy(), xt.grad.cpu().numpy(), {n: p.grad.cpu().numpy() for n, p in blk.named_parameters()})
