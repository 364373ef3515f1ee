"""Float64 restatements of hip_ops.gru_seq (wr_gru.hip, K27's whole-sequence form) and hip_ops.narm_pool (wr_narm.hip, K28), of
NARM's BPR loss through both (whisprrec_amd/narm.py), and the shapes, length patterns, figures and tolerances of their tests.  A
helper module, not a conftest.  The GRU cell's last-state form, the length patterns and rel_err are gru_ref's.

    gru_seq:    hs[b, t] = the GRU's state after step t for t < len_b, ZERO for t >= len_b;  len_b = clamp(lengths[b], 0, T)
                backward: g_hs[b, t] enters dh before step t's gate gradients for t < len_b only; g_last [B, H] (optional) is a
                gradient of the state after step len_b - 1 on top.  x and g_hs are never read at t >= len_b.
    narm_pool:  q = A1 h_g[b]   u_t = q + A2 hs[b, t]   e_t = v . sigmoid(u_t)   c[b] = sum_{t < len_b} e_t hs[b, t]   (no softmax)
                hs is never read at t >= len_b.

Figures: max |a - b| / max |b| per array (gru_ref.rel_err).  Groups of gru_seq: `hs`, `gx`, `gw` (g_w_ih, g_w_hh), `gb`; of the
pooling: `c`, `gh` (g_hs, g_h_g), `gA` (g_A1, g_A2, g_v); of the model: `loss`, `grad` (every parameter's gradient, each against
its own largest magnitude).

Tolerances: DESIGN section 2's rule.  The floor of a group is the stock fp32 torch path (what the flags leave when off: nn.GRU
over the padded batch times the mask, the torch pooling with the mask arange(T) < lengths, under autograd) against this
restatement on a CPU, the largest over the cases; TOL = 8 x floor, rounded up to one digit.  tests/test_narm_contract.py
re-measures the floors and asserts 4 x floor < TOL.
"""
import numpy as np

import gru_ref as G

PATTERNS = G.PATTERNS
rel_err = G.rel_err


def _worst(fig, group_of, groups):
    w = {g: 0.0 for g in groups}
    for n, v in fig.items():
        w[group_of[n]] = max(w[group_of[n]], v)
    return w


def _fmt(kind, tag, w, tol, groups):
    return "parity narm %s %s: " % (kind, tag) + " ".join("%s %.2e (tol %.0e)" % (g, w[g], tol[g]) for g in groups)


# ------------------------------------------------------------------------------------------------ gru_seq: cases and tolerances
SEQ_SHAPES = G.SHAPES                          # (B, T, E, H)
SEQ_WALK_SHAPE = (4100, 5, 64, 32)             # 257 tiles of 16 rows on the 256 workgroups of the backward; "mixed" only
SEQ_GROUPS = ("hs", "gx", "gw", "gb")
SEQ_GROUP_OF = {"hs": "hs", "gx": "gx", "gwih": "gw", "gwhh": "gw", "gbih": "gb", "gbhh": "gb"}
SEQ_WRONGS = ("ghs_dropped_at_last", "ghs_applied_at_len")

# Largest floor of each group over SEQ_SHAPES x PATTERNS, each with and without g_last, and the walk shape: stock fp32 against
# float64 on a CPU (measure_seq_floors() below; `python tests/narm_ref.py` prints every case).
SEQ_FLOORS = {"hs": 3.98e-7, "gx": 4.15e-7, "gw": 4.98e-7, "gb": 2.32e-7}
SEQ_TOL = {"hs": 4e-6, "gx": 4e-6, "gw": 4e-6, "gb": 2e-6}                      # 8 x floor, rounded up to one digit


def make_seq_case(i, pattern, walk=False):
    """gru_ref.make_case's inputs (SEQ_SHAPES[i], or the walk shape) plus ghs [B, T, H], which is NOT zero past the lengths:
    nothing may read it there"""
    c = G.make_case(G.WALK_SHAPES.index(SEQ_WALK_SHAPE), pattern, G.WALK_SHAPES, G.WALK_SEED) if walk else G.make_case(i, pattern)
    B, T, _ = c["x"].shape
    rng = np.random.RandomState(77100 + 10 * (99 if walk else i) + PATTERNS.index(pattern))
    c["ghs"] = rng.standard_normal((B, T, c["whh"].shape[1])).astype(np.float32)
    return c


def gru_seq_f64(x, lengths, wih, whh, bih, bhh, ghs=None, glast=None, wrong=None):
    """-> dict(hs [B, T, H], zero past the lengths, and, with ghs, gx, gwih, gwhh, gbih, gbhh).  `wrong` (SEQ_WRONGS) builds
    deliberately WRONG gradients for the power checks."""
    f = np.float64
    x, wih, whh, bih, bhh = (np.asarray(a, f) for a in (x, wih, whh, bih, bhh))
    B, T, E = x.shape
    H = whh.shape[1]
    n = np.clip(np.asarray(lengths, np.int64), 0, T)
    live = np.arange(T)[None, :] < n[:, None]
    x = np.where(live[:, :, None], x, 0.0)                                 # the padding is never read
    h, hs, keep = np.zeros((B, H), f), np.zeros((B, T, H), f), []
    for t in range(T):
        gi, gh = x[:, t] @ wih.T + bih, h @ whh.T + bhh
        r, z = G._sig(gi[:, :H] + gh[:, :H]), G._sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        cand = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        keep.append((r, z, cand, gh[:, 2 * H:], h))
        h = np.where(live[:, t, None], (1 - z) * cand + z * h, h)
        hs[:, t] = np.where(live[:, t, None], h, 0.0)
    out = {"hs": hs}
    if ghs is None:
        return out
    raw = np.asarray(ghs, f)
    g = np.where(live[:, :, None], raw, 0.0)                               # nor is the padding of g_hs
    dh = np.zeros((B, H), f) if glast is None else np.asarray(glast, f).copy()
    if wrong == "ghs_dropped_at_last":
        rows = np.nonzero(n > 0)[0]
        g[rows, n[rows] - 1] = 0.0
    if wrong == "ghs_applied_at_len":                                      # the padded step's gradient reaches the frozen state
        rows = np.nonzero(n < T)[0]
        dh[rows] += raw[rows, n[rows]]
    gx = np.zeros((B, T, E), f)
    gwih, gwhh, gbih, gbhh = np.zeros_like(wih), np.zeros_like(whh), np.zeros(3 * H, f), np.zeros(3 * H, f)
    for t in range(T - 1, -1, -1):
        r, z, cand, ghn, hp = keep[t]
        m = live[:, t, None]
        dh = dh + g[:, t]
        d_ain = dh * (1 - z) * (1 - cand * cand) * m
        d_ahn = d_ain * r
        d_ar = d_ain * ghn * r * (1 - r)
        d_az = dh * (hp - cand) * z * (1 - z) * m
        dgi, dgh = np.concatenate([d_ar, d_az, d_ain], 1), np.concatenate([d_ar, d_az, d_ahn], 1)
        gx[:, t] = dgi @ wih
        gwih += dgi.T @ x[:, t]
        gwhh += dgh.T @ hp
        gbih += dgi.sum(0)
        gbhh += dgh.sum(0)
        dh = np.where(m, dh * z + dgh @ whh, dh)
    out.update(gx=gx, gwih=gwih, gwhh=gwhh, gbih=gbih, gbhh=gbhh)
    return out


def seq_case_f64(c, with_last=False, wrong=None):
    return gru_seq_f64(c["x"], c["lengths"], c["wih"], c["whh"], c["bih"], c["bhh"], c["ghs"], c["glast"] if with_last else None,
                       wrong=wrong)


def seq_stock(c, with_last=False, dtype=None):
    """nn.GRU over the padded batch, its output times the mask (pad_packed_sequence's form), under torch.autograd for ghs (and
    glast on the row at lengths - 1) -> dict(hs, gx, gwih, gwhh, gbih, gbhh)"""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    rnn = G.torch_gru(c, dtype)
    x = torch.as_tensor(c["x"], dtype=dtype).clone().requires_grad_(True)
    lengths = torch.as_tensor(c["lengths"])
    T = x.shape[1]
    output, _ = rnn(x)
    mask = (torch.arange(T)[None, :] < lengths[:, None]).to(dtype)[:, :, None]
    hs = output * mask
    obj = (hs * torch.as_tensor(c["ghs"], dtype=dtype)).sum()
    if with_last:
        obj = obj + (output[torch.arange(x.shape[0]), lengths - 1, :] * torch.as_tensor(c["glast"], dtype=dtype)).sum()
    obj.backward()
    return {"hs": hs.detach().numpy(), "gx": x.grad.numpy(), "gwih": rnn.weight_ih_l0.grad.numpy(),
            "gwhh": rnn.weight_hh_l0.grad.numpy(), "gbih": rnn.bias_ih_l0.grad.numpy(), "gbhh": rnn.bias_hh_l0.grad.numpy()}


def seq_figures(got, ref):
    return {n: rel_err(got[n], ref[n]) for n in SEQ_GROUP_OF}


def seq_worst(fig):
    return _worst(fig, SEQ_GROUP_OF, SEQ_GROUPS)


def seq_fmt(tag, fig):
    return _fmt("gru_seq", tag, seq_worst(fig), SEQ_TOL, SEQ_GROUPS)


SEQ_CASES = [(i, pat, False) for i in range(len(SEQ_SHAPES)) for pat in PATTERNS] + [(0, "mixed", True)]


def seq_id(key):
    i, pat, walk = key
    return "%s-%s" % ("x".join(map(str, SEQ_WALK_SHAPE if walk else SEQ_SHAPES[i])), pat)


def measure_seq_floors(cases=None):
    floors, per = {g: 0.0 for g in SEQ_GROUPS}, {}
    for key in (SEQ_CASES if cases is None else cases):
        c = make_seq_case(*key)
        for with_last in (False, True):
            w = seq_worst(seq_figures(seq_stock(c, with_last), seq_case_f64(c, with_last)))
            per[key + (with_last,)] = w
            for g in SEQ_GROUPS:
                floors[g] = max(floors[g], w[g])
    return floors, per


# ------------------------------------------------------------------------------------------------ the pooling
# (B, T, H, A): one row and one step; fewer rows than a workgroup's waves; T no multiple of the chunk 64 / A; every A and H; more
# rows than the 64 workgroups x 4 waves of the kernels hold at a time (the last: a wave takes 4 - 5 rows, T below a chunk)
POOL_SHAPES = [(1, 1, 64, 16), (5, 3, 32, 16), (17, 20, 64, 32), (67, 20, 32, 64), (130, 50, 64, 16), (1029, 3, 64, 16)]
POOL_ROWS = 4 * 64                             # kNarmWaves * kNarmWg: rows in flight; one slab of parameter gradients each
POOL_GROUPS = ("c", "gh", "gA")
POOL_GROUP_OF = {"c": "c", "ghs": "gh", "ghg": "gh", "gA1": "gA", "gA2": "gA", "gv": "gA"}
POOL_WRONGS = ("mask_off_by_one", "swap_A1_A2", "no_sigma_prime")

# Largest floor of each group over POOL_SHAPES x PATTERNS, the stock fp32 torch pooling under autograd against float64 on a CPU
# (measure_pool_floors() below).
POOL_FLOORS = {"c": 2.06e-7, "gh": 4.53e-7, "gA": 5.80e-7}
POOL_TOL = {"c": 2e-6, "gh": 4e-6, "gA": 5e-6}                                 # 8 x floor, rounded up to one digit


def make_pool_case(i, pattern):
    """-> dict(hs [B, T, H], hg [B, H], lengths, A1, A2 [A, H], v [A], gc [B, H]) of POOL_SHAPES[i], fp32.  hs is NOT zero past
    the lengths: nothing may read it there."""
    B, T, H, A = POOL_SHAPES[i]
    rng = np.random.RandomState(55100 + 10 * i + PATTERNS.index(pattern))
    f = lambda *s: rng.standard_normal(s)                   # noqa: E731
    c = {"hs": np.tanh(f(B, T, H)), "hg": np.tanh(f(B, H)), "A1": f(A, H) * (2 / np.sqrt(H)), "A2": f(A, H) * (2 / np.sqrt(H)),
         "v": f(A) / np.sqrt(A), "gc": f(B, H)}
    c = {n: a.astype(np.float32) for n, a in c.items()}
    c["lengths"] = G.make_lengths(pattern, B, T, rng)
    return c


def pool_f64(hs, hg, lengths, A1, A2, v, gc=None, wrong=None):
    """-> dict(c [B, H] and, with gc, ghs [B, T, H], ghg [B, H], gA1, gA2 [A, H], gv [A]).  `wrong` (POOL_WRONGS) builds
    deliberately WRONG results."""
    f = np.float64
    hs, hg, A1, A2, v = (np.asarray(a, f) for a in (hs, hg, A1, A2, v))
    B, T, H = hs.shape
    n = np.clip(np.asarray(lengths, np.int64), 0, T)
    if wrong == "mask_off_by_one":
        n = np.minimum(n + 1, T)
    if wrong == "swap_A1_A2":
        A1, A2 = A2, A1
    mask = np.arange(T)[None, :] < n[:, None]
    hs = np.where(mask[:, :, None], hs, 0.0)                               # the padding is never read
    s = G._sig((hg @ A1.T)[:, None, :] + hs @ A2.T)                        # [B, T, A]
    e = (s @ v) * mask
    out = {"c": (e[:, :, None] * hs).sum(1)}
    if gc is None:
        return out
    gc = np.asarray(gc, f)
    de = np.einsum("bth,bh->bt", hs, gc) * mask
    du = de[:, :, None] * v[None, None, :] * (1.0 if wrong == "no_sigma_prime" else s * (1 - s))
    dq = du.sum(1)
    out.update(ghs=(e[:, :, None] * gc[:, None, :] + du @ A2) * mask[:, :, None], ghg=dq @ A1, gA1=dq.T @ hg,
               gA2=np.einsum("bta,bth->ah", du, hs), gv=(de[:, :, None] * s).sum((0, 1)))
    return out


def pool_case_f64(c, wrong=None):
    return pool_f64(c["hs"], c["hg"], c["lengths"], c["A1"], c["A2"], c["v"], c["gc"], wrong=wrong)


def torch_pool(hs, hg, lengths, A1, A2, v):
    """the pooling as --pool_native 0 runs it, on torch tensors (A1, A2 [A, H], v [A])"""
    import torch
    T = hs.shape[1]
    u = (hg @ A1.t())[:, None, :] + hs @ A2.t()
    e = torch.sigmoid(u) @ v
    e = e * (torch.arange(T, device=hs.device)[None, :] < lengths[:, None]).to(e.dtype)
    return (e[:, :, None] * hs).sum(dim=1)


def pool_stock(c, dtype=None):
    import torch
    dtype = torch.float32 if dtype is None else dtype
    t = {n: torch.as_tensor(c[n], dtype=dtype).clone().requires_grad_(True) for n in ("hs", "hg", "A1", "A2", "v")}
    out = torch_pool(t["hs"], t["hg"], torch.as_tensor(c["lengths"]), t["A1"], t["A2"], t["v"])
    out.backward(torch.as_tensor(c["gc"], dtype=dtype))
    res = {"c": out.detach().numpy()}
    res.update({"g" + n: t[n].grad.numpy() for n in t})
    return res


def pool_figures(got, ref):
    return {n: rel_err(got[n], ref[n]) for n in POOL_GROUP_OF}


def pool_worst(fig):
    return _worst(fig, POOL_GROUP_OF, POOL_GROUPS)


def pool_fmt(tag, fig):
    return _fmt("pool", tag, pool_worst(fig), POOL_TOL, POOL_GROUPS)


POOL_CASES = [(i, pat) for i in range(len(POOL_SHAPES)) for pat in PATTERNS]


def pool_id(key):
    return "%s-%s" % ("x".join(map(str, POOL_SHAPES[key[0]])), key[1])


def measure_pool_floors(cases=None):
    floors, per = {g: 0.0 for g in POOL_GROUPS}, {}
    for key in (POOL_CASES if cases is None else cases):
        c = make_pool_case(*key)
        w = pool_worst(pool_figures(pool_stock(c), pool_case_f64(c)))
        per[key] = w
        for g in POOL_GROUPS:
            floors[g] = max(floors[g], w[g])
    return floors, per


# ------------------------------------------------------------------------------------------------ the model
MODEL_GROUPS = ("loss", "grad")
# The floors of NARM's BPR loss and of its parameters' gradients: the flag-off fp32 model on a CPU against narm_f64, on
# model_batch()'s rows at (E, H, A) in MODEL_DIMS, item embeddings scaled by 8 (the gates leave their linear range).
MODEL_DIMS = [(64, 64, 16), (32, 64, 32), (64, 32, 64)]
MODEL_FLOORS = {"loss": 9.3e-8, "grad": 7.4e-7}                             # loss and grad both peak at (64, 64, 16)
MODEL_TOL = {"loss": 8e-7, "grad": 6e-6}                                      # 8 x floor, rounded up to one digit


def model_batch(n_items, B=64, T=20, seed=5):
    """left-aligned zero-padded histories [B, T], lengths (row 0: T, row 1: 1), one positive and one negative item per row"""
    rng = np.random.RandomState(seed)
    lengths = rng.randint(1, T + 1, B).astype(np.int64)
    lengths[:2] = [T, 1]
    hist = rng.randint(1, n_items, (B, T)) * (np.arange(T)[None, :] < lengths[:, None])
    return {"history_items": hist.astype(np.int64), "lengths": lengths, "pos_item": rng.randint(1, n_items, B).astype(np.int64),
            "neg_items": rng.randint(1, n_items, (B, 1)).astype(np.int64)}


def narm_f64(sd, batch, wrong=None):
    """NARM's BPR loss and the gradient of every parameter, from a state_dict of numpy arrays -> (loss, {name: gradient})"""
    f = np.float64
    sd = {n: np.asarray(a, f) for n, a in sd.items()}
    hist, lengths = batch["history_items"], batch["lengths"]
    pos, neg = batch["pos_item"], batch["neg_items"].reshape(-1)
    emb, w_out = sd["item_embedding.weight"], sd["out.weight"]
    B, T = hist.shape
    H = sd["encoder_g.weight_hh_l0"].shape[1]
    pg = [sd["encoder_g.%s_l0" % n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    pl = [sd["encoder_l.%s_l0" % n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    A1, A2, v = sd["A1.weight"], sd["A2.weight"], sd["attention_out.weight"].reshape(-1)
    x = emb[hist]
    h_g = G.gru_f64(x, lengths, *pg)["h"]
    hs_l = gru_seq_f64(x, lengths, *pl)["hs"]
    c_l = pool_f64(hs_l, h_g, lengths, A1, A2, v)["c"]
    cat = np.concatenate([c_l, h_g], 1)
    user = cat @ w_out.T
    pe, ne = emb[pos], emb[neg]
    s = G._sig((user * pe).sum(1) - (user * ne).sum(1))
    loss = float(-np.log(1e-10 + s).mean())
    dd = -(s * (1 - s) / (1e-10 + s)) / B                                   # d loss / d (pos - neg)
    d_user = dd[:, None] * (pe - ne)
    g = {"out.weight": d_user.T @ cat}
    d_cat = d_user @ w_out
    pool = pool_f64(hs_l, h_g, lengths, A1, A2, v, d_cat[:, :H], wrong=wrong)
    g.update({"A1.weight": pool["gA1"], "A2.weight": pool["gA2"], "attention_out.weight": pool["gv"][None, :]})
    loc = gru_seq_f64(x, lengths, *pl, ghs=pool["ghs"])
    glo = G.gru_f64(x, lengths, *pg, glast=d_cat[:, H:] + pool["ghg"])
    for enc, r in (("encoder_l", loc), ("encoder_g", glo)):
        g.update({"%s.weight_ih_l0" % enc: r["gwih"], "%s.weight_hh_l0" % enc: r["gwhh"], "%s.bias_ih_l0" % enc: r["gbih"],
                  "%s.bias_hh_l0" % enc: r["gbhh"]})
    ge = np.zeros_like(emb)
    np.add.at(ge, hist.reshape(-1), (loc["gx"] + glo["gx"]).reshape(B * T, -1))      # zero rows past the lengths go to row 0
    np.add.at(ge, pos, dd[:, None] * user)
    np.add.at(ge, neg, -dd[:, None] * user)
    ge[0] = 0.0                                                              # the padding row takes no gradient
    g["item_embedding.weight"] = ge
    return loss, g


def model_figures(loss, grads, ref_loss, ref_grads):
    """-> ({"loss":, "grad":}, {name: figure})"""
    per = {n: rel_err(grads[n], ref_grads[n]) for n in ref_grads}
    return {"loss": abs(loss - ref_loss) / abs(ref_loss), "grad": max(per.values())}, per


def model_fmt(tag, w, tol=None):
    return _fmt("model", tag, w, MODEL_TOL if tol is None else tol, MODEL_GROUPS)


if __name__ == "__main__":
    fl, per = measure_seq_floors()
    for key, w in per.items():
        print("gru_seq", seq_id(key[:3]), "g_last" if key[3] else "-", " ".join("%s %.2e" % (g, w[g]) for g in SEQ_GROUPS))
    print("gru_seq floors", fl)
    fl, per = measure_pool_floors()
    for key, w in per.items():
        print("pool", pool_id(key), " ".join("%s %.2e" % (g, w[g]) for g in POOL_GROUPS))
    print("pool floors", fl)
