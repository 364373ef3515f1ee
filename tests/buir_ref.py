"""Float64 restatements for the BUIR tests: the bootstrap loss (reference src/models/general/BUIR.py:76-97) with its closed-form
gradients (K16, wr_buir_loss_grad), the momentum update of the target tables (:69-74; K17, wr_ema_update), a five-step Adam run
with that update after every step, plus the cases, figures and tolerances of those tests.  A helper module, not a conftest.

For sample k with online rows x_u, x_i, target rows t_u, t_i, p = W x + b and z^ = z / max(|z|, 1e-12):
    l_k = 4 - 2 <p_u^, t_i^> - 2 <p_i^, t_u^>,   loss = mean l_k
    g_pu = (-2/B) (t_i^ - p_u^ <p_u^, t_i^>) / |p_u|   (g_pi likewise),   g_xu = W^T g_pu
    gW = sum_k g_pu x_u^T + g_pi x_i^T,   gb = sum_k g_pu + g_pi
Targets are constants.

Figures: max |a - b| / max |b| per array; the loss relatively.  Tolerances by DESIGN section 2's rule: the floor of a figure is
the stock fp32 torch path against the float64 restatement on a CPU.
  TOL      8 x the largest floor of any figure over CASES, rounded up to one digit: the kernel's outputs, the model's gradients
           and the full_predict scores
  RUN_TOL  the same rule for the five-step Adam runs of the golden file, per figure: the loss curve, and the UPDATE
           (after - before, relative to the largest update of the float64 run) of the online and of the target tables.  Adam
           divides a gradient by its own running size, so an element's update carries that element's RELATIVE gradient error,
           which for the small elements of a row is far above the row's max-normalised error: the run has its own floor.
tests/test_buir_contract.py re-measures every floor and asserts 4 x floor < tolerance.
"""
import numpy as np

EPS = 1e-12
N_USERS, N_ITEMS = 50, 70

# (tag, B, D, kind)
CASES = [("B1", 1, 64, "plain"), ("ragged", 33, 32, "plain"), ("two_wg", 129, 64, "plain"), ("d128", 300, 128, "plain"),
         ("one_pair", 64, 64, "one_pair"), ("few_ids", 96, 64, "few_ids"), ("x1e3", 96, 64, "x1e3"), ("x1e-3", 96, 64, "x1e-3"),
         ("zero_target", 40, 64, "zero_target")]
FIGS = ("loss", "gU", "gI", "gW", "gb")

# Largest floor of each figure over CASES: stock fp32 torch ops on a CPU against float64.
FLOORS = {"loss": 6.1e-8, "gU": 5.7e-7, "gI": 4.9e-7, "gW": 5.0e-7, "gb": 1.6e-7}
TOL = 5e-6                                       # 8 x the largest of them (4.6e-6), rounded up to one digit
LOSS_TOL = 1e-5                                  # the loss against the golden file, relative
# Five Adam steps on the golden batch, fp32 against float64 on a CPU: the larger of runs (a) and (b) for the loss curve and the
# online tables; the target tables on run (b) alone — in run (a) they move by 7.5e-5 against a table of 0.46, the fp32 floor of
# that move is 2e-3 of it, and no update can be judged there (run (b): a move of 1.3e-2)
RUN_FLOORS = {"losses": 1.2e-7, "online_update": 7.7e-6, "target_update": 6.8e-6}
RUN_TOL = {"losses": 1e-6, "online_update": 7e-5, "target_update": 6e-5}
RUNS = {"a": (0.995, 1e-3), "b": (0.9, 1e-2)}    # momentum, lr
TABLES = ["user_online.weight", "user_target.weight", "item_online.weight", "item_target.weight"]

WRONG = ["norm_constant", "online_for_target", "gb_user_half"]
RUN_WRONG = ["momentum_swapped", "no_target_update"]


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / den) if den > 0 else float(np.abs(a - b).max())


# ------------------------------------------------------------------------------------------------ inputs
def make_case(i):
    """-> dict(Uo, Io, Ut, It [n, D], W [D, D], b [D] fp32; users, items int64 [B]) of CASES[i].  Tables as BUIR initialises them
    (xavier_normal_; bias std 1), the targets a momentum's distance from the online tables."""
    tag, B, D, kind = CASES[i]
    rng = np.random.RandomState(8100 + i)

    def xavier(n, d):
        return (rng.standard_normal((n, d)) * np.sqrt(2.0 / (n + d))).astype(np.float32)

    Uo, Io = xavier(N_USERS, D), xavier(N_ITEMS, D)
    Ut = (Uo + 0.3 * xavier(N_USERS, D)).astype(np.float32)
    It = (Io + 0.3 * xavier(N_ITEMS, D)).astype(np.float32)
    W, b = xavier(D, D), rng.standard_normal(D).astype(np.float32)
    users = rng.randint(0, N_USERS, size=B).astype(np.int64)
    items = rng.randint(0, N_ITEMS, size=B).astype(np.int64)
    if kind == "one_pair":
        users[:], items[:] = 7, 11
    elif kind == "few_ids":
        users = rng.permutation(N_USERS)[:8][rng.randint(0, 8, size=B)].astype(np.int64)
        items = rng.permutation(N_ITEMS)[:12][rng.randint(0, 12, size=B)].astype(np.int64)
    elif kind in ("x1e3", "x1e-3"):
        s = np.float32(1e3 if kind == "x1e3" else 1e-3)
        Uo, Io, Ut, It = Uo * s, Io * s, Ut * s, It * s
    elif kind == "zero_target":
        It[items[0]] = 0.0
        Ut[users[1]] = 0.0
    return {"Uo": Uo, "Io": Io, "Ut": Ut, "It": It, "W": W, "b": b, "users": users, "items": items}


# ------------------------------------------------------------------------------------------------ the loss in float64
def _normalize(z):
    return z / np.maximum(np.sqrt((z * z).sum(1, keepdims=True)), EPS)


def buir_f64(case, wrong=None):
    """-> dict(loss, terms [B], gU / gI [B, D] per-sample rows, gW, gb, dU / dI dense table gradients) in float64.  `wrong` builds
    deliberately WRONG gradients: 'norm_constant' (the norm of p a constant of the backward), 'online_for_target' (the online row
    where the target row belongs), 'gb_user_half' (gb without the item half)."""
    f = np.float64
    Uo, Io, Ut, It, W, b = (np.asarray(case[k], f) for k in ("Uo", "Io", "Ut", "It", "W", "b"))
    users, items = np.asarray(case["users"]).reshape(-1), np.asarray(case["items"]).reshape(-1)
    B = users.size
    xu, xi = Uo[users], Io[items]
    tu, ti = (Uo[users], Io[items]) if wrong == "online_for_target" else (Ut[users], It[items])
    th_u, th_i = _normalize(tu), _normalize(ti)

    def half(x, th):
        p = x @ W.T + b
        nrm = np.sqrt((p * p).sum(1, keepdims=True))
        ph = p / np.maximum(nrm, EPS)
        c = (ph * th).sum(1, keepdims=True)
        proj = 0.0 if wrong == "norm_constant" else ph * c
        return c[:, 0], (-2.0 / B) * (th - proj) / np.maximum(nrm, EPS)

    c_ui, g_pu = half(xu, th_i)
    c_iu, g_pi = half(xi, th_u)
    terms = 4.0 - 2.0 * c_ui - 2.0 * c_iu
    gU, gI = g_pu @ W, g_pi @ W
    dU, dI = np.zeros_like(Uo), np.zeros_like(Io)
    np.add.at(dU, users, gU)
    np.add.at(dI, items, gI)
    gb = g_pu.sum(0) if wrong == "gb_user_half" else (g_pu + g_pi).sum(0)
    return {"loss": float(terms.mean()), "terms": terms, "gU": gU, "gI": gI, "gW": g_pu.T @ xu + g_pi.T @ xi, "gb": gb,
            "dU": dU, "dI": dI}


def stock_torch(case, dtype=None, device="cpu"):
    """the reference formula typed again on stock torch ops under autograd (BUIR.py:76-97), the gathered online rows as leaves
    -> the dict of buir_f64 (without terms)"""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float32
    t = {k: torch.as_tensor(case[k], device=device) for k in case}
    for k in ("Uo", "Io", "Ut", "It", "W", "b"):
        t[k] = t[k].to(dtype)
    Uo, Io = t["Uo"].clone().requires_grad_(True), t["Io"].clone().requires_grad_(True)
    W, b = t["W"].clone().requires_grad_(True), t["b"].clone().requires_grad_(True)
    xu, xi = Uo[t["users"]], Io[t["items"]]
    xu.retain_grad()
    xi.retain_grad()
    u_online = F.normalize(F.linear(xu, W, b), dim=-1)
    i_online = F.normalize(F.linear(xi, W, b), dim=-1)
    u_target = F.normalize(t["Ut"][t["users"]], dim=-1)
    i_target = F.normalize(t["It"][t["items"]], dim=-1)
    loss_ui = 2 - 2 * (u_online * i_target.detach()).sum(dim=-1)
    loss_iu = 2 - 2 * (i_online * u_target.detach()).sum(dim=-1)
    loss = (loss_ui + loss_iu).mean()
    loss.backward()
    n = lambda z: z.detach().cpu().numpy()    # noqa: E731
    return {"loss": float(loss.detach()), "gU": n(xu.grad), "gI": n(xi.grad), "gW": n(W.grad), "gb": n(b.grad), "dU": n(Uo.grad),
            "dI": n(Io.grad)}


def figures(got, ref):
    fig = {"loss": abs(got["loss"] - ref["loss"]) / abs(ref["loss"])}
    for k in ("gU", "gI", "gW", "gb"):
        fig[k] = rel_err(got[k], ref[k])
    return fig


def fmt(tag, fig, tol=None):
    tol = TOL if tol is None else tol
    return "parity buir %s: " % tag + " ".join("%s %.2e" % (k, fig[k]) for k in FIGS if k in fig) + " (tol %.0e)" % tol


# ------------------------------------------------------------------------------------------------ the momentum update
def ema_f64(t, o, m, wrong=None):
    """t m + o (1 - m) in float64.  `wrong`: 'momentum_swapped' (t (1 - m) + o m), 'no_target_update' (t)"""
    t, o = np.asarray(t, np.float64), np.asarray(o, np.float64)
    if wrong == "no_target_update":
        return t.copy()
    if wrong == "momentum_swapped":
        return t * (1. - m) + o * m
    return t * m + o * (1. - m)


def ema_fp32(t, o, m):
    """the reference's expression on fp32 NumPy arrays with fp32 scalars: two rounded products, one rounded sum"""
    t, o = np.asarray(t, np.float32), np.asarray(o, np.float32)
    return (t * np.float32(m) + o * np.float32(1. - m)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the Adam run
def adam_run(sd, users, items, momentum, lr, steps=5, dtype=None, wrong=None):
    """`steps` Adam steps on one batch with the target update after each, the reference formula typed again on stock torch ops
    (CPU) in `dtype` -> (losses [steps], {table name: final table}).  sd: name -> array, the names of the model's state dict.
    `wrong` as ema_f64."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    p = {k: torch.as_tensor(np.asarray(sd[k])).to(dtype).clone() for k in TABLES + ["predictor.weight", "predictor.bias"]}
    train = ["user_online.weight", "item_online.weight", "predictor.weight", "predictor.bias"]
    for k in train:
        p[k].requires_grad_(True)
    uu, ii = torch.as_tensor(np.asarray(users)), torch.as_tensor(np.asarray(items))
    opt = torch.optim.Adam([p[k] for k in train], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        W, b = p["predictor.weight"], p["predictor.bias"]
        u_online = F.normalize(F.linear(p["user_online.weight"][uu], W, b), dim=-1)
        i_online = F.normalize(F.linear(p["item_online.weight"][ii], W, b), dim=-1)
        u_target = F.normalize(p["user_target.weight"][uu], dim=-1)
        i_target = F.normalize(p["item_target.weight"][ii], dim=-1)
        loss = ((2 - 2 * (u_online * i_target).sum(dim=-1)) + (2 - 2 * (i_online * u_target).sum(dim=-1))).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        with torch.no_grad():
            for o, t in (("user_online.weight", "user_target.weight"), ("item_online.weight", "item_target.weight")):
                if wrong == "no_target_update":
                    continue
                if wrong == "momentum_swapped":
                    p[t] = p[t] * (1. - momentum) + p[o].detach() * momentum
                else:
                    p[t] = p[t] * momentum + p[o].detach() * (1. - momentum)
    return np.asarray(losses, np.float64), {k: p[k].detach().numpy().copy() for k in TABLES}


def run_figures(losses, tables, before, ref_losses, ref_tables):
    """figures of a run against a reference run from the same initial tables `before`: the loss curve relatively, the online and
    the target tables on their UPDATE (after - before) relative to the reference's largest update of that table"""
    fig = {"losses": float(np.max(np.abs(np.asarray(losses, np.float64) - ref_losses) / np.abs(ref_losses))),
           "online_update": 0.0, "target_update": 0.0}
    for k in TABLES:
        b0 = np.asarray(before[k], np.float64)
        e = rel_err(np.asarray(tables[k], np.float64) - b0, np.asarray(ref_tables[k], np.float64) - b0)
        key = "target_update" if "target" in k else "online_update"
        fig[key] = max(fig[key], e)
    return fig


def run_fmt(tag, fig):
    return "parity buir run %s: " % tag + " ".join("%s %.2e (tol %.0e)" % (k, fig[k], RUN_TOL[k]) for k in RUN_TOL)
