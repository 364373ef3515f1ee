"""Float64 restatement of hip_ops.gru_last (wr_gru.hip, K27; whisprrec_amd/gru4rec.py) with its five gradients, and the shapes,
length patterns, figures and tolerances of the K27 tests.  A helper module, not a conftest.

    r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)       z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
    n = tanh(W_in x + b_in + r * (W_hn h + b_hn))    h' = (1 - z) * n + z * h,   h_0 = 0     (torch's cell, gates r, z, n)
    row b takes its first len_b = clamp(lengths[b], 0, T) steps; h_last[b] is its state after them; x[b, t >= len_b] is not read

Figures: max |a - b| / max |b| per array (0 where both are exactly zero).  Groups: `h` (h_last), `gx`, `gw` (g_w_ih, g_w_hh),
`gb` (g_b_ih, g_b_hh); each array against the largest magnitude of its float64 counterpart.

Tolerances: DESIGN section 2's rule.  The floor of a group is the stock fp32 path (nn.GRU over the padded batch, the row at
lengths - 1, under autograd: what --gru_native 0 runs) against this restatement on a CPU; FLOORS holds the largest floor over
SHAPES x PATTERNS; TOL = 8 x that, rounded up to one digit.  tests/test_gru4rec_contract.py re-measures the floors and asserts
4 x floor < TOL.  WALK_SHAPES (more 16-row tiles than the kernels' workgroup caps: a workgroup takes several tiles) has
WALK_FLOORS / WALK_TOL of its own, by the same rule.
"""
import numpy as np

# (B, T, E, H): B on both sides of row tiles of 16, 32 and 64; T = 1 has no recurrent step; every E / H pairing
SHAPES = [(1, 1, 64, 64), (5, 3, 32, 32), (17, 20, 64, 32), (33, 20, 32, 64), (67, 20, 64, 64), (130, 50, 64, 64)]
PATTERNS = ("ones", "full", "mixed")       # all lengths 1; all T; uniform in [1, T] with row 0 = 1 and row 1 = T

GROUPS = ("h", "gx", "gw", "gb")
GROUP_OF = {"h": "h", "gx": "gx", "gwih": "gw", "gwhh": "gw", "gbih": "gb", "gbhh": "gb"}
WRONGS = ("bhn_outside", "swap_z", "late_last", "gbhh_no_n", "gwhh_tile_row", "gx_last_missing")

# Largest floor of each group over SHAPES x PATTERNS, stock fp32 nn.GRU + select under autograd against float64 on a CPU
# (measure_floors() below; `python tests/gru_ref.py` prints every case).  The figures were the same in repeated runs.  h peaks
# at (130, 50, 64, 64) "ones", gx at (67, 20, 64, 64) "mixed", gw at (33, 20, 32, 64) "mixed", gb at (130, 50, 64, 64) "full".
FLOORS = {"h": 3.3e-7, "gx": 3.3e-7, "gw": 6.0e-7, "gb": 5.6e-7}
TOL = {"h": 3e-6, "gx": 3e-6, "gw": 5e-6, "gb": 5e-6}                       # 8 x floor, rounded up to one digit

# The caps of wr_gru.hip restated, in rows: a workgroup takes the 16-row tiles tile, tile + cap, ... once B exceeds cap x 16 rows.
TILE = 16                   # kGruRows
FWD_ROWS = TILE * 1024      # kGruRows * kGruFwdWg
BWD_ROWS = TILE * 256       # kGruRows * kGruBwdWg: the workgroups of the backward carry the parameter-gradient partials

# Shapes at which a workgroup visits several tiles.  (8195, 3, 32, 32): 513 tiles on the 256 workgroups of the backward, the last
# tile of 3 rows — every pattern; the others with "mixed" only: (4130, 20, 64, 64) and (4100, 5, 64, 32) give a few workgroups a
# second tile (the last of 2 / 4 rows), (16400, 2, 32, 64) has 1,025 tiles: the forward walks too, the backward 4 - 5 times.
WALK_SHAPES = [(8195, 3, 32, 32), (4130, 20, 64, 64), (4100, 5, 64, 32), (16400, 2, 32, 64)]
WALK_SEED = 19100                             # make_case's seed base of this list (SHAPES: 9100)


def walk_patterns(i):
    return PATTERNS if i == 0 else ("mixed",)


# Largest floor of each group over WALK_SHAPES x walk_patterns, measured as FLOORS is (measure_floors(walk=True))
# — the same in repeated runs.  h and gx peak at (16400, 2, 32, 64), gw at (8195, 3, 32, 32) "full".
WALK_FLOORS = {"h": 3.84e-7, "gx": 4.05e-7, "gw": 3.98e-7, "gb": 1.92e-7}
WALK_TOL = {"h": 4e-6, "gx": 4e-6, "gw": 4e-6, "gb": 2e-6}                  # 8 x floor, rounded up to one digit
# The wrong results of a walk (walk_wrong below), smallest largest-figure / WALK_TOL over the walk cases: later_visits_dropped 2.0e4,
# later_visits_stale 2.3e5, length_of_first_visit 1.7e5 ("mixed" only: with equal lengths it is no mutant), h_carry 9.1e4.


# ------------------------------------------------------------------------------------------------ inputs
def make_lengths(pattern, B, T, rng):
    if pattern == "ones":
        return np.ones(B, np.int64)
    if pattern == "full":
        return np.full(B, T, np.int64)
    n = rng.randint(1, T + 1, B).astype(np.int64)
    n[0] = 1
    if B > 1:
        n[1] = T
    return n


def make_case(i, pattern, shapes=None, seed=9100):
    """-> dict(x [B, T, E], lengths int64 [B], wih [3H, E], whh [3H, H], bih, bhh [3H], glast [B, H]) of SHAPES[i], fp32; x is
    zero at t >= lengths[b] (left-aligned, zero-padded histories); the biases are not zero (scale 0.2).
    shapes / seed: another list (WALK_SHAPES) with its own seed base"""
    B, T, E, H = (SHAPES if shapes is None else shapes)[i]
    rng = np.random.RandomState(seed + 10 * i + PATTERNS.index(pattern))
    f = lambda *s: rng.standard_normal(s)                   # noqa: E731
    c = {"x": f(B, T, E) * 0.5, "wih": f(3 * H, E) / np.sqrt(E), "whh": f(3 * H, H) / np.sqrt(H), "bih": f(3 * H) * 0.2,
         "bhh": f(3 * H) * 0.2, "glast": f(B, H)}
    c = {n: a.astype(np.float32) for n, a in c.items()}
    c["lengths"] = make_lengths(pattern, B, T, rng)
    c["x"] *= (np.arange(T)[None, :] < c["lengths"][:, None])[:, :, None]
    return c


# ------------------------------------------------------------------------------------------------ the GRU in float64
def _sig(a):
    return 1.0 / (1.0 + np.exp(-a))


def gru_f64(x, lengths, wih, whh, bih, bhh, glast=None, wrong=None, h0=None):
    """-> dict(h [B, H], hs [B, T, H] and, with glast, gx, gwih, gwhh, gbih, gbhh).  `wrong` builds deliberately WRONG results for
    the power checks (WRONGS).  h0 [B, H]: a start state other than zero (walk_wrong's 'h_carry' only)."""
    f = np.float64
    x, wih, whh, bih, bhh = (np.asarray(a, f) for a in (x, wih, whh, bih, bhh))
    B, T, E = x.shape
    H = whh.shape[1]
    n_steps = np.clip(np.asarray(lengths, np.int64), 0, T)
    run = np.minimum(n_steps + 1, T) if wrong == "late_last" else n_steps           # steps the row takes
    live = np.arange(T)[None, :] < run[:, None]                                    # [B, T]
    x = np.where((np.arange(T)[None, :] < n_steps[:, None])[:, :, None], x, 0.0)    # the padding is never read
    h = np.zeros((B, H), f) if h0 is None else np.asarray(h0, f).copy()
    hs, keep = np.zeros((B, T, H), f), []
    for t in range(T):
        gi, gh = x[:, t] @ wih.T + bih, h @ whh.T + bhh
        if wrong == "bhn_outside":
            gi[:, 2 * H:] += bhh[2 * H:]
            gh[:, 2 * H:] -= bhh[2 * H:]
        r, z = _sig(gi[:, :H] + gh[:, :H]), _sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        hn = z * n + (1 - z) * h if wrong == "swap_z" else (1 - z) * n + z * h
        keep.append((r, z, n, gh[:, 2 * H:], h))
        h = np.where(live[:, t, None], hn, h)
        hs[:, t] = h
    out = {"h": h, "hs": hs}
    if glast is None:
        return out
    dh = np.asarray(glast, f).copy()
    gx = np.zeros((B, T, E), f)
    gwih, gwhh, gbih, gbhh = np.zeros_like(wih), np.zeros_like(whh), np.zeros(3 * H, f), np.zeros(3 * H, f)
    for t in range(T - 1, -1, -1):
        r, z, n, ghn, hp = keep[t]
        m = live[:, t, None]
        if wrong == "swap_z":
            d_n, d_z = dh * z, dh * (n - hp)
        else:
            d_n, d_z = dh * (1 - z), dh * (hp - n)
        d_ain = d_n * (1 - n * n) * m
        d_ahn = d_ain * r
        d_ar = d_ain * ghn * r * (1 - r)
        d_az = d_z * z * (1 - z) * m
        dgi, dgh = np.concatenate([d_ar, d_az, d_ain], 1), np.concatenate([d_ar, d_az, d_ahn], 1)
        gx[:, t] = dgi @ wih
        gwih += dgi.T @ x[:, t]
        dgh_w = dgh.copy()
        if wrong == "gwhh_tile_row":
            dgh_w[15::16] = 0.0                                  # the last row of every 16-row tile
        gwhh += dgh_w.T @ hp
        gbih += dgi.sum(0)
        gbhh += dgh.sum(0)
        direct = dh * ((1 - z) if wrong == "swap_z" else z)
        dh = np.where(m, direct + dgh @ whh, dh)
    if wrong == "gbhh_no_n":
        gbhh[2 * H:] = 0.0
    if wrong == "gx_last_missing":
        rows = np.nonzero(n_steps > 0)[0]
        gx[rows, n_steps[rows] - 1] = 0.0
    out.update(gx=gx, gwih=gwih, gwhh=gwhh, gbih=gbih, gbhh=gbhh)
    return out


def case_f64(c, wrong=None):
    return gru_f64(c["x"], c["lengths"], c["wih"], c["whh"], c["bih"], c["bhh"], c["glast"], wrong=wrong)


# ------------------------------------------------------------------------------------------------ figures
def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    diff, den = float(np.max(np.abs(a - b))), float(np.max(np.abs(b)))
    return diff / den if den > 0 else (0.0 if diff == 0 else float("inf"))


def figures(got, ref):
    """got: dict(h, gx, gwih, gwhh, gbih, gbhh) -> relative error of each against gru_f64's result"""
    return {n: rel_err(got[n], ref[n]) for n in GROUP_OF}


def worst(fig):
    w = {g: 0.0 for g in GROUPS}
    for n, v in fig.items():
        w[GROUP_OF[n]] = max(w[GROUP_OF[n]], v)
    return w


def fmt(tag, fig, tol=None):
    w, tol = worst(fig), TOL if tol is None else tol
    return "parity gru %s: " % tag + " ".join("%s %.2e (tol %.0e)" % (g, w[g], tol[g]) for g in GROUPS)


# ------------------------------------------------------------------------------------------------ several tiles per workgroup
PER_ROW = ("h", "gx")
WALK_WRONGS = ("later_visits_dropped", "later_visits_stale", "length_of_first_visit", "h_carry")


def first_visit_of(B, cap):
    """int64 [B]: b for b < cap, b - cap after it — the row a workgroup held in the same place one visit earlier"""
    src = np.arange(B)
    src[cap:] -= cap
    return src


def visit_figures(got, ref, cap):
    """{name: (first, later)}: the figure of h and gx apart for the rows of a workgroup's first tile (b < cap) and of its later
    ones, both against the whole array's max |ref|"""
    fig = {}
    for n in PER_ROW:
        a, b = np.asarray(got[n], np.float64), np.asarray(ref[n], np.float64)
        den = max(float(np.max(np.abs(b))), 1e-300)
        fig[n] = (float(np.max(np.abs(a[:cap] - b[:cap]))) / den, float(np.max(np.abs(a[cap:] - b[cap:]))) / den if len(b) > cap else 0.0)
    return fig


def visit_fmt(fig):
    return " ".join("%s first %.2e later %.2e" % (n, *v) for n, v in fig.items())


def walk_wrong(c, ref, wrong, cap):
    """deliberately WRONG results of a walk over `cap` rows per visit: 'later_visits_dropped' (the four parameter gradients summed
    over the rows b < cap only), 'later_visits_stale' (h and gx of row b >= cap those of row b - cap), 'length_of_first_visit'
    (row b >= cap takes the steps of row b - cap), 'h_carry' (row b >= cap starts from the final state of row b - cap, not zero)"""
    B = len(c["lengths"])
    src = first_visit_of(B, cap)
    if wrong == "later_visits_dropped":
        part = gru_f64(c["x"][:cap], c["lengths"][:cap], c["wih"], c["whh"], c["bih"], c["bhh"], c["glast"][:cap])
        return dict(ref, **{n: part[n] for n in ("gwih", "gwhh", "gbih", "gbhh")})
    if wrong == "later_visits_stale":
        return dict(ref, **{n: ref[n][src] for n in PER_ROW})
    if wrong == "length_of_first_visit":
        return case_f64(dict(c, lengths=c["lengths"][src]))
    if wrong == "h_carry":
        h0 = np.where((np.arange(B) >= cap)[:, None], ref["h"][src], 0.0)
        return gru_f64(c["x"], c["lengths"], c["wih"], c["whh"], c["bih"], c["bhh"], c["glast"], h0=h0)
    raise ValueError(wrong)


# ------------------------------------------------------------------------------------------------ the stock path
def torch_gru(c, dtype, device="cpu"):
    """nn.GRU(E, H, batch_first=True) holding the case's parameters"""
    import torch
    E, H = c["wih"].shape[1], c["whh"].shape[1]
    rnn = torch.nn.GRU(E, H, batch_first=True).to(device=device, dtype=dtype)
    with torch.no_grad():
        for name, key in (("weight_ih_l0", "wih"), ("weight_hh_l0", "whh"), ("bias_ih_l0", "bih"), ("bias_hh_l0", "bhh")):
            getattr(rnn, name).copy_(torch.as_tensor(c[key], dtype=dtype, device=device))
    return rnn


def stock(c, dtype=None, device="cpu", packed=False):
    """the stock path under torch.autograd -> dict(h, gx, gwih, gwhh, gbih, gbhh).  packed=False: nn.GRU over the padded batch and
    the row at lengths - 1 (what --gru_native 0 runs); packed=True: ReChorus's sort / pack_padded_sequence / unsort form."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    rnn = torch_gru(c, dtype, device)
    x = torch.as_tensor(c["x"], dtype=dtype, device=device).clone().requires_grad_(True)
    lengths = torch.as_tensor(c["lengths"], device=device)
    if packed:
        sort_len, sort_idx = torch.topk(lengths, k=len(lengths))
        packed_x = torch.nn.utils.rnn.pack_padded_sequence(x.index_select(0, sort_idx), sort_len.cpu(), batch_first=True)
        _, hidden = rnn(packed_x, None)
        unsort_idx = torch.topk(sort_idx, k=len(lengths), largest=False)[1]
        h = hidden[-1].index_select(0, unsort_idx)
    else:
        output, _ = rnn(x)
        h = output[torch.arange(x.shape[0], device=device), lengths - 1, :]
    h.backward(torch.as_tensor(c["glast"], dtype=dtype, device=device))
    return {"h": h.detach().cpu().numpy(), "gx": x.grad.cpu().numpy(), "gwih": rnn.weight_ih_l0.grad.cpu().numpy(),
            "gwhh": rnn.weight_hh_l0.grad.cpu().numpy(), "gbih": rnn.bias_ih_l0.grad.cpu().numpy(),
            "gbhh": rnn.bias_hh_l0.grad.cpu().numpy()}


def measure_floors(shapes=None, patterns=PATTERNS, walk=False):
    """-> {group: largest figure of the stock fp32 path against float64 on a CPU}, and the per-case figures; `shapes`: indices
    into SHAPES, or into WALK_SHAPES with walk=True (patterns: those of walk_patterns, unless given)"""
    floors, cases = {g: 0.0 for g in GROUPS}, {}
    lst = (WALK_SHAPES, WALK_SEED) if walk else (None, 9100)
    for i in (range(len(WALK_SHAPES if walk else SHAPES)) if shapes is None else shapes):
        for pat in (walk_patterns(i) if walk and patterns is PATTERNS else patterns):
            c = make_case(i, pat, *lst)
            w = worst(figures(stock(c), case_f64(c)))
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
