"""NumPy restatement of wr_seq_augment (whisprrec_amd/csrc/wr_seqaug.hip, K21), bit for bit: the same keys, counters, double
arithmetic and ranks, vectorised over rows.  `wrong=` switches in one deliberately wrong rule for the power tests."""
import numpy as np

GOLD = np.uint64(0x9E3779B97F4A7C15)
ROW_MUL = np.uint64(0xD1B54A32D192ED03)
DOMAIN = np.uint64(0x5345514155473231)
KEY_COUNTER, START_COUNTER, MAX_T, MAX_UNIFORMS = 16, 80, 64, 15
WRONG = ("uniform_ratio", "next_order_statistic", "rounded_sel", "short_start", "prefix_mask")
M64 = (1 << 64) - 1


def mix64(x):
    """splitmix64 finaliser (wr_common.h)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def supported(T, a, b):
    return 1 <= T <= MAX_T and a >= 1 and b >= 1 and a + b - 1 <= MAX_UNIFORMS


def view_keys(seed, epoch, rows, view):
    """the key of (seed, epoch, dataset row, view), uint64 [n]"""
    with np.errstate(over="ignore"):
        key_epoch = mix64(mix64(np.uint64(seed & M64) ^ (np.uint64(epoch & M64) * GOLD)) ^ DOMAIN)
        return mix64(key_epoch ^ ((np.asarray(rows).astype(np.uint64) * np.uint64(2) + np.uint64(view)) * ROW_MUL + np.uint64(1)))


def draw(key, counter):
    with np.errstate(over="ignore"):
        return mix64(key + (np.asarray(counter, dtype=np.uint64) + np.uint64(1)) * GOLD)


def unit(d):
    return (d >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def mulhi(d, n):
    """high 64 bits of d * n for n < 2^32"""
    n = np.asarray(n).astype(np.uint64)
    lo32 = np.uint64(0xFFFFFFFF)
    return ((d >> np.uint64(32)) * n + (((d & lo32) * n) >> np.uint64(32))) >> np.uint64(32)


def decisions(rows, L, a, b, seed, epoch, view, wrong=None):
    """per row: its key, the op (mask or reorder), ratio, sel and start"""
    key = view_keys(seed, epoch, rows, view)
    L = np.asarray(L, dtype=np.int64)
    do_mask = unit(draw(key, 0)) > 0.5
    n_unif = a + b - 1
    U = unit(draw(key[:, None], 1 + np.arange(n_unif)[None, :]))
    # the value of rank a - 1 by (value, index): ties share the value, so the sorted column is that value
    ratio = np.sort(U, axis=1)[:, a - 1]
    if wrong == "uniform_ratio":
        ratio = U[:, 0]
    elif wrong == "next_order_statistic":
        ratio = np.sort(U, axis=1)[:, a]
    sel = (L.astype(np.float64) * ratio).astype(np.int64)            # truncation
    if wrong == "rounded_sel":
        sel = np.minimum(np.floor(L.astype(np.float64) * ratio + 0.5).astype(np.int64), L)
    span = L - sel if wrong == "short_start" else L - sel + 1
    start = mulhi(draw(key, START_COUNTER), np.maximum(span, 0)).astype(np.int64)
    return {"key": key, "mask": do_mask, "ratio": ratio, "sel": sel, "start": start}


def ranks(keys, lo, hi):
    """the kernel's loop: rank[r, t] = #{ j in [lo_r, hi_r) : (key_j, j) < (key_t, t) }"""
    n, T = keys.shape
    t = np.arange(T)
    out = np.zeros((n, T), np.int16)
    for j in range(T):
        kj = keys[:, j:j + 1]
        live = ((j >= lo) & (j < hi))[:, None]
        out += live & ((kj < keys) | ((kj == keys) & (j < t)[None, :]))
    return out.astype(np.int64)


def one_view(src, L, rows, mask_token, a, b, seed, epoch, view, wrong=None):
    """src [n, T] (zero past L), L [n] in [1, T], rows [n] -> (view [n, T], decisions)"""
    src = np.asarray(src, dtype=np.int64)
    n, T = src.shape
    L = np.asarray(L, dtype=np.int64)
    d = decisions(rows, L, a, b, seed, epoch, view, wrong)
    t = np.arange(T)[None, :]
    lo = np.where(d["mask"], 0, d["start"])
    hi = np.where(d["mask"], L, d["start"] + d["sel"])
    keys = draw(d["key"][:, None], KEY_COUNTER + np.arange(T)[None, :])
    rank = ranks(keys, lo, hi)
    if wrong == "prefix_mask":
        rank = np.broadcast_to(t, (n, T))
    masked = np.where((t < L[:, None]) & (rank < d["sel"][:, None]), np.int64(mask_token), src)
    inwin = (t >= lo[:, None]) & (t < hi[:, None])
    frm = np.where(inwin, d["start"][:, None] + rank, t)
    moved = np.take_along_axis(src, np.clip(frm, 0, T - 1), axis=1)
    d["rank"] = rank
    return np.where(d["mask"][:, None], masked, moved), d


def seq_augment(hist, lengths, rows, mask_token, a, b, seed, epoch, wrong=None):
    """-> (out_a, out_b, err_word) as wr_seq_augment writes them"""
    hist, lengths, rows = (np.asarray(x, dtype=np.int64) for x in (hist, lengths, rows))
    n_rows, T = hist.shape
    assert supported(T, a, b)
    bad_row = (rows < 0) | (rows >= n_rows)
    safe = np.where(bad_row, 0, rows)
    raw = lengths[safe]
    bad_len = ((raw < 1) | (raw > T)) & ~bad_row
    L = np.clip(raw, 1, T)
    src = np.where(np.arange(T)[None, :] < L[:, None], hist[safe], 0)
    outs = []
    for view in (0, 1):
        out, _ = one_view(src, L, rows, mask_token, a, b, seed, epoch, view, wrong)
        out[bad_row] = 0
        outs.append(out)
    return outs[0], outs[1], (1 if bad_len.any() else 0) | (2 if bad_row.any() else 0)
