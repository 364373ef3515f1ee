"""CPU checks of ContraRec's device view builder (--aug_native, wr_seq_augment, K21) through its NumPy restatement
(contrarec_aug_ref): the structure of the views, exactly, for every length; the distribution against the reference's rule (exact
Beta cell probabilities, uniform start / subset / permutation) with the project's own NumPy augmentations as the control arm under
the same thresholds; wrong variants land above those thresholds; the flag, the model's switch and the entry point's argument
errors.

Every chi-square statistic is held against the upper critical value at 1e-6 for its degrees of freedom, by Wilson-Hilferty:
df (1 - 2/(9 df) + 4.753 sqrt(2/(9 df)))^3 (4.753 is the normal quantile of 1 - 1e-6); the mask share against 4.9 sigma
(two-sided 1e-6).  Seeds are fixed: the tests are deterministic.  Cells whose expected count is below 5 are pooled with their
neighbours (Pearson's rule of thumb; df is that of the pooled table) — at N = 200,000 this touches the tail of Beta(1, 5) only.
The control arm of the two extra Beta pairs draws N / 4 rows (it is a Python loop over rows): same statistic, same threshold rule."""
import argparse
import ctypes
import logging
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrarec_aug_ref as A  # noqa: E402
from whisprrec_amd import host  # noqa: E402

TOKEN = 1000
N, L, SEED, EPOCH = 200_000, 20, 3407, 1
PERMS3 = {p: i for i, p in enumerate([(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)])}


def crit(df):
    """chi-square upper critical value at 1e-6 (Wilson-Hilferty)"""
    c = 2.0 / (9.0 * df)
    return df * (1.0 - c + 4.753 * math.sqrt(c)) ** 3


def chi2(observed, expected):
    """Pearson's statistic and its degrees of freedom; neighbouring cells are pooled until each expects at least 5"""
    observed, expected = np.asarray(observed, np.float64), np.asarray(expected, np.float64)
    assert abs(observed.sum() - expected.sum()) <= 1e-6 * expected.sum()
    obs, exp = [], []
    o = e = 0.0
    for oi, ei in zip(observed, expected):
        o, e = o + oi, e + ei
        if e >= 5.0:
            obs.append(o)
            exp.append(e)
            o = e = 0.0
    if e > 0.0 or o > 0.0:
        obs[-1] += o
        exp[-1] += e
    obs, exp = np.asarray(obs), np.asarray(exp)
    return float(((obs - exp) ** 2 / exp).sum()), len(obs) - 1


def sel_pmf(length, a, b):
    """P(int(L * ratio) = k), ratio ~ Beta(a, b) with integer a, b: F((k + 1) / L) - F(k / L)"""
    n = a + b - 1
    x = np.arange(length + 1, dtype=np.float64) / length
    F = sum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a, n + 1))
    return np.diff(F)


# ------------------------------------------------------------------------------------------------ the two arms
def _source(n, length):
    return np.tile(np.arange(1, length + 1, dtype=np.int64), (n, 1))


def restated(a, b, wrong=None, full=True, n=N):
    """view 0 of n rows of length L from the restatement -> {mask, sel, start, out}; full=False: the decisions alone"""
    rows = np.arange(n)
    lens = np.full(n, L)
    if not full:
        return A.decisions(rows, lens, a, b, SEED, EPOCH, 0, wrong)
    out, d = A.one_view(_source(n, L), lens, rows, TOKEN, a, b, SEED, EPOCH, 0, wrong)
    d["out"] = out
    d["sel"] = np.where(d["mask"], (out == TOKEN).sum(axis=1), d["sel"])          # a masked view shows its own sel
    return d


def control(a, b, monkeypatch, n=N):
    """the same from the project's Dataset.augment / mask_op / reorder_op (NumPy's global stream), on a stub model: the op and the
    draws are recorded on their way through"""
    from whisprrec_amd.contrarec import ContraRec
    log = {"op": [], "ratio": [], "start": []}
    beta, randint = np.random.beta, np.random.randint

    def rec_beta(*args, **kw):
        r = beta(*args, **kw)
        log["ratio"].append(r)
        return r

    def rec_randint(*args, **kw):
        r = randint(*args, **kw)
        log["start"].append(r)
        return r

    class Recording(ContraRec.Dataset):
        def mask_op(self, seq):
            log["op"].append(True)
            log["start"].append(0)
            return super().mask_op(seq)

        def reorder_op(self, seq):
            log["op"].append(False)
            return super().reorder_op(seq)

    ds = Recording.__new__(Recording)
    ds.model = types.SimpleNamespace(beta_a=a, beta_b=b, mask_token=TOKEN)
    monkeypatch.setattr(np.random, "beta", rec_beta)
    monkeypatch.setattr(np.random, "randint", rec_randint)
    np.random.seed(SEED)
    src = np.arange(1, L + 1, dtype=np.int64)
    out = np.stack([ds.augment(src) for _ in range(n)])
    monkeypatch.undo()
    mask = np.asarray(log["op"])
    sel = np.where(mask, (out == TOKEN).sum(axis=1), (L * np.asarray(log["ratio"])).astype(np.int64))
    return {"mask": mask, "sel": sel, "start": np.asarray(log["start"], dtype=np.int64), "out": out}


def fig_share(d):
    n = len(d["mask"])
    return abs(float(d["mask"].mean()) - 0.5) / (0.5 / math.sqrt(n))


def fig_sel(d, a, b, op):
    pick = d["mask"] == op
    return chi2(np.bincount(d["sel"][pick], minlength=L)[:L], sel_pmf(L, a, b) * pick.sum()) if (d["sel"][pick] < L).all() \
        else (float("inf"), L - 1)


def fig_start(d, sel=10):
    pick = ~d["mask"] & (d["sel"] == sel)
    cells = L - sel + 1
    return chi2(np.bincount(d["start"][pick], minlength=cells), np.full(cells, pick.sum() / cells))


def fig_positions(d):
    hits = (d["out"][d["mask"]] == TOKEN).sum(axis=0)
    return chi2(hits, np.full(L, hits.sum() / L))


def fig_perms(d, sel=3):
    pick = ~d["mask"] & (d["sel"] == sel)
    start, out = d["start"][pick], d["out"][pick]
    window = np.take_along_axis(out, start[:, None] + np.arange(sel)[None, :], axis=1) - 1 - start[:, None]
    idx = [PERMS3[tuple(w)] for w in window.tolist()]
    return chi2(np.bincount(idx, minlength=6), np.full(6, len(idx) / 6))


@pytest.fixture(scope="module")
def base():
    return restated(3, 3)


# ------------------------------------------------------------------------------------------------ structure, exact
@pytest.mark.parametrize("T", [1, 2, 20, 64])
def test_structure_of_the_views_for_every_length(T):
    reps = 40 if T <= 20 else 12
    lens = np.repeat(np.arange(1, T + 1), reps)
    n = lens.size
    rng = np.random.RandomState(T)
    hist = np.zeros((n, T), np.int64)
    for r, ln in enumerate(lens):
        hist[r, :ln] = rng.permutation(900)[:ln] + 1                          # distinct items: a permutation is visible
    seen = {"mask": 0, "reorder": 0, "moved": 0}
    for a, b in ((3, 3), (1, 1), (1, 5), (8, 8)):
        for view in (0, 1):
            out, d = A.one_view(hist, lens, np.arange(n), TOKEN, a, b, SEED, EPOCH, view)
            t = np.arange(T)[None, :]
            assert (out[t >= lens[:, None]] == 0).all()                                       # padding stays 0
            assert (d["sel"] <= lens - 1).all() and (d["sel"] >= 0).all()
            assert (d["sel"] == (lens * d["ratio"]).astype(np.int64)).all()
            assert np.array_equal(out[lens == 1], hist[lens == 1])                            # L = 1 returns the source
            m = d["mask"]
            changed = out != hist
            assert ((out == TOKEN) == changed)[m].all() and (changed[m].sum(axis=1) == d["sel"][m]).all()
            ro, rh = out[~m], hist[~m]
            assert np.array_equal(np.sort(ro, axis=1), np.sort(rh, axis=1))                    # a permutation of the source ...
            start, sel = d["start"][~m], d["sel"][~m]
            assert (start >= 0).all() and (start + sel <= lens[~m]).all()
            outside = (t < start[:, None]) | (t >= (start + sel)[:, None])
            assert (ro == rh)[outside].all()                                                   # ... identical outside the window
            assert not changed[~m][sel <= 1].any()
            seen["mask"] += int(m.sum())
            seen["reorder"] += int((~m).sum())
            seen["moved"] += int(changed[~m].any(axis=1).sum())
    assert seen["mask"] > 0 and seen["reorder"] > 0 and (T <= 2 or seen["moved"] > 0)      # sel <= L - 1 <= 1 moves nothing


def test_views_do_not_depend_on_the_batch_and_differ_between_epochs_seeds_and_views():
    rng = np.random.RandomState(7)
    n_rows, T = 300, 20
    lens = rng.randint(1, T + 1, size=n_rows)
    hist = np.where(np.arange(T)[None, :] < lens[:, None], rng.randint(1, 900, size=(n_rows, T)), 0)
    every = np.arange(n_rows)
    fa, fb, err = A.seq_augment(hist, lens, every, TOKEN, 3, 3, SEED, EPOCH)
    assert err == 0
    for rows in (np.array([5]), np.array([7, 5, 299, 5, 0]), rng.randint(0, n_rows, size=257), every[::-1].copy()):
        a, b, _ = A.seq_augment(hist, lens, rows, TOKEN, 3, 3, SEED, EPOCH)
        assert np.array_equal(a, fa[rows]) and np.array_equal(b, fb[rows])
    long = lens >= 8
    other_epoch = A.seq_augment(hist, lens, every, TOKEN, 3, 3, SEED, EPOCH + 1)
    other_seed = A.seq_augment(hist, lens, every, TOKEN, 3, 3, SEED + 1, EPOCH)
    for x, y in ((fa, other_epoch[0]), (fb, other_epoch[1]), (fa, other_seed[0]), (fb, other_seed[1]), (fa, fb)):
        assert (x[long] != y[long]).any(axis=1).mean() > 0.8


def test_lengths_and_row_ids_out_of_range_are_clamped_or_zeroed():
    hist = np.array([[4, 5, 6], [7, 8, 0], [9, 0, 0]], np.int64)
    good = A.seq_augment(hist, [3, 2, 1], [0, 1, 2], TOKEN, 3, 3, SEED, EPOCH)
    a, b, err = A.seq_augment(hist, [4, 2, 0], [0, 1, 2, 3, -1], TOKEN, 3, 3, SEED, EPOCH)
    assert err == 3 and not a[3:].any() and not b[3:].any()
    assert np.array_equal(a[:3], good[0]) and np.array_equal(b[:3], good[1])           # clamped to 3 and to 1
    assert A.seq_augment(hist, [3, 2, 1], [3], TOKEN, 3, 3, SEED, EPOCH)[2] == 2
    assert A.seq_augment(hist, [3, 2, 0], [2], TOKEN, 3, 3, SEED, EPOCH)[2] == 1


# ------------------------------------------------------------------------------------------------ distribution
def test_distribution_follows_the_reference_rule_and_so_does_the_control_arm(base, monkeypatch):
    arms = {"restatement": base, "numpy control": control(3, 3, monkeypatch)}
    for name, d in arms.items():
        share = fig_share(d)
        print("aug %s: mask share %.5f, %.2f sigma (bound 4.9)" % (name, d["mask"].mean(), share))
        assert share <= 4.9, name
        figs = {"sel | mask": fig_sel(d, 3, 3, True), "sel | reorder": fig_sel(d, 3, 3, False), "start | sel = 10": fig_start(d),
                "mask position": fig_positions(d), "window permutation | sel = 3": fig_perms(d)}
        for what, (stat, df) in figs.items():
            print("aug %s: chi2 %s = %.1f (df %d, threshold %.1f)" % (name, what, stat, df, crit(df)))
        assert [figs[k][1] for k in figs] == [19, 19, 10, 19, 5]
        for what, (stat, df) in figs.items():
            assert stat <= crit(df), (name, what, stat)


@pytest.mark.parametrize("beta", [(1, 1), (1, 5)])
def test_sel_follows_other_beta_parameters(beta, monkeypatch):
    arms = {"restatement": restated(*beta, full=False), "numpy control": control(*beta, monkeypatch, n=N // 4)}
    for name, d in arms.items():
        for op in (True, False):
            stat, df = fig_sel(d, beta[0], beta[1], op)
            print("aug %s beta=%s: chi2 sel | %s = %.1f (df %d, threshold %.1f)" % (name, beta, "mask" if op else "reorder", stat, df,
                                                                                  crit(df)))
            assert stat <= crit(df), (name, beta, op, stat)


def test_thresholds_are_the_derived_ones():
    assert [round(crit(df), 1) for df in (19, 10, 5)] == [64.4, 48.0, 37.5]


@pytest.mark.parametrize("wrong", A.WRONG)
def test_wrong_variants_land_above_the_threshold(wrong):
    if wrong == "prefix_mask":
        stat, df = fig_positions(restated(3, 3, wrong))
    elif wrong == "short_start":
        stat, df = fig_start(restated(3, 3, wrong, full=False))
    else:
        d = restated(3, 3, wrong, full=False)
        stat, df = max(fig_sel(d, 3, 3, True), fig_sel(d, 3, 3, False))
    print("aug wrong %s: chi2 %.1f (df %d, threshold %.1f)" % (wrong, stat, df, crit(df)))
    assert stat > crit(df)


# ------------------------------------------------------------------------------------------------ plumbing
def _args(**kw):
    base_args = dict(device="cpu", model_path="/tmp/wr_contrarec_aug.pt", buffer=1, num_neg=1, test_all=1, history_max=20, emb_size=64,
                     gamma=0.5, beta_a=3, beta_b=3, ccc_temp=0.2)
    base_args.update(kw)
    return argparse.Namespace(**base_args)


def test_launcher_knows_the_flag():
    from whisprrec_amd import main as launcher
    from whisprrec_amd.contrarec import ContraRec
    assert launcher.build_args(["--model_name", "ContraRec", "--aug_native", "1"])[0].aug_native == 1
    assert launcher.build_args(["--model_name", "ContraRec"])[0].aug_native == 0
    text = " ".join(ContraRec.parse_model_args(argparse.ArgumentParser()).format_help().split())
    assert "--aug_native" in text and "reference's distribution" in text and "--random_seed" in text and "not NumPy's stream" in text


def test_the_flag_clears_per_sample_feed_for_supported_shapes_only(caplog):
    from whisprrec_amd.contrarec import ContraRec
    corpus = host.Corpus(40, 300, {})
    assert ContraRec.per_sample_feed is True
    assert ContraRec(_args(), corpus).per_sample_feed is True
    assert ContraRec(_args(aug_native=0), corpus).per_sample_feed is True
    on = ContraRec(_args(aug_native=1, random_seed=11), corpus)
    assert on.per_sample_feed is False and on.aug_seed == 11 and ContraRec.per_sample_feed is True
    assert ContraRec(_args(aug_native=1, history_max=64, beta_a=8, beta_b=8), corpus).per_sample_feed is False
    for kw in (dict(history_max=65), dict(history_max=0), dict(beta_a=8, beta_b=9)):
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            m = ContraRec(_args(aug_native=1, **kw), corpus)
        assert m.per_sample_feed is True, kw
        assert sum("keeping the host path" in r.getMessage() for r in caplog.records) == 1, kw


def test_supported_set():
    from whisprrec_amd import abi, hip_ops
    S = abi.lib().wr_seq_augment_supported
    assert [S(T, 3, 3) for T in (0, 1, 20, 64, 65)] == [0, 1, 1, 1, 0]
    assert [S(20, a, b) for a, b in ((1, 1), (1, 15), (8, 8), (8, 9), (16, 1), (0, 3), (3, 0), (-1, 17))] == [1, 1, 1, 0, 0, 0, 0, 0]
    assert hip_ops.seq_augment_supports(20, 3, 3) and not hip_ops.seq_augment_supports(20, 2.5, 3)
    assert all(A.supported(T, a, b) == bool(S(T, a, b)) for T in (0, 1, 64, 65) for a in (0, 1, 8, 15, 16) for b in (0, 1, 8, 15))


def test_argument_errors_are_reported_before_any_launch():
    """no GPU here: every one of these returns before a launch"""
    from whisprrec_amd import abi
    lib = abi.lib()
    buf = (ctypes.c_int64 * 256)()
    p = ctypes.addressof(buf)

    def call(hist=p, lengths=p, n_rows=4, T=20, rows=p, B=4, a=3, b=3, out_a=p, out_b=p):
        return lib.wr_seq_augment(hist, lengths, n_rows, T, rows, B, 300, a, b, 1, 1, out_a, out_b, None, None)

    for name in ("hist", "lengths", "rows", "out_a", "out_b"):
        assert call(**{name: None}) == -1 and "NULL" in abi.last_error(), name
    assert call(T=65) == -5 and "T=65" in abi.last_error()
    assert call(T=0) == -5 and call(a=8, b=9) == -5 and call(a=0) == -5 and call(b=0) == -5
    assert call(B=-1) == -2 and "B=-1" in abi.last_error()
    assert call(n_rows=0) == -2
    assert call(B=0) == 0                                                                  # an empty batch launches nothing


def test_wrapper_refuses_cpu_tensors():
    from whisprrec_amd import abi, hip_ops
    hist = torch.zeros((4, 20), dtype=torch.int64)
    lens = torch.ones(4, dtype=torch.int64)
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.seq_augment(hist, lens, torch.arange(4), 300, 3, 3, 1, 1)
