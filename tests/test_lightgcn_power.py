"""What the checks of LightGCN's EmbLoss term can and cannot see (CPU only; oracle/lightgcn_parity.py).

Floor: an fp32 restatement against the float64 reference — never the code under test — on the exact inputs of the GPU cases
(tests/test_hip_embloss.py, the whole-step cases of tests/test_lightgcn.py, g4's inputs at g11's reg_weight).  The whole step
is restated by the C oracle; the isolated term in NumPy fp32: sums of squares in fp32, rob / sqrt, count * coef * row, one
multiply-add into the gradient buffer.  Every TOL_* of lightgcn_parity is 8 x its largest floor rounded up to one significant
digit, and every floor leaves a factor 4.

Power: seven wrong versions of the term, restated on the float64 values, exceed the new tolerances at least five times at the
new tests' reg_weight — and pass conftest.rel_err < 1e-5 on the gradient at reg_weight 1e-5 on g4's inputs, which is all the
suite asked before (the recorded reason for the new tests).  The loss without its term is 1.5e-5 off on g4 and 7.7e-7 on the
ml-1m-shaped batch of test_hip_config_shapes.py (C3): accepted there."""
import functools
import math

import numpy as np
import pytest

import oracle
from conftest import rel_err
from oracle import lightgcn_parity as lp
from oracle import parity

F32 = np.float32
TOL = 1e-5                                  # the bound of test_lightgcn.py / test_oracle_golden.py, unchanged
ALL_EMBLOSS = tuple((D, B, "plain") for D, B in lp.EMBLOSS_CASES) + tuple((D, B, k) for k, D, B in lp.EMBLOSS_SPECIAL)


@pytest.fixture(scope="module")
def g11():
    return oracle.load_golden("g11_lightgcn_reg")


# ------------------------------------------------------------------------------------------------ fp32 restatements
def _sumsq_f32(c):
    return np.array([np.sum(t[i] * t[i], dtype=F32) for t, i in ((c["U0"], c["ub"]), (c["I0"], c["pb"]), (c["I0"], c["nb"]))],
                    dtype=F32)


def _embloss_grad_f32(c, sq, G0u=None, G0i=None):
    """count * (rob / sqrt(sq)) per row in fp32, then ONE multiply-add per element into the buffer"""
    nU, nI = c["U0"].shape[0], c["I0"].shape[0]
    rob = F32(c["reg_weight"]) / F32(c["B"])
    nrm = np.sqrt(sq)
    cnt = [np.bincount(c[k], minlength=r).astype(F32) for k, r in (("ub", nU), ("pb", nI), ("nb", nI))]
    per = [cnt[k] * (rob / nrm[k]) if nrm[k] > 0 else np.zeros_like(cnt[k]) for k in range(3)]
    coef_u, coef_i = per[0], (per[1] + per[2]).astype(F32)

    def fma(G0, coef, tab):
        base = 0.0 if G0 is None else G0.astype(np.float64)
        return (base + coef[:, None].astype(np.float64) * tab.astype(np.float64)).astype(F32)

    return fma(G0u, coef_u, c["U0"]), fma(G0i, coef_i, c["I0"])


def _loss_f32(c, sq, reg_weight):
    """the loss tail in fp32: dots carried in double and rounded once (as wr_oracle.c), fp32 sigmoid / log, fp32 fold"""
    ue, pe, ne = c["Ua"][c["ub"]], c["Ia"][c["pb"]], c["Ia"][c["nb"]]
    x = (ue * pe).sum(axis=1, dtype=np.float64).astype(F32) - (ue * ne).sum(axis=1, dtype=np.float64).astype(F32)
    with np.errstate(over="ignore"):
        s = F32(1) / (F32(1) + np.exp(-x))
    term = -np.log(F32(1e-10) + s)
    B = F32(c["B"])
    mean = F32(term.sum(dtype=np.float64)) / B
    reg = (np.sqrt(sq[0]) + np.sqrt(sq[1]) + np.sqrt(sq[2])) / B
    return F32(mean + F32(reg_weight) * reg)


@functools.lru_cache(maxsize=None)
def _embloss_floor(D, B, kind):
    c = lp.embloss_case(D, B, kind)
    sq = _sumsq_f32(c)
    live = c["sq3"] > 0
    f = {"sq": float(np.max(np.abs(sq.astype(np.float64)[live] - c["sq3"][live]) / c["sq3"][live]))}
    assert np.all(sq[~live] == 0)
    term = float(F32(c["reg_weight"])) * c["reg_loss"]
    l0, l1 = float(_loss_f32(c, sq, 0.0)), float(_loss_f32(c, sq, c["reg_weight"]))
    f["loss0"] = abs(l0 - c["bpr_loss"]) / c["bpr_loss"]
    f["reg_loss"] = abs((l1 - l0) - term) / term
    f["reg_share_of_loss"] = term / (c["bpr_loss"] + term)
    gU, gI = _embloss_grad_f32(c, sq)
    f["row_u"], f["row_i"] = lp.row_err(gU, c["gU"]), lp.row_err(gI, c["gI"])
    hU, hI = _embloss_grad_f32(c, sq, c["G0u"], c["G0i"])
    f["row_u_G0"] = lp.row_err(hU, c["G0u"].astype(np.float64) + c["gU"], scale=c["gU"])
    f["row_i_G0"] = lp.row_err(hI, c["G0i"].astype(np.float64) + c["gI"], scale=c["gI"])
    print("floor embloss D %d B %d %s: rw %.3g sq %.2e loss0 %.2e reg_loss %.2e row u %.2e i %.2e, into G0 u %.2e i %.2e" % (
        D, B, kind, c["reg_weight"], f["sq"], f["loss0"], f["reg_loss"], f["row_u"], f["row_i"], f["row_u_G0"], f["row_i_G0"]))
    return f


def _whole_floor(tag, nU, nI, rp, col, val, E0, L, rw, u, p, n, ref):
    bpr, reg, g_bpr, g_reg = ref
    loss, g = oracle.lightgcn_loss_grads(nU, nI, rp, col, val, E0, L, rw, u, p, n)
    want, g64 = bpr + float(F32(rw)) * reg, g_bpr + g_reg
    f = {"loss": abs(loss - want) / want, "rel": max(rel_err(g[:nU], g64[:nU]), rel_err(g[nU:], g64[nU:])),
         "row": max(lp.row_err(g[:nU], g64[:nU]), lp.row_err(g[nU:], g64[nU:])), "share": lp.reg_share(g_bpr, g_reg)}
    print("floor step %s: rw %.3g share %.3f loss %.2e rel_err %.2e row_err %.2e" % (tag, rw, f["share"], f["loss"], f["rel"], f["row"]))
    return f


@functools.lru_cache(maxsize=None)
def _step_floor(case):
    c = lp.step_case(*case)
    return _whole_floor(str(case), c["n_users"], c["n_items"], c["row_ptr"], c["col"], c["val"], c["E0"], c["L"], c["reg_weight"],
                        c["u"], c["p"], c["n"], (c["bpr_loss"], c["reg_loss"], c["g_bpr"], c["g_reg"]))


def _g4_at(g4, rw):
    nU, nI = g4["U0"].shape[0], g4["I0"].shape[0]
    rp, col, val = lp.g4_csr(g4)
    return nU, nI, rp, col, val, np.concatenate([g4["U0"], g4["I0"]]), int(g4["hp"][0]), rw, g4["u"], g4["p"], g4["n"]


def _round_up_one_digit(x):
    e = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / e - 1e-9) * e


# ------------------------------------------------------------------------------------------------ the inputs are what they claim
@pytest.mark.parametrize("D,B,kind", ALL_EMBLOSS)
def test_embloss_inputs_have_the_properties_the_cases_rely_on(D, B, kind):
    c = lp.embloss_case(D, B, kind)
    ub, pb, nb = c["ub"], c["pb"], c["nb"]
    assert ub.size == B < c["batch_size"] and c["u"].size == c["batch_size"] + B
    nrm = np.sqrt(c["sq3"])
    assert nrm[1] >= 2 * nrm[2] > 0                                   # the two item norms cannot be confused
    assert (nU := c["U0"].shape[0]) == 300 and (nI := c["I0"].shape[0]) == 400
    assert nI - 1 in pb and 0 in nb
    if B >= 15:
        m1, m2 = c["m"]
        assert m1 != m2 and np.sum(pb == 250) == m1 and np.sum(nb == 250) == m2 and min(m1, m2) >= 2
        assert 0.25 * B <= np.sum(ub == 7) <= 0.4 * B
        assert 0 in ub and nU - 1 in ub
    assert (nrm[0] == 0) == (kind == "zero_users")
    if kind == "saturated":
        assert np.sum(c["x"] > 40) >= 1 and np.sum(c["x"] < -40) >= 1
    term = c["reg_weight"] * c["reg_loss"]
    assert term >= 0.25 * (c["bpr_loss"] + term)                      # the term is at least a quarter of the loss
    # every D meets a B that is no multiple of its teams per workgroup, every B of the issue occurs
    teams = lambda d: 256 // (16 if d >= 64 or d not in (4, 8, 16, 32) else d // 4)
    for d in (4, 8, 16, 20, 32, 64, 96, 128, 200, 256):
        assert any(b % teams(d) for dd, b in lp.EMBLOSS_CASES if dd == d), d
    assert {b for _, b in lp.EMBLOSS_CASES} == {1, 15, 17, 255, 257, 2048}


@pytest.mark.parametrize("case", lp.STEP_CASES)
def test_step_inputs_have_the_properties_the_cases_rely_on(case):
    c = lp.step_case(*case)
    assert lp.SHARE[0] <= c["share"] <= lp.SHARE[1]
    ptr, _ = lp.step_graph()
    deg = np.diff(ptr)
    assert deg[0] == c["n_items"] and deg[5] == 0 and 5 in c["u"] and 0 in c["u"] and c["n_users"] - 1 in c["u"]
    nU, E0 = c["n_users"], c["E0"].astype(np.float64)
    nrm = [np.sqrt(np.sum(E0[nU + c[k]] ** 2)) for k in ("p", "n")]
    assert nrm[0] >= 2 * nrm[1]
    m1, m2 = c["m"]
    assert m1 != m2 and min(m1, m2) >= 2 and np.sum(c["p"] == 150) == m1 and np.sum(c["n"] == 150) == m2
    if case == lp.STEP_CASES[-1]:                                      # user 0's row alone needs two combine levels
        assert -(-int(deg[0]) // c["max_nnz"]) > 48


# ------------------------------------------------------------------------------------------------ floors and tolerances
def test_tolerances_are_eight_times_the_largest_floor(g4, g11):
    fe = [_embloss_floor(*k) for k in ALL_EMBLOSS]
    worst = {k: max(f[k] for f in fe) for k in fe[0]}
    print("largest floors, isolated term: %s" % {k: "%.2e" % v for k, v in worst.items()})
    row = max(worst[k] for k in ("row_u", "row_i", "row_u_G0", "row_i_G0"))
    assert math.isclose(lp.TOL_SQ, _round_up_one_digit(8 * worst["sq"]), rel_tol=1e-9), worst["sq"]
    assert math.isclose(lp.TOL_REG_LOSS, _round_up_one_digit(8 * worst["reg_loss"]), rel_tol=1e-9), worst["reg_loss"]
    assert math.isclose(lp.TOL_REG_ROW, _round_up_one_digit(8 * row), rel_tol=1e-9), row
    for f in fe:
        assert 4 * f["sq"] < lp.TOL_SQ and 4 * f["reg_loss"] < lp.TOL_REG_LOSS and f["loss0"] < parity.TOL_TABLE
        assert 4 * max(f[k] for k in ("row_u", "row_i", "row_u_G0", "row_i_G0")) < lp.TOL_REG_ROW
        assert f["reg_share_of_loss"] >= 0.25
    rw = float(g11["reg_weight"][0])
    fs = [_step_floor(case) for case in lp.STEP_CASES] + [_whole_floor("g4 inputs at g11", *_g4_at(g4, rw), lp.g4_terms_f64(g4, rw))]
    worst_row = max(f["row"] for f in fs)
    print("largest floors, whole step: row_err %.2e rel_err %.2e loss %.2e" % (worst_row, max(f["rel"] for f in fs),
                                                                             max(f["loss"] for f in fs)))
    assert math.isclose(lp.TOL_LGCN_ROW, _round_up_one_digit(8 * worst_row), rel_tol=1e-9), worst_row
    for f in fs:
        assert 4 * f["row"] < lp.TOL_LGCN_ROW and 4 * f["rel"] < TOL and 4 * f["loss"] < TOL
        assert lp.SHARE[0] <= f["share"] <= lp.SHARE[1]


# ------------------------------------------------------------------------------------------------ wrong versions of the term
MUTANTS = ("term_missing_from_gradient", "term_missing_from_loss", "negatives_by_positives_norm", "row_counted_once",
           "shared_item_positive_share_only", "sumsq_for_norm", "full_batch_size_in_short_batch")
NEED_REPEATS = ("row_counted_once", "shared_item_positive_share_only")     # nothing to get wrong in a batch of one


def _mutant(kind, U0, I0, u, p, n, reg_weight, full_B):
    """-> (EmbLoss as the wrong version reports it, gU, gI of reg_weight * EmbLoss as it computes them), float64"""
    U0, I0 = np.asarray(U0, dtype=np.float64), np.asarray(I0, dtype=np.float64)
    u, p, n = (np.asarray(a, dtype=np.int64) for a in (u, p, n))
    B, rw = float(u.size), float(F32(reg_weight))
    sq = np.array([np.sum(U0[u] ** 2), np.sum(I0[p] ** 2), np.sum(I0[n] ** 2)])
    den = np.sqrt(sq)
    reg_loss = float(den.sum() / B)
    cu, cp, cn = (np.bincount(i, minlength=r).astype(np.float64) for i, r in ((u, U0.shape[0]), (p, I0.shape[0]), (n, I0.shape[0])))
    if kind == "term_missing_from_gradient":
        return reg_loss, np.zeros_like(U0), np.zeros_like(I0)
    if kind == "term_missing_from_loss":
        reg_loss = 0.0
    if kind == "negatives_by_positives_norm":
        den[2] = den[1]
    if kind == "row_counted_once":
        cu, cp, cn = (np.minimum(c, 1.0) for c in (cu, cp, cn))
    if kind == "shared_item_positive_share_only":
        cn = np.where(cp > 0, 0.0, cn)
    if kind == "sumsq_for_norm":
        den = sq.copy()
    if kind == "full_batch_size_in_short_batch":
        reg_loss, B = reg_loss * B / full_B, float(full_B)
    part = [c * (rw / (B * d)) if d > 0 else 0.0 * c for c, d in zip((cu, cp, cn), den)]
    return reg_loss, part[0][:, None] * U0, (part[1] + part[2])[:, None] * I0


@pytest.mark.parametrize("D,B,kind", ALL_EMBLOSS)
def test_wrong_terms_are_rejected_by_the_isolated_checks(D, B, kind):
    c = lp.embloss_case(D, B, kind)
    for mutant in MUTANTS:
        if B < 15 and mutant in NEED_REPEATS:
            continue
        reg, gU, gI = _mutant(mutant, c["U0"], c["I0"], c["ub"], c["pb"], c["nb"], c["reg_weight"], c["batch_size"])
        e_loss = abs(reg - c["reg_loss"]) / c["reg_loss"]
        e_row = max(lp.row_err(gU, c["gU"]), lp.row_err(gI, c["gI"]))
        print("embloss D %d B %d %s %s: reg_loss err %.2e row_err %.2e" % (D, B, kind, mutant, e_loss, e_row))
        if mutant == "term_missing_from_loss":
            assert e_loss > 5 * lp.TOL_REG_LOSS
        else:
            assert e_row > 5 * lp.TOL_REG_ROW, (mutant, e_row)


def _whole_step_mutants(tag, nU, E0, u, p, n, rw, full_B, ref):
    bpr, reg, g_bpr, g_reg = ref
    for mutant in MUTANTS:
        reg_m, gU, gI = _mutant(mutant, E0[:nU], E0[nU:], u, p, n, rw, full_B)
        g_m, g = g_bpr + np.concatenate([gU, gI]), g_bpr + g_reg
        rw32 = float(F32(rw))
        e_loss = abs(rw32 * (reg_m - reg)) / (bpr + rw32 * reg)
        e_row = max(lp.row_err(g_m[:nU], g[:nU]), lp.row_err(g_m[nU:], g[nU:]))
        e_rel = max(rel_err(g_m[:nU], g[:nU]), rel_err(g_m[nU:], g[nU:]))
        print("%s rw %.3g %s: loss err %.2e row_err %.2e rel_err %.2e" % (tag, rw, mutant, e_loss, e_row, e_rel))
        yield mutant, e_loss, e_row, e_rel


@pytest.mark.parametrize("case", lp.STEP_CASES)
def test_wrong_terms_are_rejected_by_the_whole_step_checks(case):
    c = lp.step_case(*case)
    ref = (c["bpr_loss"], c["reg_loss"], c["g_bpr"], c["g_reg"])
    for mutant, e_loss, e_row, _ in _whole_step_mutants(str(case), c["n_users"], c["E0"], c["u"], c["p"], c["n"], c["reg_weight"],
                                                        c["B"] + c["B"] // 4 + 3, ref):
        if mutant == "term_missing_from_loss":
            assert e_loss > 5 * TOL
        else:
            assert e_row > 5 * lp.TOL_LGCN_ROW, (mutant, e_row)


def test_wrong_terms_on_g4_rejected_at_g11_and_accepted_by_the_old_bound(g4, g11):
    """g4's batch is one full batch of 256; for the batch-size mutant it stands for the short last batch of an epoch run at
    320, the ratio of the new cases"""
    nU, E0 = g4["U0"].shape[0], np.concatenate([g4["U0"], g4["I0"]])
    rw = float(g11["reg_weight"][0])
    for mutant, e_loss, e_row, _ in _whole_step_mutants("g4 inputs", nU, E0, g4["u"], g4["p"], g4["n"], rw, 320,
                                                        lp.g4_terms_f64(g4, rw)):
        if mutant == "term_missing_from_loss":
            assert e_loss > 5 * TOL
        else:
            assert e_row > 5 * lp.TOL_LGCN_ROW, (mutant, e_row)
    # ... and at the reference's default reg_weight, against the golden itself with the suite's old metric: all pass
    old = float(g4["hp"][1])
    assert old == 1e-5
    bpr, reg, g_bpr, g_reg = lp.g4_terms_f64(g4, old)
    for mutant in MUTANTS:
        reg_m, gU, gI = _mutant(mutant, g4["U0"], g4["I0"], g4["u"], g4["p"], g4["n"], old, 320)
        e = max(rel_err(g_bpr[:nU] + gU, g4["gU"]), rel_err(g_bpr[nU:] + gI, g4["gI"]))
        e_loss = abs(bpr + float(F32(old)) * reg_m - float(g4["loss"][0])) / float(g4["loss"][0])
        print("g4 inputs rw 1e-05 %s: rel_err of the gradient %.2e, loss err %.2e" % (mutant, e, e_loss))
        if mutant != "term_missing_from_loss":
            assert e < TOL, (mutant, e)


def test_loss_without_its_term_passes_the_old_bound_at_the_ml1m_shape():
    """the C3 inputs of test_hip_config_shapes.py: loss with and without reg_weight * EmbLoss, from the C oracle"""
    from test_hip_config_shapes import ml1m_shaped_pairs
    nU, nI, D, B, L = 6040, 3706, 64, 2048, 2
    uu, ii = ml1m_shaped_pairs()
    ptr = np.zeros(nU + 1, np.int64)
    np.cumsum(np.bincount(uu, minlength=nU), out=ptr[1:])
    rng = np.random.RandomState(7)
    E0 = (rng.standard_normal((nU + nI, D)) * 0.1).astype(np.float32)
    rows = rng.randint(0, uu.size, B)
    u, p, n = uu[rows], ii[rows], rng.randint(1, nI, B)
    rp, col, val = oracle.lightgcn_build_adj(nU, nI, ptr, ii.astype(np.int32))
    with_term, g = oracle.lightgcn_loss_grads(nU, nI, rp, col, val, E0, L, 1e-5, u, p, n)
    without, g0 = oracle.lightgcn_loss_grads(nU, nI, rp, col, val, E0, L, 0.0, u, p, n)
    e = abs(without - with_term) / with_term
    eg = max(rel_err(g0[:nU], g[:nU]), rel_err(g0[nU:], g[nU:]))
    print("ml-1m shape rw 1e-05: loss without the term %.2e off, gradient without the term %.2e off" % (e, eg))
    assert e < TOL
