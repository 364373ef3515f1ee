"""The kernels of LightGCN's / SGL's EmbLoss term on their own (wr_rows.hip: embloss_sumsq + finish, lightgcn_tail_fwd + finish,
embloss_grad) against the float64 reference of oracle/lightgcn_parity.py, at every branch of WR_DISPATCH_D up to 256 and
batch sizes around the teams-per-workgroup counts.  Inputs (lightgcn_parity.embloss_case): one user takes 30 % of the batch,
one item is m1 times a positive and m2 times a negative, positives come from rows scaled x4 (the two item norms differ by
more than a factor 2), row 0 and the last row of both tables occur, and the batch is the short last one (k = 1) of a plan of
two.  Tolerances: lightgcn_parity.TOL_*, derived in tests/test_lightgcn_power.py, which also shows that seven wrong versions
of the term fail these checks by a factor 5 or more."""
import numpy as np
import pytest
import torch

from oracle import lightgcn_parity as lp
from oracle import parity

pytestmark = pytest.mark.gpu

CASES = tuple((D, B, "plain") for D, B in lp.EMBLOSS_CASES) + tuple((D, B, k) for k, D, B in lp.EMBLOSS_SPECIAL)


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _rel(got, want):
    return abs(float(got) - want) / abs(want)


@pytest.mark.parametrize("D,B,kind", CASES)
def test_sums_of_squares_and_loss_tail_match_float64(D, B, kind):
    from whisprrec_amd import hip_ops
    c = lp.embloss_case(D, B, kind)
    U0, I0, Ua, Ia = (_t(c[k]) for k in ("U0", "I0", "Ua", "Ia"))
    u, p, n = (_t(c[k]) for k in ("ub", "pb", "nb"))
    rw, want = c["reg_weight"], c["sq3"]
    sq_a = hip_ops.embloss_sumsq(U0, I0, u, p, n).cpu().numpy().astype(np.float64)
    loss0, sq_b = hip_ops.lightgcn_loss(Ua, Ia, U0, I0, u, p, n, 0.0)
    loss1, sq_c = hip_ops.lightgcn_loss(Ua, Ia, U0, I0, u, p, n, rw)
    assert torch.equal(sq_b, sq_c)
    sq_b = sq_b.cpu().numpy().astype(np.float64)
    live = want > 0
    e_a, e_b = (float(np.max(np.abs(s[live] - want[live]) / want[live])) for s in (sq_a, sq_b))
    term = float(np.float32(rw)) * c["reg_loss"]
    e0 = _rel(loss0, c["bpr_loss"])
    e_term = abs((float(loss1) - float(loss0)) - term) / term
    print("embloss D %d B %d %s: sq3 err sumsq %.2e tail %.2e (tol %.0e) | loss at rw 0 %.2e (tol %.0e) | loss(rw %.3g) - loss(0) "
          "against rw * EmbLoss %.2e (tol %.0e), the term is %.2f of the loss" % (
              D, B, kind, e_a, e_b, lp.TOL_SQ, e0, parity.TOL_TABLE, rw, e_term, lp.TOL_REG_LOSS, term / (c["bpr_loss"] + term)),
          flush=True)
    assert np.all(sq_a[~live] == 0) and np.all(sq_b[~live] == 0)        # a block of zero rows: exactly zero
    assert e_a < lp.TOL_SQ and e_b < lp.TOL_SQ
    assert loss0.shape == (1,) and np.isfinite(float(loss0)) and np.isfinite(float(loss1))
    assert e0 < parity.TOL_TABLE
    assert term >= 0.25 * (c["bpr_loss"] + term)
    assert e_term < lp.TOL_REG_LOSS


@pytest.mark.parametrize("D,B,kind", CASES)
def test_embloss_grad_matches_float64_per_row(D, B, kind):
    from whisprrec_amd import hip_ops
    c = lp.embloss_case(D, B, kind)
    nU, nI = c["U0"].shape[0], c["I0"].shape[0]
    U0, I0 = _t(c["U0"]), _t(c["I0"])
    ub, pb, nb = c["ub"], c["pb"], c["nb"]
    nrm = np.sqrt(c["sq3"])
    assert nrm[1] >= 2 * nrm[2]                                           # the two item norms cannot be taken for each other
    plan = hip_ops.BatchPlan(_t(c["u"]), _t(c["p"]), _t(c["n"]), c["batch_size"], nU, nI, builder="small", hot=False)
    assert plan.n_batches == 2 and plan.batch_len(1) == B < plan.batch_size
    sq = hip_ops.embloss_sumsq(U0, I0, _t(ub), _t(pb), _t(nb))
    out_u, out_i = np.setdiff1d(np.arange(nU), ub), np.setdiff1d(np.arange(nI), np.concatenate([pb, nb]))
    for tag, G0u, G0i in (("zeros", np.zeros_like(c["G0u"]), np.zeros_like(c["G0i"])), ("G0", c["G0u"], c["G0i"])):
        runs = []
        for _ in range(2):
            gu, gi = _t(G0u), _t(G0i)
            hip_ops.embloss_grad(U0, I0, plan, 1, sq, c["reg_weight"], gu, gi)
            runs.append((gu.cpu().numpy(), gi.cpu().numpy()))
        (gu, gi), again = runs
        assert np.array_equal(gu, again[0]) and np.array_equal(gi, again[1])            # reproducible
        assert np.isfinite(gu).all() and np.isfinite(gi).all()
        # rows of no occurrence in batch 1 — those of batch 0 among them — keep their bits
        assert np.array_equal(gu[out_u].view(np.int32), G0u[out_u].view(np.int32))
        assert np.array_equal(gi[out_i].view(np.int32), G0i[out_i].view(np.int32))
        if kind == "zero_users":                                                        # zero norm: nothing is added
            assert np.array_equal(gu.view(np.int32), G0u.view(np.int32))
        lp.check_rows("embloss_grad D %d B %d %s into %s" % (D, B, kind, tag), gu, gi, G0u.astype(np.float64) + c["gU"],
                      G0i.astype(np.float64) + c["gI"], lp.TOL_REG_ROW, ub, pb, nb, scale_U=c["gU"], scale_I=c["gI"], sq3=c["sq3"])
