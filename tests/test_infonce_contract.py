"""CPU checks around wr_infonce_loss_grad: the float64 restatement the GPU test compares against equals torch's float64
autograd of the reference's formula; the tolerances stand well above the fp32 floor of the reference itself on the GPU test's
own shapes; deliberately wrong results land above them on the figure meant to catch each; and the header, the binding and
the model flag exist."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infonce_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402

WEIGHT = 0.05


def _torch_f64(A, Bm, idx, tau, weight):
    """calc_ssl_loss for one side, written out from SGL.py:213-220, in float64 with torch.autograd"""
    import torch
    import torch.nn.functional as F
    A = torch.tensor(A, dtype=torch.float64, requires_grad=True)
    Bm = torch.tensor(Bm, dtype=torch.float64, requires_grad=True)
    idx = torch.from_numpy(idx)
    ssl_emb1 = F.normalize(A[idx], dim=1)
    ssl_emb2 = F.normalize(Bm[idx], dim=1)
    all_emb2 = F.normalize(Bm, dim=1)
    v1 = torch.sum(ssl_emb1 * ssl_emb2, dim=1)
    v2 = ssl_emb1.matmul(all_emb2.T)
    v1 = torch.exp(v1 / tau)
    v2 = torch.sum(torch.exp(v2 / tau), dim=1)
    loss = -torch.sum(torch.log(v1 / v2)) * weight
    gA, gB = torch.autograd.grad(loss, [A, Bm])
    return float(loss.detach()), gA.numpy(), gB.numpy()


@pytest.mark.parametrize("dup", [False, True])
def test_restatement_equals_torch_float64_autograd(dup):
    A, Bm, idx = R.make_case(700, 96, 32, 1, dup)
    Bm[5] = 0.0                    # clamped rows, outside and inside the batch, in both tables
    Bm[idx[2]] = 0.0
    A[idx[4]] = 0.0
    for tau in (0.2, 0.05):
        ref = _torch_f64(A, Bm, idx, tau, WEIGHT)
        got = R.infonce_f64(A, Bm, idx, tau, WEIGHT, block=40)
        assert abs(got[0] - ref[0]) <= 1e-12 * abs(ref[0])
        assert R.rel_err(got[1], ref[1]) <= 1e-12 and R.rel_err(got[2], ref[2]) <= 1e-12
        clamped = np.abs(ref[2][5]).max()
        assert clamped > 1e6 and np.abs(got[2][5] - ref[2][5]).max() <= 1e-12 * clamped


def test_tolerances_stand_above_the_fp32_floor_of_the_reference():
    """the stock fp32 formula against the restatement on the GPU test's shapes: 4 x floor < TOL for each figure"""
    worst = {k: 0.0 for k in R.TOL}
    for i, (n, B, D, tau) in enumerate(R.SHAPES):
        for dup in (False, True):
            A, Bm, idx = R.make_case(n, B, D, 100 + i, dup)
            fig = R.figures(R.stock_fp32(A, Bm, idx, tau, WEIGHT), R.infonce_f64(A, Bm, idx, tau, WEIGHT), idx)
            print(R.fmt("floor n=%d B=%d D=%d tau=%g dup=%d" % (n, B, D, tau, dup), fig))
            for k in worst:
                worst[k] = max(worst[k], fig[k])
    print(R.fmt("floor (largest)", worst))
    for k in R.TOL:
        assert 4.0 * worst[k] < R.TOL[k], (k, worst[k], R.TOL[k])
        assert R.TOL[k] <= 16.0 * R.FLOORS[k]          # and the bar is the 8 x rule of the recorded floors, not a loose one


def test_wrong_results_land_above_the_tolerances():
    n, B, D, tau = R.SHAPES[0]
    A, Bm, idx = R.make_case(n, B, D, 100, dup=True)
    ref = R.infonce_f64(A, Bm, idx, tau, WEIGHT)
    inb = np.zeros(n, bool)
    inb[idx] = True

    def fig(loss=None, gA=None, gB=None):
        return R.figures((ref[0] if loss is None else loss, ref[1] if gA is None else gA, ref[2] if gB is None else gB), ref, idx)

    clean = fig()
    assert all(v == 0.0 for v in clean.values())
    # out-of-batch rows 1 % too large: invisible in a whole-table max-norm, caught by gB_out
    g = ref[2].copy()
    g[~inb] *= 1.01
    assert fig(gB=g)["gB_out"] > R.TOL["gB_out"] and R.rel_err(g, ref[2]) < R.TOL["gB_in"]
    # the positive term missing
    wrong = R.infonce_f64(A, Bm, idx, tau, WEIGHT, positive=False)
    f = R.figures(wrong, ref, idx)
    assert f["loss"] > R.TOL["loss"] and f["gA"] > R.TOL["gA"] and f["gB_in"] > R.TOL["gB_in"]
    # one occurrence of the duplicated id missing from gA
    one = R.infonce_f64(A, Bm, idx[:1], tau, WEIGHT)[1]          # position 0 alone names the duplicated row
    g = ref[1].copy()
    g[idx[0]] -= one[idx[0]] * 0.5                                # even half of one occurrence out of B / 4
    assert fig(gA=g)["gA"] > R.TOL["gA"]
    # the projection term of the normalisation backward missing
    f = R.figures(R.infonce_f64(A, Bm, idx, tau, WEIGHT, project=False), ref, idx)
    assert f["gA"] > R.TOL["gA"] and f["gB_in"] > R.TOL["gB_in"] and f["gB_out"] > R.TOL["gB_out"]
    # sum exp missing its last item chunk (the 58 rows past the last full 64-row tile)
    f = R.figures(R.infonce_f64(A, Bm, idx, tau, WEIGHT, drop_last=n % 64), ref, idx)
    assert f["loss"] > R.TOL["loss"]


# ------------------------------------------------------------------------------------------------ interface
def test_header_declares_and_binding_binds_the_entry_points():
    from whisprrec_amd import abi
    src = open(os.path.join(ROOT, "include", "whisprrec_hip.h")).read()
    for name, nargs in (("wr_infonce_supported", 1), ("wr_infonce_workspace_bytes", 3), ("wr_infonce_loss_grad", 16)):
        m = re.search(r"\b(int32_t|int64_t)\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m is not None, name
        assert len(m.group(2).split(",")) == nargs, name
        assert name in abi.SIGNATURES and len(abi.SIGNATURES[name][1]) == nargs, name
    doc = src[src.index("K12"):src.index("wr_infonce_supported(int32_t D);")]
    for word in ("1e-12", "tau", "float atomics", "hipGraph", "clamped"):
        assert word in doc, word


def test_sgl_accepts_the_flag():
    from whisprrec_amd.sgl import SGL
    p = argparse.ArgumentParser()
    SGL.parse_model_args(p)
    assert p.parse_args([]).ssl_native == 0
    assert p.parse_args(["--ssl_native", "1"]).ssl_native == 1
    from whisprrec_amd import main as launcher
    args = launcher.build_args(["--model_name", "SGL", "--ssl_native", "1"])[0]
    assert args.ssl_native == 1


def test_workspace_is_monotone_and_has_no_batch_times_rows_term():
    from whisprrec_amd import abi
    if not os.path.exists(abi.LIB_PATH):
        pytest.skip("library not built")
    L = abi.lib()
    assert [L.wr_infonce_supported(d) for d in (32, 64, 128)] == [1, 1, 1]
    assert [L.wr_infonce_supported(d) for d in (0, 4, 48, 96, 256)] == [0, 0, 0, 0, 0]
    assert L.wr_infonce_workspace_bytes(1000, 100, 48) < 0 and "D" in abi.last_error()
    assert L.wr_infonce_workspace_bytes(0, 100, 64) < 0
    for D in (32, 64, 128):
        ns = [1, 100, 3706, 6040, 16383, 16384, 100003, 1_000_003, 8_000_000]
        Bs = [1, 127, 128, 129, 480, 2048, 4096, 65536, 1_000_000]
        grid = np.array([[L.wr_infonce_workspace_bytes(n, B, D) for B in Bs] for n in ns], dtype=np.int64)
        assert (grid > 0).all()
        assert (np.diff(grid, axis=0) >= 0).all() and (np.diff(grid, axis=1) >= 0).all()
        for n, B in ((3706, 480), (100_003, 2048), (1_000_003, 2048), (4_000_000, 65536)):
            w1, w2 = L.wr_infonce_workspace_bytes(n, B, D), L.wr_infonce_workspace_bytes(2 * n, 2 * B, D)
            assert w2 < 4 * w1 and w2 <= 2 * w1 + 4096            # linear in each: doubling both at most doubles it
        assert L.wr_infonce_workspace_bytes(1_000_003, 2048, D) < 2048 * 1_000_003 * 4 / 4
    # argument errors before any launch (no GPU here): NULL tables, loss-only needs both gradients NULL
    rc = L.wr_infonce_loss_grad(None, None, 100, 64, None, 10, 0.2, 1.0, None, 0, None, None, None, None, 0, None)
    assert rc == -1 and "NULL" in abi.last_error()
    rc = L.wr_infonce_loss_grad(None, None, 100, 48, None, 10, 0.2, 1.0, None, 0, None, None, None, None, 0, None)
    assert rc < 0 and "D=48" in abi.last_error()


def test_wrapper_refuses_cpu_tensors():
    import torch
    from whisprrec_amd import abi, hip_ops
    t = torch.zeros(8, 64)
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.infonce_loss_grad(t, t, torch.zeros(4, dtype=torch.int64), 0.2)
