"""wr_infonce_loss_grad (whisprrec_amd/csrc/wr_infonce.hip) on the GPU: parity with the float64 restatement of
tests/infonce_ref.py at its tolerances, bitwise reproducibility, parity with the stock torch path, the absence of any
[B, n] array at a million rows, bad ids, and SGL with --ssl_native 1 under the bounds of the existing SGL tests."""
import argparse
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infonce_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

WEIGHT = 0.05


def _dev():
    import torch
    return torch.device("cuda:0")


def _native(A, Bm, idx, tau, weight=WEIGHT, **kw):
    import torch
    from whisprrec_amd import hip_ops
    dev = _dev()
    loss, gA, gB = hip_ops.infonce_loss_grad(torch.from_numpy(A).to(dev), torch.from_numpy(Bm).to(dev), torch.from_numpy(idx).to(dev),
                                             tau, weight, **kw)
    torch.cuda.synchronize()
    return loss, gA, gB


def _triple(loss, gA, gB):
    return float(loss.cpu()[0]), gA.cpu().numpy(), gB.cpu().numpy()


def _check(tag, fig, scale=1.0):
    print(R.fmt(tag, fig))
    for k, v in fig.items():
        assert v <= scale * R.TOL[k], (tag, k, v, scale * R.TOL[k])


# ------------------------------------------------------------------------------------------------ parity with float64
@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("case", range(len(R.SHAPES)))
def test_parity_with_float64(case, dup):
    import torch
    n, B, D, tau = R.SHAPES[case]
    A, Bm, idx = R.make_case(n, B, D, 100 + case, dup)
    ref = R.infonce_f64(A, Bm, idx, tau, WEIGHT)
    loss, gA, gB = _native(A, Bm, idx, tau)
    _check("infonce n=%d B=%d D=%d tau=%g dup=%d" % (n, B, D, tau, dup), R.figures(_triple(loss, gA, gB), ref, idx))
    only, none_a, none_b = _native(A, Bm, idx, tau, grads=False)
    assert none_a is None and none_b is None
    assert torch.equal(only, loss)                      # the loss-only call: the same bits


def test_zero_rows_follow_the_clamped_branch():
    n, B, D, tau = R.SHAPES[0]
    A, Bm, idx = R.make_case(n, B, D, 7)
    inb = np.zeros(n, bool)
    inb[idx] = True
    z_out = int(np.flatnonzero(~inb)[5])
    z_in = int(idx[3])
    Bm[z_out] = 0.0
    Bm[z_in] = 0.0
    ref = R.infonce_f64(A, Bm, idx, tau, WEIGHT)
    got = _triple(*_native(A, Bm, idx, tau))
    _check("infonce zero rows (others)", R.figures(got, ref, idx, skip_rows=(z_out, z_in)))
    for tag, r in (("outside the batch", z_out), ("inside the batch", z_in)):
        e = R.rel_err(got[2][r], ref[2][r])
        print("parity infonce zero row %s: gB row rel %.2e (|g| %.2e)" % (tag, e, np.abs(ref[2][r]).max()))
        assert np.abs(ref[2][r]).max() > 1e6            # g / eps: the clamped branch, no projection
        assert e <= R.TOL["gB_in"]
    # a zero row of A inside the batch: the query's own clamped branch
    A[z_in] = 0.0
    ref = R.infonce_f64(A, Bm, idx, tau, WEIGHT)
    got = _triple(*_native(A, Bm, idx, tau))
    e = R.rel_err(got[1][z_in], ref[1][z_in])
    print("parity infonce zero row of A: gA row rel %.2e" % e)
    assert e <= R.TOL["gA"]
    _check("infonce zero rows in A and Bm (others)", R.figures(got, ref, idx, skip_rows=(z_out, z_in)))


# ------------------------------------------------------------------------------------------------ bits
def test_bitwise_reproducible_and_accumulate():
    import torch
    from whisprrec_amd import hip_ops
    dev = _dev()
    n, B, D, tau = 6040, 480, 64, 0.2
    A, Bm, idx = R.make_case(n, B, D, 11, dup=True)
    a = _native(A, Bm, idx, tau)
    a = tuple(t.clone() for t in a)
    A2, Bm2, idx2 = R.make_case(3706, 512, D, 12)
    _native(A2, Bm2, idx2, tau)                                         # other work in between
    b = _native(A, Bm, idx, tau)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # two sides into one loss word = the fp32 sum in that order
    l1 = _native(A2, Bm2, idx2, tau, grads=False)[0]
    l2 = a[0]
    acc = l1.clone()
    hip_ops.infonce_loss_grad(torch.from_numpy(A).to(dev), torch.from_numpy(Bm).to(dev), torch.from_numpy(idx).to(dev), tau, WEIGHT,
                              loss=acc, grads=False)
    assert torch.equal(acc, l1 + l2)
    # slices of one larger table as inputs and outputs: the same bits as separate tensors
    big1 = torch.from_numpy(np.concatenate([A2, A])).to(dev)
    big2 = torch.from_numpy(np.concatenate([Bm2, Bm])).to(dev)
    g1, g2 = torch.full_like(big1, 7.0), torch.full_like(big2, 7.0)
    off = A2.shape[0]
    ls, _, _ = hip_ops.infonce_loss_grad(big1[off:], big2[off:], torch.from_numpy(idx).to(dev), tau, WEIGHT, out=(g1[off:], g2[off:]))
    assert torch.equal(ls, a[0]) and torch.equal(g1[off:], a[1]) and torch.equal(g2[off:], a[2])
    assert bool((g1[:off] == 7.0).all()) and bool((g2[:off] == 7.0).all())


# ------------------------------------------------------------------------------------------------ the stock path
@pytest.mark.parametrize("n", [6040, 3706])
def test_parity_with_the_stock_path(n):
    B, D, tau = 2048, 64, 0.2
    A, Bm, idx = R.make_case(n, B, D, 21 + n)
    ref = R.infonce_f64(A, Bm, idx, tau, WEIGHT)
    stock = R.stock_fp32(A, Bm, idx, tau, WEIGHT, device="cuda:0")
    got = _triple(*_native(A, Bm, idx, tau))
    _check("infonce ml-1m side n=%d native vs f64" % n, R.figures(got, ref, idx))
    _check("infonce ml-1m side n=%d stock vs f64" % n, R.figures(stock, ref, idx))
    _check("infonce ml-1m side n=%d native vs stock" % n, R.figures(got, stock, idx), scale=2.0)


# ------------------------------------------------------------------------------------------------ no [B, n] matrix
def test_a_million_rows_without_a_score_matrix():
    import torch
    from whisprrec_amd import hip_ops
    dev = _dev()
    n, B, D, tau = 1_000_003, 2048, 64, 0.1
    g = torch.Generator(device="cpu").manual_seed(5)
    A = (torch.randn(n, D, generator=g) * 0.1 * (0.2 + 1.8 * torch.rand(n, 1, generator=g))).to(dev)
    Bm = (A.cpu() * 0.7 + torch.randn(n, D, generator=g) * 0.05).to(dev)
    idx = torch.randint(0, n, (B,), generator=g)
    idx[torch.randperm(B, generator=g)[:64]] = int(idx[0])
    idx = idx.to(dev)
    hip_ops.infonce_release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    loss, gA, gB = hip_ops.infonce_loss_grad(A, Bm, idx, tau, WEIGHT)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    ws = hip_ops.infonce_workspace_bytes(n, B, D)
    outputs = 2 * n * D * 4
    print("infonce n=%d B=%d: peak above the inputs %.1f MB = outputs %.1f MB + workspace %.1f MB + %.1f MB; one [B, n] fp32 matrix "
          "would be %.1f MB" % (n, B, peak / 2**20, outputs / 2**20, ws / 2**20, (peak - outputs - ws) / 2**20, B * n * 4 / 2**20))
    assert peak < outputs + ws + (64 << 20)
    assert ws < B * n * 4 / 4
    hip_ops.infonce_release_workspaces()
    # float64 on the device, in column chunks
    wt = WEIGHT / tau
    A64, B64 = A.double(), Bm.double()
    nB = B64.norm(dim=1, keepdim=True)
    K = B64 / nB.clamp_min(R.EPS)
    del B64
    a = A64[idx]
    del A64
    nA = a.norm(dim=1, keepdim=True)
    Q = a / nA.clamp_min(R.EPS)
    Z = torch.zeros(B, 1, dtype=torch.float64, device=dev)
    G = torch.zeros(B, D, dtype=torch.float64, device=dev)
    for lo in range(0, n, 16384):
        E = torch.exp((Q @ K[lo:lo + 16384].T - 1.0) / tau)
        Z += E.sum(dim=1, keepdim=True)
        G += E @ K[lo:lo + 16384]
    Kp = K[idx]
    ref_loss = WEIGHT * float((torch.log(Z) + 1.0 / tau - (Q * Kp).sum(dim=1, keepdim=True) / tau).sum())
    gq = wt * (G / Z - Kp)
    ga = (gq - Q * (Q * gq).sum(dim=1, keepdim=True)) / nA
    ref_gA = torch.zeros(n, D, dtype=torch.float64, device=dev).index_add_(0, idx, ga)
    uniq = torch.unique(idx)
    e_loss = abs(float(loss[0]) - ref_loss) / abs(ref_loss)
    e_gA = R.rel_err(gA[uniq].cpu().numpy(), ref_gA[uniq].cpu().numpy())
    outside = torch.ones(n, dtype=torch.bool, device=dev)
    outside[uniq] = False
    assert not bool(gA[outside].any())
    del ref_gA
    # gB on the batch rows and on 4,096 sampled other rows
    cand = torch.randperm(n, generator=g)[:8192].to(dev)
    sample = cand[outside[cand]][:4096]
    rows = torch.cat([uniq, sample])
    P = torch.exp((Q @ K[rows].T - 1.0) / tau) / Z                       # [B, rows]
    gk = wt * (P.T @ Q)
    hit = (idx.unsqueeze(1) == uniq.unsqueeze(0)).double()               # [B, uniq]
    gk[:uniq.numel()] -= wt * (hit.T @ Q)
    Kr = K[rows]
    ref_gB = (gk - Kr * (Kr * gk).sum(dim=1, keepdim=True)) / nB[rows]
    got_gB = gB[rows].cpu().numpy()
    ref_gB = ref_gB.cpu().numpy()
    u = uniq.numel()
    fig = {"loss": e_loss, "gA": e_gA, "gB_in": R.rel_err(got_gB[:u], ref_gB[:u]), "gB_out": R.rel_err(got_gB[u:], ref_gB[u:])}
    assert sample.numel() == 4096
    _check("infonce n=%d B=%d D=%d tau=%g (float64 on the device)" % (n, B, D, tau), fig)


# ------------------------------------------------------------------------------------------------ bad ids
def test_bad_ids_raise_and_are_never_dereferenced():
    import torch
    from whisprrec_amd import hip_ops
    dev = _dev()
    n, B, D, tau = 3706, 512, 64, 0.1
    A, Bm, idx = R.make_case(n, B, D, 31)
    idx[17] = n
    idx[400] = -1
    At, Bt, it = torch.from_numpy(A).to(dev), torch.from_numpy(Bm).to(dev), torch.from_numpy(idx).to(dev)
    with pytest.raises(IndexError):
        hip_ops.infonce_loss_grad(At, Bt, it, tau, WEIGHT, validate=True)
    loss, gA, gB = hip_ops.infonce_loss_grad(At, Bt, it, tau, WEIGHT, validate=False)     # clamped, not dereferenced
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(gA).all()) and bool(torch.isfinite(gB).all())
    idx[17], idx[400] = n - 1, 0                                                          # what the clamp makes of them
    good = hip_ops.infonce_loss_grad(At, Bt, torch.from_numpy(idx).to(dev), tau, WEIGHT)
    assert torch.equal(good[0], loss) and torch.equal(good[1], gA) and torch.equal(good[2], gB)
    with pytest.raises(Exception):
        hip_ops.infonce_loss_grad(At[:, :48].contiguous(), Bt[:, :48].contiguous(), it, tau)   # D = 48: refused before a launch
    assert not hip_ops.infonce_supports(48) and all(hip_ops.infonce_supports(d) for d in (32, 64, 128))


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def g7():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "g7_sgl.npz"))


def _clicked(g7):
    ptr, idx = g7["clicked_ptr"], g7["clicked_idx"]
    return {u: set(int(x) for x in idx[ptr[u]:ptr[u + 1]]) for u in range(len(ptr) - 1) if ptr[u + 1] > ptr[u]}


def _g7_model(g7, t, dev, **kw):
    import torch
    from whisprrec_amd import host
    from whisprrec_amd.sgl import SGL
    nU, nI = int(g7["shape"][0]), int(g7["shape"][1])
    corpus = host.Corpus(nU, nI, {"train": {"user_id": [], "item_id": []}, "dev": {"user_id": [], "item_id": []},
                                  "test": {"user_id": [], "item_id": []}}, _clicked(g7), {})
    hp = g7[t + "_hp"]
    base = dict(device=dev, model_path="/tmp/wr_sgl_nce.pt", buffer=1, num_neg=1, test_all=1, embedding_size=int(g7["shape"][2]),
                gcn_layers=int(g7["shape"][3]), type=t.upper(), reg_weight=float(hp[0]), ssl_tau=float(hp[1]),
                ssl_weight=float(hp[2]), drop_ratio=float(hp[3]))
    base.update(kw)
    m = SGL(argparse.Namespace(**base), corpus).to(dev)
    with torch.no_grad():
        m.user_embedding.weight.copy_(torch.from_numpy(g7[t + "_U0"]))
        m.item_embedding.weight.copy_(torch.from_numpy(g7[t + "_I0"]))
    return m


def _g7_batch(g7, dev):
    import torch
    return {k: torch.from_numpy(g7[s]).to(dev) for k, s in (("user_id", "u"), ("pos_item", "p"), ("neg_items", "n"))}


@pytest.mark.parametrize("t", ["ed", "nd", "rw"])
def test_sgl_native_ssl_matches_the_reference(g7, t):
    """the bounds of test_sgl_views.py::test_loss_grads_full_predict_match_reference, with --ssl_native 1"""
    from conftest import rel_err
    dev = _dev()
    m = _g7_model(g7, t, dev, ssl_native=1)
    assert m._use_ssl_native()
    random.seed(2024)
    m.graph_construction()
    m.train()
    loss = m.predict(_g7_batch(g7, dev))
    e_loss = abs(float(loss.detach()) - float(g7[t + "_loss"][0])) / abs(float(g7[t + "_loss"][0]))
    loss.backward()
    e_u = rel_err(m.user_embedding.weight.grad.cpu().numpy(), g7[t + "_gU"])
    e_i = rel_err(m.item_embedding.weight.grad.cpu().numpy(), g7[t + "_gI"])
    print("parity sgl %s --ssl_native 1: loss %.2e gU %.2e gI %.2e" % (t, e_loss, e_u, e_i))
    assert e_loss < 1e-5 and e_u < 2e-5 and e_i < 2e-5


def _parent_loss_and_grad(m, u, p, n):
    """SGL._loss_and_grad as it was before --ssl_native existed, kept here: what the flag at 0 must still compute"""
    import torch
    import torch.nn.functional as F
    from whisprrec_amd import hip_ops

    def ssl_fn(u, p, E1, E2):
        nU, tau = m.n_users, m.ssl_tau

        def side(idx, A, Bm):
            e1 = F.normalize(A[idx], dim=1)
            e2 = F.normalize(Bm[idx], dim=1)
            all2 = F.normalize(Bm, dim=1)
            v1 = torch.exp(torch.sum(e1 * e2, dim=1) / tau)
            v2 = torch.sum(torch.exp(e1.matmul(all2.T) / tau), dim=1)
            return -torch.sum(torch.log(v1 / v2))

        return (side(p, E1[nU:], E2[nU:]) + side(u, E1[:nU], E2[:nU])) * m.ssl_weight

    with torch.no_grad():
        nU, L, B = m.n_users, m.gcn_layers, u.numel()
        U0, I0 = m.user_embedding.weight.data, m.item_embedding.weight.data
        E0 = torch.cat([U0, I0], dim=0)
        gm, g1, g2 = m._graph("train"), m._graph("sub1"), m._graph("sub2")
        Em, E1, E2 = gm.propagate(E0, L), g1.propagate(E0, L), g2.propagate(E0, L)
        idx = torch.cat([u, p + nU, n + nU])
        rows = hip_ops.gather_rows(Em, idx)
        ue, pe, ne = rows[:B], rows[B:2 * B], rows[2 * B:]
        x = (ue * pe).sum(dim=1) - (ue * ne).sum(dim=1)
        l1 = F.softplus(-x).sum()
        coef = -torch.sigmoid(-x).unsqueeze(1)
        gEm = torch.zeros_like(Em)
        hip_ops.scatter_add_rows(gEm, idx, torch.cat([coef * (pe - ne), coef * ue, -coef * ue]))
        sq = hip_ops.embloss_sumsq(U0, I0, u, p, n)
        reg = torch.sqrt(sq).sum() / B
        with torch.enable_grad():
            E1r, E2r = E1.detach().requires_grad_(True), E2.detach().requires_grad_(True)
            ssl = ssl_fn(u, p, E1r, E2r)
            gE1, gE2 = torch.autograd.grad(ssl, [E1r, E2r])
        loss = l1 + reg * m.reg_weight + ssl.detach()
        gE0 = gm.propagate(gEm, L, transpose=True)
        gE0 += g1.propagate(gE1.contiguous(), L, transpose=True)
        gE0 += g2.propagate(gE2.contiguous(), L, transpose=True)
        plan = hip_ops.BatchPlan(u, p, n, B, nU, m.n_items, builder="small" if B <= 4096 else "generic", hot=False, validate=True)
        hip_ops.embloss_grad(U0, I0, plan, 0, sq, m.reg_weight, gE0[:nU], gE0[nU:])
        return loss, gE0


def test_flag_at_zero_changes_nothing(g7):
    """--ssl_native 0 (and no flag at all): the bits of the step as it was, from a copy of it kept in this file.  torch's
    backward of A[idx] adds duplicates with float atomics unless told otherwise, so both runs ask for deterministic
    algorithms: the comparison is about the code path, not about the order of those atomics."""
    import torch
    dev = _dev()
    before = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        for kw in ({}, {"ssl_native": 0}):
            m = _g7_model(g7, "ed", dev, **kw)
            assert not m._use_ssl_native()
            random.seed(2024)
            m.graph_construction()
            b = _g7_batch(g7, dev)
            u, p, n = b["user_id"].reshape(-1), b["pos_item"].reshape(-1), b["neg_items"].reshape(-1)
            loss, g = m._loss_and_grad(u, p, n)
            loss0, g0 = _parent_loss_and_grad(m, u, p, n)
            assert torch.equal(loss, loss0) and torch.equal(g, g0)
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])


def test_unsupported_embedding_size_keeps_the_stock_path(g7, caplog):
    import logging
    import torch
    from whisprrec_amd import host
    from whisprrec_amd.sgl import SGL
    dev = _dev()
    nU, nI = int(g7["shape"][0]), int(g7["shape"][1])
    corpus = host.Corpus(nU, nI, {"train": {"user_id": [], "item_id": []}, "dev": {"user_id": [], "item_id": []},
                                  "test": {"user_id": [], "item_id": []}}, _clicked(g7), {})
    args = argparse.Namespace(device=dev, model_path="/tmp/wr_sgl_nce.pt", buffer=1, num_neg=1, test_all=1, embedding_size=48,
                              gcn_layers=2, type="ED", reg_weight=1e-4, ssl_tau=0.2, ssl_weight=0.05, drop_ratio=0.1, ssl_native=1)
    torch.manual_seed(0)
    m = SGL(args, corpus).to(dev)
    random.seed(3)
    m.graph_construction()
    with caplog.at_level(logging.WARNING):
        l1 = m.predict(_g7_batch(g7, dev))
        l2 = m.predict(_g7_batch(g7, dev))
    assert bool(torch.isfinite(l1)) and bool(torch.isfinite(l2))
    assert sum("ssl_native" in r.getMessage() for r in caplog.records) == 1        # logged once


def test_end_to_end_sgl_run_with_native_ssl(tmp_path):
    """the G9 'sgl' run of tests/test_reader.py through HipRunner with --ssl_native 1, under that test's bounds"""
    import torch
    from whisprrec_amd import main as launcher
    golden = os.path.join(os.path.dirname(__file__), "golden")
    g8 = np.load(os.path.join(golden, "g8_reader.npz"))
    g9 = np.load(os.path.join(golden, "g9_end_to_end.npz"))
    d = tmp_path / "ml-100k"
    d.mkdir()
    with open(d / "ml-100k.inter", "w") as f:
        f.write("user_id:token\titem_id:token\trating:float\ttimestamp:float\n")
        for a, b, c, t in zip(g8["in_user"].tolist(), g8["in_item"].tolist(), g8["in_rating"].tolist(), g8["in_time"].tolist()):
            f.write("%d\t%d\t%d\t%d\n" % (a, b, c, t))
    lr, l2, epochs = g9["sgl_hp"]
    argv = ["--gcn_layers", "2", "--reg_weight", "1e-4", "--type", "ED", "--ssl_tau", "0.2", "--ssl_weight", "0.05", "--drop_ratio", "0.1",
            "--ssl_native", "1", "--model_name", "SGL", "--runner_name", "HipRunner", "--dataset", "ml-100k", "--path", str(tmp_path) + "/",
            "--epoch", str(int(epochs)), "--batch_size", "1024", "--eval_batch_size", "2048", "--optimizer", "Adam", "--lr", repr(float(lr)),
            "--l2", repr(float(l2)), "--log_file", str(tmp_path / "log.txt"), "--model_path", str(tmp_path / "m.pt"),
            "--num_workers", "0", "--topk", "10,20", "--metric", "NDCG, HR", "--random_seed", "3407"]
    args, model_class, reader_class, runner_class = launcher.build_args(argv)
    assert args.ssl_native == 1                                       # main.py passes the model's flag through
    launcher.init_seed(args.random_seed)
    args.device = torch.device("cuda")
    corpus = reader_class(args).corpus()
    model = model_class(args, corpus).to(args.device)
    data = {ph: model_class.Dataset(model, corpus, ph) for ph in ("train", "dev", "test")}
    run = runner_class(args)
    losses, devs = [], []
    for epoch in range(args.epoch):
        losses.append(run.fit(data["train"], epoch=epoch + 1))
        devs.append(run.evaluate(data["dev"], run.topk[:1], run.metrics))
    test = run.evaluate(data["test"], run.topk, run.metrics)
    assert model._use_ssl_native()
    print("parity sgl g9 --ssl_native 1: loss rel %.2e" % np.max(np.abs(np.asarray(losses) / g9["sgl_loss"] - 1.0)))
    assert np.allclose(losses, g9["sgl_loss"], rtol=5e-5, atol=0)
    flips = 6.0 / len(data["dev"])
    dev = np.asarray([[dd[k] for k in g9["sgl_dev_keys"]] for dd in devs])
    assert np.abs(dev - g9["sgl_dev"]).max() <= flips, np.abs(dev - g9["sgl_dev"]).max()
    tst = np.asarray([test[k] for k in g9["sgl_test_keys"]])
    assert np.abs(tst - g9["sgl_test"]).max() <= flips


def test_captured_step_graph_equals_eager_loop_with_native_ssl():
    """HipRunner's hipGraph of the SGL step with the InfoNCE kernels inside: replays equal the eager loop bit for bit"""
    import torch
    from whisprrec_amd import host, runner
    from whisprrec_amd.sgl import SGL
    dev = _dev()
    rng = np.random.RandomState(3)
    nU, nI, B = 500, 300, 256
    sets, tu, ti = {}, [], []
    for uu in range(nU):
        items = np.unique(rng.randint(0, nI - 40, rng.randint(4, 30)))
        sets[uu] = set(items.tolist()); tu += [uu] * len(items); ti += items.tolist()
    frames = {"train": {"user_id": np.asarray(tu), "item_id": np.asarray(ti)},
              "dev": {"user_id": np.zeros(0, np.int64), "item_id": np.zeros(0, np.int64)},
              "test": {"user_id": np.zeros(0, np.int64), "item_id": np.zeros(0, np.int64)}}
    corpus = host.Corpus(nU, nI, frames, sets, {u: set() for u in sets})
    assert len(tu) >= 10 * B
    out = []
    for graphs in (0, 1):
        random.seed(1); np.random.seed(1); torch.manual_seed(1)
        args = argparse.Namespace(device=dev, model_path="/tmp/wr_sgl_nce.pt", buffer=1, num_neg=1, test_all=1, embedding_size=64,
                                  gcn_layers=2, type="ED", reg_weight=1e-4, ssl_tau=0.2, ssl_weight=0.05, drop_ratio=0.1, ssl_native=1,
                                  optimizer="Adam", lr=2e-3, l2=0.0, epoch=1, check_epoch=1, test_epoch=-1, early_stop=10, batch_size=B,
                                  eval_batch_size=256, num_workers=0, pin_memory=0, topk="10", metric="NDCG", device_epoch_prep=0,
                                  hip_graphs=graphs)
        m = SGL(args, corpus).to(dev)
        ds = SGL.Dataset(m, corpus, "train")
        r = runner.HipRunner(args)
        l1, l2 = r.fit(ds, epoch=1), r.fit(ds, epoch=2)
        assert m._use_ssl_native()
        assert (getattr(r, "_graph_cache", None) is not None) == bool(graphs)
        out.append((l1, l2, m.user_embedding.weight.detach().clone(), m.item_embedding.weight.detach().clone(), m.optimizer.t))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert torch.equal(out[0][2], out[1][2]) and torch.equal(out[0][3], out[1][3])
    assert out[0][4] == out[1][4]
