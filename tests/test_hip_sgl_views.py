"""SGL's views built on the device (--views_native 1: wr_views.hip through hip_ops.sgl_views_build) against the host functions
on the restated keep set (tests/sgl_views_ref.py): every structural array exactly, every value bit for bit, forward and
transposed, edge and node dropout."""
import argparse
import random

import numpy as np
import pytest

import sgl_views_ref as ref

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _build(N, rows, cols, kind, ratio, seed, version=1, view=0):
    """-> (device view [forward, transposed] as host dicts, expected [forward, transposed])"""
    import torch
    from whisprrec_amd import hip_ops
    base = hip_ops.sgl_views_base(rows, cols, N, _dev())
    errs = []
    (parts,) = hip_ops.sgl_views_build(base, kind, [(ref.n_select(kind, rows, N, ratio), ref.stream_ids(kind, version, view))], seed,
                                       err_words=errs)
    got = [dict(row_ptr=p[0].cpu().numpy(), col=p[1].cpu().numpy(), val=p[2].cpu().numpy(), chunk_ptr=p[3].cpu().numpy(),
                chunk_row=p[4].cpu().numpy(), levels=p[4]._wr_levels) for p in parts]
    assert int(torch.cat(errs).sum()) == 0
    mask = ref.keep_mask(kind, rows, cols, N, ratio, seed, version, view)
    return got, ref.expected(N, rows, cols, mask)


def _assert_same(got, want):
    for d, name in ((0, "forward"), (1, "transposed")):
        g, w = got[d], want[d]
        for k in ("row_ptr", "col", "chunk_ptr", "chunk_row"):
            assert g[k].dtype == w[k].dtype and np.array_equal(g[k], w[k]), (name, k)
        assert g["levels"] == w["levels"], name
        assert g["val"].dtype == np.float32 and np.array_equal(g["val"].view(np.int32), w["val"].view(np.int32)), name


@pytest.mark.parametrize("kind", ["ED", "ND"])
def test_toy_graph(kind):
    """7 nodes, 10 edges, half dropped: emptied rows, dis_tab[0] on a kept edge, cycle walking for N and E
    (test_sgl_views_native_contract.py checks that this keep set has them)"""
    N, r, c = ref.toy()
    got, want = _build(N, r, c, kind, ref.TOY["ratio"], ref.TOY_SEED[kind])
    _assert_same(got, want)
    assert (got[0]["val"] > 1e4).any()


@pytest.mark.parametrize("kind", ["ED", "ND"])
def test_hub_graph_at_the_chunk_boundaries(kind):
    """a 5400-edge hub row (two combine levels, base chunks inside one row) and rows of view degree 0, 96 and 97"""
    N, r, c = ref.hub_graph()
    got, want = _build(N, r, c, kind, ref.HUB["ratio"], ref.HUB_SEED[kind])
    assert {0, 96, 97} <= set(np.diff(got[0]["row_ptr"]).tolist()) and got[0]["levels"] == 2
    _assert_same(got, want)


@pytest.fixture(scope="module")
def g7():
    return ref.g7()


@pytest.mark.parametrize("kind", ["ED", "ND"])
def test_g7_graph_at_its_ratio(g7, kind):
    N, r, c = ref.g7_graph(g7)
    for view in (0, 1):
        got, want = _build(N, r, c, kind, float(g7[kind.lower() + "_hp"][3]), 2024, version=2, view=view)
        _assert_same(got, want)


def test_rate_zero_is_the_pinned_train_graph(g7):
    N, r, c = ref.g7_graph(g7)
    got, want = _build(N, r, c, "ED", 0.0, 2024)
    _assert_same(got, want)
    rows = np.repeat(np.arange(N), np.diff(got[0]["row_ptr"])).astype(np.int32)
    assert np.array_equal(rows, g7["ed_g0_row"]) and np.array_equal(got[0]["col"], g7["ed_g0_col"])
    assert np.array_equal(got[0]["val"].view(np.int32), g7["ed_g0_val"].view(np.int32))
    got, want = _build(N, r, c, "ND", 0.0, 2024)
    _assert_same(got, want)
    assert np.array_equal(got[0]["val"].view(np.int32), g7["ed_g0_val"].view(np.int32))


@pytest.mark.parametrize("kind", ["ED", "ND"])
def test_nothing_kept(g7, kind):
    """ED at ratio 1 keeps int(E * 0) = 0 edges, ND at ratio 1 drops every node: all rows empty, one empty chunk each"""
    N, r, c = ref.g7_graph(g7)
    got, want = _build(N, r, c, kind, 1.0, 2024)
    _assert_same(got, want)
    for d in (0, 1):
        assert got[d]["col"].size == 0 and not got[d]["row_ptr"].any()
        assert np.array_equal(got[d]["chunk_row"], np.arange(N)) and not got[d]["chunk_ptr"].any() and got[d]["levels"] == 1


@pytest.mark.parametrize("ratio", [0.0, 0.5])
def test_one_edge(ratio):
    """E = 1: the one symmetric base with a single directed edge is a loop; node 0 has an empty base row"""
    r, c = np.asarray([1]), np.asarray([1])
    for kind in ("ED", "ND"):
        got, want = _build(2, r, c, kind, ratio, 11)
        _assert_same(got, want)
        if ratio == 0.0:
            assert got[0]["col"].tolist() == [1] and got[1]["row_ptr"].tolist() == [0, 0, 1]
        elif kind == "ED":
            assert got[0]["col"].size == 0                       # int(1 * 0.5) = 0 edges kept


def test_spmm_chunks_device_equals_the_host_cut():
    import torch
    from whisprrec_amd import hip_ops
    N, r, c = ref.hub_graph()
    rp = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=N), out=rp[1:])
    for row_ptr in (rp, np.zeros(5, np.int64), np.asarray([0, 96, 96, 193, 193 + 48 * 96, 193 + 48 * 96 + 1])):
        cptr, crow = hip_ops.spmm_chunks(row_ptr)
        dptr, drow = hip_ops.spmm_chunks_device(torch.from_numpy(row_ptr).to(_dev()))
        assert np.array_equal(dptr.cpu().numpy(), cptr.numpy()) and np.array_equal(drow.cpu().numpy(), crow.numpy())
        assert drow._wr_levels == crow._wr_levels and drow.dtype == torch.int32 and dptr.dtype == torch.int64


def test_base_refuses_what_is_not_a_base():
    from whisprrec_amd import abi, hip_ops
    with pytest.raises(ValueError):
        hip_ops.sgl_views_base(np.asarray([0]), np.asarray([1]), 2, _dev())               # not symmetric
    with pytest.raises(ValueError):
        hip_ops.sgl_views_base(np.asarray([0, 0, 1, 1]), np.asarray([1, 1, 0, 0]), 2, _dev())   # a pair twice
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.sgl_views_base(np.zeros(0, np.int64), np.zeros(0, np.int64), 2, _dev())   # no edge


@pytest.mark.parametrize("kind", ["ED", "ND"])
def test_propagation_from_device_parts_equals_the_host_upload(kind):
    import torch
    from whisprrec_amd import hip_ops, sgl
    N, r, c = ref.hub_graph()
    dev = _dev()
    base = hip_ops.sgl_views_base(r, c, N, dev)
    (parts,) = hip_ops.sgl_views_build(base, kind, [(ref.n_select(kind, r, N, 0.1), ref.stream_ids(kind, 3, 1))], 5)
    g_dev = sgl.CsrGraph.from_device_parts(N, *parts)
    mask = ref.keep_mask(kind, r, c, N, 0.1, 5, 3, 1)
    g_host = sgl.CsrGraph(N, *sgl.norm_csr(N, r[mask], c[mask]), dev)
    E0 = torch.from_numpy(np.random.RandomState(0).standard_normal((N, 32)).astype(np.float32)).to(dev)
    for transpose in (False, True):
        assert torch.equal(g_dev.propagate(E0, 2, transpose=transpose), g_host.propagate(E0, 2, transpose=transpose))


# ------------------------------------------------------------------------------------------------ model
def _g7_model(g7, t, **kw):
    import torch
    from whisprrec_amd import host
    from whisprrec_amd.sgl import SGL
    nU, nI = int(g7["shape"][0]), int(g7["shape"][1])
    corpus = host.Corpus(nU, nI, {k: {"user_id": [], "item_id": []} for k in ("train", "dev", "test")}, ref.g7_clicked(g7), {})
    hp = g7[t + "_hp"]
    base = dict(device=_dev(), model_path="/tmp/wr_sgl_vn.pt", buffer=1, num_neg=1, test_all=1, embedding_size=int(g7["shape"][2]),
                gcn_layers=int(g7["shape"][3]), type=t.upper(), reg_weight=float(hp[0]), ssl_tau=float(hp[1]),
                ssl_weight=float(hp[2]), drop_ratio=float(hp[3]), views_native=1, random_seed=2024)
    base.update(kw)
    m = SGL(argparse.Namespace(**base), corpus).to(_dev())
    with torch.no_grad():
        m.user_embedding.weight.copy_(torch.from_numpy(g7[t + "_U0"]))
        m.item_embedding.weight.copy_(torch.from_numpy(g7[t + "_I0"]))
    return m


def _view_arrays(m, name):
    g = m._graph(name)
    return [t.cpu().numpy() for d in (g.fwd, g.bwd) for t in d] + [t.cpu().numpy() for t in g.row_ptr]


@pytest.mark.parametrize("t", ["ed", "nd"])
def test_model_views_follow_seed_and_version(g7, t):
    N, r, c = ref.g7_graph(g7)
    ratio = float(g7[t + "_hp"][3])
    m1, m2 = _g7_model(g7, t), _g7_model(g7, t)
    with pytest.raises(AttributeError):
        m1._graph("sub1")
    state = random.getstate()
    seen = []
    for version in (1, 2):
        m1.graph_construction(); m2.graph_construction()
        assert m1.graph_key() == version                          # the captured step graph is re-captured
        for view, name in enumerate(("sub1", "sub2")):
            a1, a2 = _view_arrays(m1, name), _view_arrays(m2, name)
            assert all(np.array_equal(x, y) for x, y in zip(a1, a2))          # same random_seed, same version: same arrays
            want = ref.expected(N, r, c, ref.keep_mask(t.upper(), r, c, N, ratio, 2024, version, view))
            g = m1._graph(name)
            for d, part in enumerate((g.fwd, g.bwd)):
                for got, key in zip(part, ("chunk_ptr", "chunk_row", "col", "val")):
                    assert np.array_equal(got.cpu().numpy(), want[d][key]), (name, d, key)
                assert part[1]._wr_levels == want[d]["levels"]
            seen.append(a1[2])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])      # sub1 != sub2, epoch 1 != epoch 2
    assert random.getstate() == state                             # the native path leaves Python's stream alone
    m3 = _g7_model(g7, t, random_seed=2025)
    m3.graph_construction()
    assert not np.array_equal(_view_arrays(m3, "sub1")[2], seen[0])


@pytest.mark.parametrize("t", ["ed", "nd"])
def test_three_training_steps_lower_the_loss(g7, t):
    import torch
    m = _g7_model(g7, t, optimizer="Adam", lr=5e-3, l2=0.0)
    batch = {k: torch.from_numpy(g7[s]).to(_dev()) for k, s in (("user_id", "u"), ("pos_item", "p"), ("neg_items", "n"))}
    m.graph_construction()
    m.train()
    losses = []
    for _ in range(3):
        m.optimizer.zero_grad(); loss = m.predict(batch); loss.backward(); m.optimizer.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[0] > losses[1] > losses[2], losses


def test_captured_step_graph_equals_eager_loop_with_native_views():
    """HipRunner's hipGraph of the SGL step over device-built views: re-captured after the second graph_construction(), its
    replays equal the eager loop bit for bit"""
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
        args = argparse.Namespace(device=dev, model_path="/tmp/wr_sgl_vn.pt", buffer=1, num_neg=1, test_all=1, embedding_size=64,
                                  gcn_layers=2, type="ED", reg_weight=1e-4, ssl_tau=0.2, ssl_weight=0.05, drop_ratio=0.1, ssl_native=1,
                                  views_native=1, random_seed=9, optimizer="Adam", lr=2e-3, l2=0.0, epoch=1, check_epoch=1,
                                  test_epoch=-1, early_stop=10, batch_size=B, eval_batch_size=256, num_workers=0, pin_memory=0,
                                  topk="10", metric="NDCG", device_epoch_prep=0, hip_graphs=graphs)
        m = SGL(args, corpus).to(dev)
        ds = SGL.Dataset(m, corpus, "train")
        r = runner.HipRunner(args)
        l1, l2 = r.fit(ds, epoch=1), r.fit(ds, epoch=2)
        assert m.graph_key() == 2 and m._graphs["sub1"] == "device"
        cache = getattr(r, "_graph_cache", None)
        assert (cache is not None) == bool(graphs)
        if graphs:
            assert cache[0][2] == 2                               # captured again for the second epoch's views
        out.append((l1, l2, m.user_embedding.weight.detach().clone(), m.item_embedding.weight.detach().clone(), m.optimizer.t))
    assert np.isfinite(out[0][0]) and out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert torch.equal(out[0][2], out[1][2]) and torch.equal(out[0][3], out[1][3])
    assert out[0][4] == out[1][4]
