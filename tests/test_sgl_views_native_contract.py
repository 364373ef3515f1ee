"""CPU contract of SGL's device view builder (--views_native): the flag, the ABI, the stream-id layout and — on the NumPy
restatement alone (tests/sgl_views_ref.py) — the distribution the keep rule draws from.  The kernels themselves are compared
with the restatement in tests/test_hip_sgl_views.py."""
import argparse
import os
import re

import numpy as np
import pytest

import sgl_views_ref as ref
from conftest import ROOT

NEW_SYMBOLS = ["wr_sgl_views_workspace_bytes", "wr_sgl_view_count", "wr_sgl_view_rows", "wr_sgl_view_fill",
               "wr_spmm_chunks_count", "wr_spmm_chunks_fill"]


def test_flag_parses_and_defaults_to_off():
    from whisprrec_amd.sgl import SGL
    p = argparse.ArgumentParser()
    SGL.parse_model_args(p)
    assert p.parse_args([]).views_native == 0
    assert p.parse_args(["--views_native", "1"]).views_native == 1
    with pytest.raises(SystemExit):
        p.parse_args(["--views_native", "2"])


def test_header_and_binding_list_the_new_entries():
    from whisprrec_amd import abi
    header = open(os.path.join(ROOT, "include", "whisprrec_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.SIGNATURES, name
    assert abi.lib().wr_abi_version() == 1                       # additive exports only


def test_argument_errors_come_before_any_launch():
    """no device here: every refusal below is decided on the host side of the entry"""
    from whisprrec_amd import abi
    L = abi.lib()
    assert L.wr_sgl_views_workspace_bytes(0, 10) == -2 and L.wr_sgl_views_workspace_bytes(10, 1 << 31) == -2
    assert L.wr_sgl_views_workspace_bytes(7, 10) >= 10 + 2 * 7
    buf = (np.zeros(64, np.int64).ctypes.data + 15) // 16 * 16
    assert L.wr_sgl_view_count(0, None, buf, buf, 10, 7, buf, 7, 5, 1, 4, 5, buf, buf, None, buf, 64, None) == -1
    assert L.wr_sgl_view_count(2, buf, buf, buf, 10, 7, buf, 7, 5, 1, 4, 5, buf, buf, None, buf, 64, None) == -5
    assert L.wr_sgl_view_count(0, buf, buf, buf, 10, 7, buf, 7, 11, 1, 4, 5, buf, buf, None, buf, 64, None) == -5   # n_keep > E
    assert L.wr_sgl_view_count(1, buf, buf, buf, 10, 7, buf, 7, 8, 1, 4, 5, buf, buf, None, buf, 64, None) == -5    # n_drop > N
    assert L.wr_sgl_view_count(0, buf, buf, buf, 10, 7, buf, 6, 5, 1, 4, 5, buf, buf, None, buf, 64, None) == -2    # a row without chunk
    assert L.wr_sgl_view_count(0, buf, buf, buf, 10, 7, buf, 7, 5, 1, 4, 5, buf, buf, None, buf, 16, None) == -3
    assert "workspace" in abi.last_error()
    assert L.wr_sgl_view_fill(buf, buf, buf, 10, 7, buf, 7, buf, buf, buf, buf, 4, None, None, 3, buf, buf, 3, None, buf, 64,
                              None) == -1                                                                       # col of nnz 3 NULL
    assert L.wr_sgl_view_fill(buf, buf, buf, 10, 7, buf, 7, buf, buf, buf, buf, 4, buf, buf, 11, buf, buf, 3, None, buf, 64,
                              None) == -2                                                                       # nnz > E
    assert L.wr_sgl_view_rows(buf, 7, 6, buf, buf, buf, buf, None) == -2
    assert L.wr_spmm_chunks_count(buf, 0, 96, buf, buf, None) == -2 and L.wr_spmm_chunks_count(buf, 7, 0, buf, buf, None) == -2
    assert L.wr_spmm_chunks_fill(buf, 7, 96, buf, 6, buf, buf, None) == -2 and L.wr_spmm_chunks_fill(buf, 7, 96, None, 7, buf, buf, None) == -1


def test_view_stream_is_injective():
    from whisprrec_amd.sgl import view_stream
    ids = {view_stream(v, k, r) for v in range(1001) for k in (0, 1) for r in (0, 1)}
    assert len(ids) == 1001 * 4 and min(ids) >= 0


def test_model_raises_before_the_first_construction_and_keeps_the_host_path_on_cpu():
    import random
    import torch
    from whisprrec_amd import host
    from whisprrec_amd.sgl import SGL
    g = ref.g7()
    nU, nI = int(g["shape"][0]), int(g["shape"][1])
    corpus = host.Corpus(nU, nI, {k: {"user_id": [], "item_id": []} for k in ("train", "dev", "test")}, ref.g7_clicked(g), {})
    args = argparse.Namespace(device=torch.device("cpu"), model_path="/tmp/wr_sgl_vn.pt", buffer=1, num_neg=1, test_all=1,
                              embedding_size=8, gcn_layers=2, type="ED", reg_weight=1e-4, ssl_tau=0.2, ssl_weight=0.05,
                              drop_ratio=0.1, views_native=1, random_seed=3)
    m = SGL(args, corpus)
    assert m.views_native and m.views_seed == 3
    with pytest.raises(AttributeError):
        m._graph("sub1")
    random.seed(7)
    m.graph_construction()                       # parameters on the CPU: the host views, from the `random` stream
    random.seed(7)
    r, c = m._edges
    from whisprrec_amd import sgl
    rp, col, val = sgl.norm_csr(nU + nI, *sgl.edge_dropout_edges(r, c, 0.1))
    assert np.array_equal(m._graphs["sub1"][0][1], col) and m.graph_key() == 1


# ------------------------------------------------------------------------------------------------ distribution (restatement)
E_DIST, RATE, STREAMS = 2000, 0.1, 64


@pytest.fixture(scope="module")
def ed_masks():
    return np.stack([_keep_at_stream(E_DIST, RATE, 2024, s) for s in range(STREAMS)])


def _keep_at_stream(n, rate, seed, stream):
    import oracle
    return oracle.epoch_permutation_at(np.arange(n, dtype=np.uint64), n, seed, stream) < int(n * (1 - rate))


def test_every_stream_keeps_exactly_n_keep_edges(ed_masks):
    from whisprrec_amd.sgl import view_stream
    assert view_stream(3, 1, 0) == 14                             # stream 14 is sub2's edge draw of the third construction
    assert np.array_equal(ed_masks[14], ref.ed_keep(E_DIST, RATE, 2024, 3, 1))
    assert (ed_masks.sum(axis=1) == int(E_DIST * (1 - RATE))).all() and int(E_DIST * (1 - RATE)) == 1800


def test_keep_frequency_is_uniform_over_edges(ed_masks):
    """every edge is kept with probability n_keep / E = 0.9 in a uniform subset of exact size: over 64 streams its count is
    Binomial(64, 0.9) up to the (negligible) dependence between streams — within 5 standard deviations for all 2000 edges"""
    p = 0.9
    sd = np.sqrt(p * (1 - p) / STREAMS)
    freq = ed_masks.mean(axis=0)
    assert np.abs(freq - p).max() <= 5 * sd, (freq.min(), freq.max(), 5 * sd)
    assert abs(freq.mean() - p) < 1e-12


def test_streams_differ(ed_masks):
    assert len({m.tobytes() for m in ed_masks}) == STREAMS


def test_node_drop_sets_have_exact_size_and_are_independent():
    N = 777
    for version in (1, 2, 3):
        for view in (0, 1):
            dr, dc = ref.nd_drops(N, RATE, 2024, version, view)
            assert dr.sum() == dc.sum() == int(N * RATE) == 77
            assert not np.array_equal(dr, dc)


# ------------------------------------------------------------------------------------------------ the graphs of the GPU tests
def test_base_edge_lists_hold_distinct_pairs():
    for N, r, c in (ref.toy(), ref.hub_graph(), ref.g7_graph(ref.g7())):
        keys = r * N + c
        assert np.all(keys[1:] > keys[:-1])                     # sorted by (row, col), no multiplicities
        assert np.array_equal(np.sort(c * N + r), keys)         # symmetric


def test_toy_graph_exercises_what_it_is_for():
    N, r, c = ref.toy()
    assert (N, r.size) == (7, 10) and N & (N - 1) and r.size & (r.size - 1)          # cycle walking runs for both
    for kind in ("ED", "ND"):
        m = ref.keep_mask(kind, r, c, N, ref.TOY["ratio"], ref.TOY_SEED[kind], 1, 0)
        p = ref.view_properties(N, r, c, m)
        assert p["emptied"] > 0 and p["col_without_rows"] > 0 and m.sum() >= 3, (kind, p)
        ex = ref.expected(N, r, c, m)
        assert (ex[0]["val"] > 1e4).any()                        # dis_tab[0] ~ 1e5 on a kept edge


def test_hub_graph_exercises_the_chunk_boundaries():
    N, r, c = ref.hub_graph()
    assert np.bincount(r).max() >= 5000
    for kind in ("ED", "ND"):
        m = ref.keep_mask(kind, r, c, N, ref.HUB["ratio"], ref.HUB_SEED[kind], 1, 0)
        ex = ref.expected(N, r, c, m)
        deg = set(np.diff(ex[0]["row_ptr"]).tolist())
        assert {0, 96, 97} <= deg, kind
        assert ex[0]["levels"] == 2 and ex[1]["levels"] == 2


def test_degree_table_carries_norm_csr_bits():
    """the device multiplies two entries of degree_scale(arange): the same expression, element by element, as norm_csr's"""
    from whisprrec_amd import sgl
    N, r, c = ref.hub_graph()
    rp, col, val = sgl.norm_csr(N, r, c)
    tab = sgl.degree_scale(np.arange(np.bincount(r).max() + 1))
    cnt = np.bincount(r, minlength=N)
    assert np.array_equal(val, tab[cnt[r]] * tab[cnt[c]])
    assert tab[0] == np.power(np.float32(0) + np.float32(1e-10), np.float32(-0.5))
