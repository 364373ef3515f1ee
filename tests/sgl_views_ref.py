"""What the device view builder (--views_native 1, whisprrec_amd/csrc/wr_views.hip) must produce, from host code only: the
keep sets are restated with oracle.epoch_permutation_at and sgl.view_stream, then passed through the existing sgl.norm_csr,
sgl.transpose_csr and hip_ops.spmm_chunks.  Shared by test_sgl_views_native_contract.py (CPU) and test_hip_sgl_views.py (GPU)."""
import os

import numpy as np

import oracle
from whisprrec_amd import hip_ops, sgl


def ed_keep(n_edges, ratio, seed, version, view):
    """edge e survives iff perm(e) < int(E * (1 - ratio))"""
    n_keep = int(n_edges * (1 - ratio))
    perm = oracle.epoch_permutation_at(np.arange(n_edges, dtype=np.uint64), n_edges, seed, sgl.view_stream(version, view, 0))
    return perm < n_keep


def nd_drops(n_nodes, ratio, seed, version, view):
    """(row node dropped, column node dropped): node v iff perm_role(v) < int(N * ratio), two independent bijections"""
    n_drop = int(n_nodes * ratio)
    ids = np.arange(n_nodes, dtype=np.uint64)
    return tuple(oracle.epoch_permutation_at(ids, n_nodes, seed, sgl.view_stream(version, view, role)) < n_drop for role in (0, 1))


def keep_mask(kind, rows, cols, n_nodes, ratio, seed, version, view):
    if kind == "ED":
        return ed_keep(rows.size, ratio, seed, version, view)
    drop_r, drop_c = nd_drops(n_nodes, ratio, seed, version, view)
    return ~drop_r[rows] & ~drop_c[cols]


def n_select(kind, rows, n_nodes, ratio):
    return int(rows.size * (1 - ratio)) if kind == "ED" else int(n_nodes * ratio)


def stream_ids(kind, version, view):
    return (sgl.view_stream(version, view, 0),) if kind == "ED" else tuple(sgl.view_stream(version, view, r) for r in (0, 1))


def expected(n_nodes, rows, cols, mask):
    """[forward, transposed] of the view that keeps rows[mask], cols[mask]: dicts of row_ptr, col, val, chunk_ptr, chunk_row, levels"""
    rp, col, val = sgl.norm_csr(n_nodes, rows[mask], cols[mask])
    out = []
    for a, b, c in ((rp, col, val), sgl.transpose_csr(n_nodes, rp, col, val)):
        cptr, crow = hip_ops.spmm_chunks(a)
        out.append(dict(row_ptr=a, col=b, val=c, chunk_ptr=cptr.numpy(), chunk_row=crow.numpy(), levels=crow._wr_levels))
    return out


def edges_of(n_users, n_items, pairs):
    """base edge list of distinct (user, item) pairs"""
    sets = {}
    for u, i in pairs:
        sets.setdefault(int(u), set()).add(int(i))
    return sgl.adjacency_edges(n_users, n_items, sets)


# ------------------------------------------------------------------------------------------------ graphs
TOY = dict(n_users=3, n_items=4, pairs=[(0, 0), (0, 1), (1, 1), (1, 2), (2, 3)], ratio=0.5)     # N = 7, E = 10: no power of two
TOY_SEED = {"ED": 5, "ND": 1}       # seeds (version 1, view 0) whose restated keep sets have the properties toy_properties asks for


def toy():
    r, c = edges_of(TOY["n_users"], TOY["n_items"], TOY["pairs"])
    return TOY["n_users"] + TOY["n_items"], r, c


def view_properties(n_nodes, rows, cols, mask):
    """what a keep set exercises: rows the drop emptied, kept edges whose column node has no kept row edge (dis_tab[0])"""
    base_deg = np.bincount(rows, minlength=n_nodes)
    deg = np.bincount(rows[mask], minlength=n_nodes)
    return dict(emptied=int(((base_deg > 0) & (deg == 0)).sum()), col_without_rows=int((deg[cols[mask]] == 0).sum()), deg=deg)


HUB = dict(n_users=61, n_items=5400, hub_degree=5400, others_degree=107, ratio=0.1, graph_seed=0)
HUB_SEED = {"ED": 0, "ND": 0}       # seeds (version 1, view 0) whose restated views have rows of degree exactly 0, 96 and 97


def hub_graph():
    """user 0 is a hub over every item (5400 >= 5000 edges: more than 48 chunks of 96, base chunks that lie inside one row);
    60 users of 107 items each, so a 0.1 drop leaves degrees around 96"""
    rng = np.random.RandomState(HUB["graph_seed"])
    pairs = [(0, i) for i in range(HUB["hub_degree"])]
    for u in range(1, HUB["n_users"]):
        pairs += [(u, int(i)) for i in rng.choice(HUB["n_items"], HUB["others_degree"], replace=False)]
    r, c = edges_of(HUB["n_users"], HUB["n_items"], pairs)
    return HUB["n_users"] + HUB["n_items"], r, c


def g7():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g7_sgl.npz"))


def g7_clicked(g):
    ptr, idx = g["clicked_ptr"], g["clicked_idx"]
    return {u: set(int(x) for x in idx[ptr[u]:ptr[u + 1]]) for u in range(len(ptr) - 1) if ptr[u + 1] > ptr[u]}


def g7_graph(g):
    nU, nI = int(g["shape"][0]), int(g["shape"][1])
    r, c = sgl.adjacency_edges(nU, nI, g7_clicked(g))
    return nU + nI, r, c
