"""CPU-only checks of the top-K recommendation boundary (K11): argument errors of wr_topk_recommend before any launch, the
workspace bound, the tensor binding's device check, the rec-<model>.csv writer and the --save_rec flag."""
import argparse
import csv
import ctypes

import pytest
import torch

from whisprrec_amd import abi, hip_ops, main as launcher
from whisprrec_amd.runner import write_rec_csv

N_USERS, N_ITEMS, D, N, K = 8, 16, 64, 4, 10


@pytest.fixture
def bufs():
    """16-byte aligned host buffers standing in for device pointers: every call below fails its argument check first"""
    raw = (ctypes.c_char * (1 << 16))()
    base = (ctypes.addressof(raw) + 15) // 16 * 16
    return raw, base


def _call(base, **kw):
    args = dict(user_mat=base, n_user_rows=N_USERS, item_tab=base + 4096, n_items=N_ITEMS, D=D, query_user=base + 8192,
                n=N, mask_ptr=None, mask_idx=None, k=K, out_item=base + 12288, out_score=base + 16384, workspace=base + 20480,
                workspace_bytes=None)
    args.update(kw)
    if args["workspace_bytes"] is None:
        args["workspace_bytes"] = abi.lib().wr_topk_workspace_bytes(args["n"], args["n_items"], args["D"], args["k"])
    order = ["user_mat", "n_user_rows", "item_tab", "n_items", "D", "query_user", "n", "mask_ptr", "mask_idx", "k", "out_item",
             "out_score", "workspace", "workspace_bytes"]
    return abi.lib().wr_topk_recommend(*[args[o] for o in order], None)


def test_null_tables_and_outputs(bufs):
    _, base = bufs
    assert _call(base, user_mat=None) == -1 and "NULL" in abi.last_error()
    assert _call(base, item_tab=None) == -1
    assert _call(base, query_user=None) == -1
    assert _call(base, out_item=None) == -1
    assert _call(base, out_score=None) == -1


@pytest.mark.parametrize("k", [0, 257])
def test_k_out_of_range(bufs, k):
    _, base = bufs
    assert _call(base, k=k, workspace_bytes=1 << 30) == -5 and "k=" in abi.last_error()


def test_unsupported_embedding_sizes(bufs):
    _, base = bufs
    assert _call(base, D=256) == -5 and "D=256" in abi.last_error()       # LDS-operand staging does not fit
    assert _call(base, D=6) == -2 and "multiple of 4" in abi.last_error()
    assert not hip_ops.topk_supports(256, 10) and not hip_ops.topk_supports(6, 10)
    for d in (8, 16, 32, 64, 24, 128, 252):
        assert hip_ops.topk_supports(d, 1) and hip_ops.topk_supports(d, 256)
        assert hip_ops.topk_supports(d, 10) == hip_ops.rank_eval_supports(d)
    assert not hip_ops.topk_supports(64, 0) and not hip_ops.topk_supports(64, 257)


def test_mask_pointer_without_its_index_array(bufs):
    _, base = bufs
    assert _call(base, mask_ptr=base + 24576) == -1 and "mask" in abi.last_error()
    assert _call(base, mask_idx=base + 24576) == -1


def test_workspace_one_byte_too_small(bufs):
    _, base = bufs
    need = abi.lib().wr_topk_workspace_bytes(N, N_ITEMS, D, K)
    assert _call(base, workspace_bytes=need - 1) == -3 and "workspace" in abi.last_error()
    assert _call(base, workspace=None, workspace_bytes=need) == -3


def test_workspace_bound_is_positive_and_monotone():
    f = abi.lib().wr_topk_workspace_bytes
    assert f(1, 1, 64, 1) > 0
    ns = [1, 127, 128, 129, 1000, 6040, 20_000, 100_000, 1_000_000]
    items = [1, 40, 4096, 8192, 100_000, 1_000_000]
    ks = [1, 10, 100, 128, 129, 256]
    for k in ks:
        for ni in items:
            row = [f(n, ni, 64, k) for n in ns]
            assert all(a > 0 for a in row) and row == sorted(row), (k, ni, row)
        for n in ns:
            col = [f(n, ni, 64, k) for ni in items]
            assert col == sorted(col), (k, n, col)
    for n in ns:
        for ni in items:
            byk = [f(n, ni, 64, k) for k in ks]
            assert byk == sorted(byk)
    assert f(-1, 10, 64, 10) < 0 and f(10, 10, 64, 0) < 0


def test_binding_refuses_cpu_tensors():
    U, I = torch.zeros(4, 64), torch.zeros(8, 64)
    with pytest.raises(abi.WhisprRecHipError, match="ROCm device"):
        hip_ops.topk_recommend(U, I, torch.arange(4), 3)


@pytest.mark.parametrize("sep", ["\t", ","])
def test_rec_csv_format(tmp_path, sep):
    path = str(tmp_path / "rec.csv")
    users = [3, 0, 7]
    recs = [[5, 1, 9], [2, 3, -1], [10, 11, 12]]
    write_rec_csv(path, users, recs, sep)
    lines = open(path).read().split("\n")
    assert lines[0] == "user_id" + sep + "rec_items" and lines[-1] == "" and len(lines) == 5
    quote = '"' if sep == "," else ""
    assert lines[1] == "3" + sep + quote + "[5, 1, 9]" + quote
    with open(path, newline="") as f:
        rows = list(csv.reader(f, delimiter=sep))
    assert rows[0] == ["user_id", "rec_items"]
    assert [int(r[0]) for r in rows[1:]] == users
    assert [eval(r[1]) for r in rows[1:]] == recs


def test_save_rec_flag_parses_through_the_launcher():
    args = launcher.build_args(["--model_name", "BPRMF", "--runner_name", "HipRunner"])[0]
    assert args.save_rec == 0 and args.model_name == "BPRMF"
    args = launcher.build_args(["--model_name", "BPRMF", "--runner_name", "HipRunner", "--save_rec", "100"])[0]
    assert args.save_rec == 100
    args = launcher.build_args(["--model_name", "BPRMF"])[0]      # BaseRunner: the flag belongs to HipRunner
    assert not hasattr(args, "save_rec")
    assert isinstance(args, argparse.Namespace)
