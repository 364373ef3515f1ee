"""CPU-only checks of the per-row evaluation boundary (K14): the --seq_eval_native flag, the two new C entries in the ctypes
table and their argument errors before any launch, the tensor wrappers' checks, and HipRunner's per-dataset history cache."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

from whisprrec_amd import abi, hip_ops, host, main as launcher, runner

N_Q, N_ITEMS, D, N, K = 8, 16, 64, 4, 10


def test_flag_defaults_to_off_and_parses_through_the_launcher():
    p = argparse.ArgumentParser()
    runner.HipRunner.parse_runner_args(p)
    assert p.parse_args([]).seq_eval_native == 0
    assert p.parse_args(["--seq_eval_native", "1"]).seq_eval_native == 1
    with pytest.raises(SystemExit):
        p.parse_args(["--seq_eval_native", "2"])
    base = ["--model_name", "SASRec", "--runner_name", "HipRunner"]
    assert launcher.build_args(base)[0].seq_eval_native == 0
    args, _, _, runner_class = launcher.build_args(base + ["--seq_eval_native", "1", "--block_native", "1"])
    assert args.seq_eval_native == 1 and args.block_native == 1 and runner_class is runner.HipRunner
    assert not hasattr(launcher.build_args(["--model_name", "SASRec"])[0], "seq_eval_native")   # BaseRunner has no such flag
    args.eval_batch_size, args.random_seed = 64, 1
    assert runner.HipRunner(args).seq_eval_native is True


def test_new_entries_are_bound_with_the_documented_argument_counts():
    res, args = abi.SIGNATURES["wr_rank_eval_rows"]
    assert res is ctypes.c_int32 and len(args) == 15
    res, args = abi.SIGNATURES["wr_topk_recommend_rows"]
    assert res is ctypes.c_int32 and len(args) == 17
    # the roles that wr_rank_eval folds into eval_user: query_row, mask_row, n_mask_rows
    assert len(abi.SIGNATURES["wr_rank_eval_rows"][1]) == len(abi.SIGNATURES["wr_rank_eval"][1]) + 2
    assert len(abi.SIGNATURES["wr_topk_recommend_rows"][1]) == len(abi.SIGNATURES["wr_topk_recommend"][1]) + 2
    assert hasattr(ctypes.CDLL(abi.LIB_PATH), "wr_rank_eval_rows") and hasattr(ctypes.CDLL(abi.LIB_PATH), "wr_topk_recommend_rows")


@pytest.fixture
def base():
    """a 16-byte aligned host buffer standing in for device pointers: every call below fails its argument check first"""
    raw = (ctypes.c_char * (1 << 16))()
    yield (ctypes.addressof(raw) + 15) // 16 * 16
    del raw


def _rank(base, **kw):
    a = dict(query_mat=base, n_query_rows=N_Q, item_tab=base + 4096, n_items=N_ITEMS, D=D, query_row=None, eval_target=base + 8192,
             n=N, mask_row=None, n_mask_rows=0, mask_ptr=None, mask_idx=None, rank=base + 12288, target_score=base + 16384)
    a.update(kw)
    return abi.lib().wr_rank_eval_rows(*a.values(), None)


def _topk(base, **kw):
    a = dict(query_mat=base, n_query_rows=N_Q, item_tab=base + 4096, n_items=N_ITEMS, D=D, query_row=None, n=N, mask_row=None,
             n_mask_rows=0, mask_ptr=None, mask_idx=None, k=K, out_item=base + 12288, out_score=base + 16384,
             workspace=base + 20480, workspace_bytes=None)
    a.update(kw)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = abi.lib().wr_topk_workspace_bytes(a["n"], a["n_items"], a["D"], a["k"])
    return abi.lib().wr_topk_recommend_rows(*a.values(), None)


@pytest.mark.parametrize("call", [_rank, _topk])
def test_entries_report_argument_errors_before_any_launch(base, call):
    assert call(base, query_mat=None) == -1 and "NULL" in abi.last_error()
    assert call(base, item_tab=None) == -1
    # the three mask arguments are all NULL or all non-NULL
    m = base + 24576
    for given in ({"mask_row": m}, {"mask_ptr": m}, {"mask_idx": m}, {"mask_ptr": m, "mask_idx": m}, {"mask_row": m, "mask_ptr": m},
                  {"mask_row": m, "mask_idx": m}):
        assert call(base, n_mask_rows=3, **given) == -1 and "go together" in abi.last_error(), given
    # no query_row: row e of query_mat is the query of row e, so there must be n of them
    assert call(base, n=N_Q + 1) == -2 and "query_row" in abi.last_error()
    # the set of D of wr_rank_eval / wr_topk_supported
    assert call(base, D=256) == -5 and "D=256" in abi.last_error()
    assert call(base, D=6) == -2 and "multiple of 4" in abi.last_error()
    assert call(base, n=-1) == -2


def test_entry_specific_argument_errors(base):
    assert _rank(base, eval_target=None) == -1 and _rank(base, rank=None) == -1 and _rank(base, target_score=None) == -1
    assert _topk(base, out_item=None) == -1 and _topk(base, out_score=None) == -1
    assert _topk(base, k=0, workspace_bytes=1 << 30) == -5 and _topk(base, k=257, workspace_bytes=1 << 30) == -5
    need = abi.lib().wr_topk_workspace_bytes(N, N_ITEMS, D, K)
    assert _topk(base, workspace_bytes=need - 1) == -3 and "workspace" in abi.last_error()
    assert _topk(base, workspace=None, workspace_bytes=need) == -3


def test_wrappers_refuse_cpu_tensors():
    Q, I = torch.zeros(4, 64), torch.zeros(8, 64)
    with pytest.raises(abi.WhisprRecHipError, match="ROCm device"):
        hip_ops.rank_eval_rows(Q, I, torch.arange(4))
    with pytest.raises(abi.WhisprRecHipError, match="ROCm device"):
        hip_ops.topk_recommend_rows(Q, I, 3)


def test_wrappers_refuse_a_mask_without_mask_row_and_the_reverse():
    Q, I = torch.zeros(4, 64), torch.zeros(8, 64)
    ptr, idx = torch.zeros(3, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    rows = torch.zeros(4, dtype=torch.int64)
    for kw in ({"mask_ptr": ptr, "mask_idx": idx}, {"mask_row": rows}, {"mask_row": rows, "mask_ptr": ptr}):
        with pytest.raises(ValueError, match="mask_row|go together"):
            hip_ops.rank_eval_rows(Q, I, torch.arange(4), **kw)
        with pytest.raises(ValueError, match="mask_row|go together"):
            hip_ops.topk_recommend_rows(Q, I, 3, **kw)


# ------------------------------------------------------------------------------------------------ history cache
class _Model:
    history_max = 3
    test_all = 1


def _seq_corpus():
    """3 users with histories of 5, 2 and 4 (item, time) pairs; train / dev rows name (user, position)"""
    his = {0: [(11, 0), (12, 1), (13, 2), (14, 3), (15, 4)], 1: [(21, 0), (22, 1)], 2: [(31, 0), (32, 1), (33, 2), (34, 3)]}
    frames = {"train": {"user_id": np.array([0, 0, 0, 1, 2, 2]), "item_id": np.array([12, 13, 14, 22, 32, 33]),
                        "position": np.array([1, 2, 3, 1, 1, 2])},
              "dev": {"user_id": np.array([0, 2]), "item_id": np.array([15, 34]), "position": np.array([4, 3])},
              "test": {"user_id": np.array([1]), "item_id": np.array([21]), "position": np.array([0])}}
    corpus = host.Corpus(3, 40, frames)
    corpus.user_his = his
    return corpus


def _expected(ds):
    rows = []
    for u, p in zip(ds.data["user_id"].tolist(), ds.data["position"].tolist()):
        rows.append([x[0] for x in ds.corpus.user_his[u][:p]][-_Model.history_max:])
    return rows


def test_history_cache_keeps_every_dataset_its_own_arrays():
    corpus = _seq_corpus()
    train = host.SequentialModel.Dataset(_Model(), corpus, "train")
    dev = host.SequentialModel.Dataset(_Model(), corpus, "dev")
    args = launcher.build_args(["--model_name", "SASRec", "--runner_name", "HipRunner"])[0]
    rn = runner.HipRunner(args)
    cpu = torch.device("cpu")
    first = {}
    for _ in range(3):                                    # train and dev alternate, as fit and evaluate do every epoch
        for name, ds in (("train", train), ("dev", dev)):
            hist, lens = rn._history_columns(ds, cpu)
            want = _expected(ds)
            assert lens.tolist() == [len(w) for w in want]
            assert hist.shape == (len(want), max(len(w) for w in want))
            for r, w in enumerate(want):
                assert hist[r].tolist() == w + [0] * (hist.shape[1] - len(w)), (name, r)
            if name in first:                             # the arrays built at the first visit, not rebuilt ones
                assert hist is first[name][0] and lens is first[name][1]
            first[name] = (hist, lens)
    assert first["train"][0] is not first["dev"][0]
    # a dataset object the cache has not seen is built, not served from a stale entry
    dev2 = host.SequentialModel.Dataset(_Model(), corpus, "dev")
    assert rn._history_columns(dev2, cpu)[0] is not first["dev"][0]
    assert torch.equal(rn._history_columns(dev2, cpu)[0], first["dev"][0])
