"""CPU checks for the top-K over several interests (K23, wr_topk_recommend_multi): the supported set, the workspace bound, the
C-ABI argument errors (all reported before a launch), the runner's flag and refusals, and the power of the float64 restatement
of tests/if4rec_topk_ref.py — nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import if4rec_ref as R  # noqa: E402
import if4rec_topk_ref as T  # noqa: E402
from whisprrec_amd import host  # noqa: E402


def _lib():
    from whisprrec_amd import abi
    assert os.path.exists(abi.LIB_PATH), "run __graft_entry__.build() first"    # a missing library is a failed build, not a skip
    return abi, abi.lib()


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_entries_are_bound_with_the_documented_argument_counts():
    from whisprrec_amd import abi
    raw = ctypes.CDLL(abi.LIB_PATH)
    for name, n in {"wr_topk_multi_supported": 3, "wr_topk_multi_workspace_bytes": 5, "wr_topk_recommend_multi": 18}.items():
        assert len(abi.SIGNATURES[name][1]) == n and hasattr(raw, name), name
    # KQ and out_interest in, query_row out
    assert len(abi.SIGNATURES["wr_topk_recommend_multi"][1]) == len(abi.SIGNATURES["wr_topk_recommend_rows"][1]) + 1


def test_supported_set_is_topk_supports_times_one_two_four():
    from whisprrec_amd import hip_ops
    _, L = _lib()
    for D in (0, 4, 6, 8, 16, 24, 32, 64, 128, 252, 256):
        for KQ in (0, 1, 2, 3, 4, 8):
            for k in (0, 1, 256, 257):
                want = hip_ops.topk_supports(D, k) and KQ in (1, 2, 4)
                assert L.wr_topk_multi_supported(D, KQ, k) == int(want), (D, KQ, k)
                assert hip_ops.topk_multi_supports(D, KQ, k) == bool(want)
    assert L.wr_topk_multi_supported(64, 2, 20) == 1 and L.wr_topk_multi_supported(24, 4, 256) == 1


def test_workspace_bound_never_decreases_and_is_the_single_query_bound_for_one_interest():
    abi, L = _lib()
    ns = (0, 1, 31, 32, 33, 64, 127, 128, 129, 1000, 6040, 100_000, 524_288, 524_289, 2_000_000)
    items = (0, 1, 4095, 4096, 8191, 8192, 8300, 100_000, 262_144, 1_000_000)
    ks = (1, 20, 128, 129, 256)
    for KQ in (1, 2, 4):
        grid = np.array([[[L.wr_topk_multi_workspace_bytes(n, m, 64, KQ, k) for k in ks] for m in items] for n in ns])
        assert (grid > 0).all()
        for axis in range(3):
            assert (np.diff(grid, axis=axis) >= 0).all(), (KQ, axis)
        if KQ == 1:
            single = np.array([[[L.wr_topk_workspace_bytes(n, m, 64, k) for k in ks] for m in items] for n in ns])
            assert np.array_equal(grid, single)
    # n rows of KQ interests never need more than n KQ single rows, and at least the regions of their own lists
    for KQ in (2, 4):
        for n in (129, 6040, 100_000):
            for k in (20, 256):
                got = L.wr_topk_multi_workspace_bytes(n, 8300, 64, KQ, k)
                assert got <= L.wr_topk_workspace_bytes(n * KQ, 8300, 64, k)
                assert got >= n * (256 if k <= 128 else 512) * 8                # one region per row at the least
    assert L.wr_topk_multi_workspace_bytes(10, 10, 64, 3, 5) == -2 and "KQ=3" in abi.last_error()
    assert L.wr_topk_multi_workspace_bytes(-1, 10, 64, 2, 5) == -2 and L.wr_topk_multi_workspace_bytes(10, 10, 64, 2, 257) == -2
    assert L.wr_topk_multi_workspace_bytes(1 << 31, 10, 64, 2, 5) == -2


def test_argument_errors_are_reported_before_any_launch():
    """no GPU here: every one of these returns before a launch"""
    abi, L = _lib()
    buf = (ctypes.c_float * 4096)()
    a16 = (ctypes.addressof(buf) + 15) // 16 * 16

    def multi(Q=a16, nq=8, I=a16, n_items=10, D=64, KQ=2, n=4, mrow=a16, n_mask=5, ptr=a16, idx=a16, k=5, oi=a16, osc=a16, oint=a16,
              ws=a16, ws_bytes=1 << 40):
        return L.wr_topk_recommend_multi(Q, nq, I, n_items, D, KQ, n, mrow, n_mask, ptr, idx, k, oi, osc, oint, ws, ws_bytes, None)

    assert multi(KQ=3) == -5 and "KQ=3" in abi.last_error()
    assert multi(KQ=8) == -5 and multi(KQ=0) == -5
    assert multi(Q=None) == -1 and "NULL" in abi.last_error()
    assert multi(I=None) == -1 and multi(oi=None) == -1 and multi(osc=None) == -1
    assert multi(mrow=None) == -1 and "go together" in abi.last_error()
    assert multi(ptr=None) == -1 and multi(idx=None) == -1
    assert multi(Q=a16 + 4) == -4 and multi(I=a16 + 4) == -4 and multi(ws=a16 + 8) == -4 and "aligned" in abi.last_error()
    assert multi(D=256) == -5 and "D=256" in abi.last_error()
    assert multi(k=0) == -5 and multi(k=257) == -5 and "k=257" in abi.last_error()
    assert multi(D=6) == -2 and multi(n=-1) == -2 and multi(n_mask=0) == -2
    assert multi(nq=7) == -2 and "query_mat has 7 rows" in abi.last_error()
    assert multi(n=1 << 30) == -2 and "n out of range" in abi.last_error()        # n KQ must stay below 2^31
    need = L.wr_topk_multi_workspace_bytes(4, 10, 64, 2, 5)
    assert multi(ws_bytes=need - 1) == -3 and "%d B needed" % need in abi.last_error()
    assert multi(ws=None) == -3
    assert multi(n=0) == 0 and multi(n=0, oint=None, mrow=None, ptr=None, idx=None) == 0


def test_wrapper_refuses_cpu_tensors_and_bad_shapes():
    from whisprrec_amd import abi, hip_ops
    item = torch.zeros(30, 64)
    with pytest.raises(abi.WhisprRecHipError, match="ROCm device"):
        hip_ops.topk_recommend_multi(torch.zeros(4, 2, 64), item, 5)
    with pytest.raises(TypeError):
        hip_ops.topk_recommend_multi(np.zeros((4, 2, 64), np.float32), item, 5)


# ------------------------------------------------------------------------------------------------ the runner
class _Interests:
    """a model with the interest protocol and nothing else"""
    history_max, test_all, user_num = 3, 1, 3

    def __init__(self, K):
        self.n_interests = K
        self._items = torch.zeros(40, 64)

    def eval_interests(self, history_items, lengths):
        return torch.zeros(history_items.shape[0], self.n_interests, 64)

    def eval_items(self):
        return self._items


class _Queries:
    """a model with one query per row"""
    history_max, test_all, user_num = 3, 1, 3

    def eval_queries(self, history_items, lengths):
        return torch.zeros(history_items.shape[0], 64)

    def eval_items(self):
        return torch.zeros(40, 64)


def _runner_and_dataset(model, flag="1"):
    from test_seq_eval_contract import _seq_corpus
    from whisprrec_amd import main as launcher, runner
    ds = host.SequentialModel.Dataset(model, _seq_corpus(), "dev")
    extra = ["--interest_topk_native", flag] if flag is not None else []
    args = launcher.build_args(["--model_name", "IF4Rec", "--runner_name", "HipRunner", "--seq_eval_native", "1"] + extra)[0]
    return runner.HipRunner(args), ds


def test_flag_parses_and_defaults_to_zero():
    from whisprrec_amd import main as launcher, runner
    base = ["--model_name", "IF4Rec", "--runner_name", "HipRunner"]
    args = launcher.build_args(base)[0]
    assert args.interest_topk_native == 0 and runner.HipRunner(args).interest_topk_native is False
    args = launcher.build_args(base + ["--interest_topk_native", "1"])[0]
    assert args.interest_topk_native == 1 and runner.HipRunner(args).interest_topk_native is True
    with pytest.raises(SystemExit):
        launcher.build_args(base + ["--interest_topk_native", "2"])


def test_flag_off_keeps_the_refusal_and_names_the_flag():
    rn, ds = _runner_and_dataset(_Interests(2), flag="0")
    for call in (lambda: rn.recommend_rows(ds, 5), lambda: rn.recommend_next(ds.model, ds.corpus, [[1, 2]], 5),
                 lambda: rn.save_rec_results(ds, 5, "/tmp/never.csv")):
        with pytest.raises(NotImplementedError, match="top-K over several interests.*--interest_topk_native 1"):
            call()


def test_three_interests_are_refused_by_name_and_number():
    rn, ds = _runner_and_dataset(_Interests(3))
    for call in (lambda: rn.recommend_rows(ds, 5), lambda: rn.recommend_next(ds.model, ds.corpus, [[1, 2]], 5),
                 lambda: rn.save_rec_results(ds, 5, "/tmp/never.csv")):
        with pytest.raises(NotImplementedError, match="_Interests.*3 interests of size 64 with k=5"):
            call()
    rn, ds = _runner_and_dataset(_Interests(2))
    with pytest.raises(NotImplementedError, match="2 interests of size 64 with k=300"):
        rn.recommend_rows(ds, 300)


def test_recommend_per_user_points_to_the_row_entries():
    rn, ds = _runner_and_dataset(_Interests(2))
    with pytest.raises(NotImplementedError, match="recommend_rows.*recommend_next"):
        rn.recommend(ds.model, ds.corpus, [0, 1], 5)


def test_with_interest_needs_a_multi_interest_model():
    for flag in ("0", "1"):
        rn, ds = _runner_and_dataset(_Queries(), flag=flag)
        with pytest.raises(ValueError, match="with_interest"):
            rn.recommend_rows(ds, 5, with_interest=True)
        with pytest.raises(ValueError, match="with_interest"):
            rn.recommend_next(ds.model, ds.corpus, [[1, 2]], 5, with_interest=True)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_a_tiny_example():
    c = dict(queries=np.array([[[1.0, 0.0], [0.0, 1.0]], [[1.0, 1.0], [1.0, 1.0]]], np.float32),
             items=np.array([[3, 0], [0, 2], [1, 1], [4, 4], [0, 3]], np.float32),
             mask_ptr=np.array([0, 1, 1]), mask_idx=np.array([3], np.int32), mask_row=np.array([0, 1]))
    items, sc, interest, _ = T.topk_ref(c, 6)
    # row 0: scores 3 (q0), 2 (q1), 1 (both: the first), masked, 3 (q1) -> 0 and 4 tie at 3: the smaller id first
    assert items[0].tolist() == [0, 4, 1, 2, -1, -1] and interest[0].tolist() == [0, 1, 1, 0, -1, -1]
    assert sc[0].tolist() == [3.0, 3.0, 2.0, 1.0, -np.inf, -np.inf]
    # row 1: the empty list; scores 3, 2, 2, 8, 3 and every interest ties
    assert items[1].tolist() == [3, 0, 4, 1, 2, -1] and interest[1].tolist() == [0, 0, 0, 0, 0, -1]


@pytest.mark.parametrize("KQ", [2, 4])
@pytest.mark.parametrize("wrong", T.WRONG_TOPK)
def test_wrong_variants_change_the_list_of_a_judged_row(wrong, KQ):
    c = R.make_rank_case(64, 2100, 257, KQ)
    items, _, _, judged = T.topk_ref(c, 10)
    assert judged.mean() >= 0.9
    bad = T.topk_ref(c, 10, variant=wrong)[0]
    changed = (bad[judged] != items[judged]).any(axis=1)
    assert changed.sum() >= 1, wrong
