"""CPU checks for --train_loss softmax (K26): the float64 restatement of tests/softmax_ref.py against torch's own float64
autograd of the stock lines, the tolerances against the fp32 floor, the power of the four figures against deliberately wrong
results, and the interface (header, binding, workspace bound, C-ABI argument errors, parser flags, the --emb_lazy refusal, the
untouched BPR path) — nothing here needs a GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softmax_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRY_POINTS = ("wr_softmax_ce_supported", "wr_softmax_ce_workspace_bytes", "wr_softmax_ce_loss_grad")


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("shape", [0, 3, 4])
def test_restatement_equals_float64_autograd_of_the_stock_lines(shape, variant):
    Q, E, t = R.make_case(*R.SHAPES[shape], 7 + shape, variant)
    if variant == "large":
        assert np.abs(Q.astype(np.float64) @ E[1:].astype(np.float64).T).max() > 150
    if variant == "dup" and len(t) >= 4:
        assert np.unique(t, return_counts=True)[1].max() >= len(t) // 4
    q = torch.tensor(Q, dtype=torch.float64, requires_grad=True)
    e = torch.tensor(E, dtype=torch.float64, requires_grad=True)
    loss = R.stock_lines(q, e, torch.from_numpy(t))
    gq, ge = torch.autograd.grad(loss, [q, e])
    ref = R.softmax_ce_f64(Q, E, t)
    assert abs(float(loss.detach()) - ref[0]) / abs(ref[0]) < 1e-12
    assert R.rel_err(ref[1], gq.numpy()) < 1e-12 and R.rel_err(ref[2], ge.numpy()) < 1e-12
    assert not ref[2][0].any()                                              # the padding row is no class


def test_an_unshifted_fp32_exp_overflows_on_the_large_variant():
    Q, E, t = R.make_case(*R.SHAPES[0], 100, "large")
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp((Q @ E[1:].T).astype(np.float32))).any()


@pytest.fixture(scope="module")
def floors():
    return R.measure_floors()


def test_tolerances_follow_the_floor_rule(floors):
    print("floors re-measured: " + " ".join("%s %.2e" % kv for kv in floors.items()))
    for k in R.FIGURES:
        assert 4 * floors[k] < R.TOL[k] <= 16 * R.FLOORS[k], (k, floors[k], R.TOL[k], R.FLOORS[k])
        want = 8 * R.FLOORS[k]
        digit = 10.0 ** np.floor(np.log10(want))
        assert np.isclose(R.TOL[k], np.ceil(want / digit - 1e-9) * digit), k      # 8 x floor, rounded up to one digit


WRONG = [("column 0 left in the softmax", "random", dict(keep_excluded=True), "gQ"),
         ("the target term dropped", "random", dict(target_term=False), "gE_in"),
         ("the last partial tile left out", "random", dict(drop_last=None), "gE_out"),
         ("gE_out 1 % too large", "random", dict(out_scale=1.01), "gE_out"),
         ("one occurrence of a repeated target missing", "dup", dict(miss_one_dup=True), "gE_in"),
         ("sum instead of mean", "random", dict(weight=1.0), "loss")]


@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("what,variant,switch,figure", WRONG, ids=[w[0].replace(" ", "_") for w in WRONG])
def test_wrong_results_miss_the_tolerance(shape, what, variant, switch, figure):
    n, B, D = R.SHAPES[shape]
    Q, E, t = R.make_case(n, B, D, 100 + 10 * shape, variant)
    switch = dict(switch)
    if "drop_last" in switch:
        switch["drop_last"] = n % 64
        assert switch["drop_last"] > 0
    ref = R.softmax_ce_f64(Q, E, t)
    fig = R.figures(R.softmax_ce_f64(Q, E, t, **switch), ref, t)
    print("%s at %s: " % (what, (n, B, D)) + " ".join("%s %.2e" % kv for kv in fig.items()))
    assert fig[figure] > R.TOL[figure], (what, figure, fig[figure])


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_header_declares_and_binding_binds_the_entry_points():
    from whisprrec_amd import abi
    src = open(os.path.join(ROOT, "include", "whisprrec_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int32_t|int64_t)\s+%s\s*\(" % name, src), name
        assert name in abi.SIGNATURES and hasattr(abi.lib(), name), name
    assert len(abi.SIGNATURES["wr_softmax_ce_loss_grad"][1]) == 16
    assert "wr_softmax.hip" in open(os.path.join(ROOT, "whisprrec_amd", "csrc", "Makefile")).read()


def test_workspace_is_monotone_and_far_below_a_score_matrix():
    from whisprrec_amd import abi
    L = abi.lib()
    for D in (32, 64, 128):
        prev = 0
        for n in (1, 70, 3706, 100_000, 1_000_000, 5_000_000):
            cur = L.wr_softmax_ce_workspace_bytes(n, 2048, D)
            assert cur >= prev > -1, (n, D)
            prev = cur
        prev = 0
        for B in (1, 127, 128, 129, 2048, 65536, 1_000_000):
            cur = L.wr_softmax_ce_workspace_bytes(100_000, B, D)
            assert cur >= prev > -1, (B, D)
            prev = cur
    n, B = 1_000_000, 2048
    assert L.wr_softmax_ce_workspace_bytes(n, B, 64) < B * n * 4 // 8


def test_c_abi_refuses_unsupported_shapes_with_the_numbers():
    from whisprrec_amd import abi
    L = abi.lib()
    assert [L.wr_softmax_ce_supported(D) for D in (32, 64, 128)] == [1, 1, 1]
    assert [L.wr_softmax_ce_supported(D) for D in (0, 16, 48, 96, 256)] == [0, 0, 0, 0, 0]
    assert L.wr_softmax_ce_workspace_bytes(1000, 8, 48) < 0
    assert "D=48" in abi.last_error() and "{32, 64, 128}" in abi.last_error()
    assert L.wr_softmax_ce_workspace_bytes(0, 8, 64) < 0 and "n_items=0" in abi.last_error()
    keep = ctypes.create_string_buffer(96)                                  # nothing is dereferenced: every call is refused
    addr = (ctypes.addressof(keep) + 15) // 16 * 16
    rc = L.wr_softmax_ce_loss_grad(addr, 8, addr, 1000, 48, addr, 1, 1.0, addr, 0, addr, addr, None, addr, 1 << 30, None)
    assert rc < 0 and "D=48" in abi.last_error()
    rc = L.wr_softmax_ce_loss_grad(addr, 8, addr, 1000, 64, addr, 1000, 1.0, addr, 0, addr, addr, None, addr, 1 << 30, None)
    assert rc < 0 and "first_class=1000" in abi.last_error()
    rc = L.wr_softmax_ce_loss_grad(None, 8, addr, 1000, 64, addr, 1, 1.0, addr, 0, addr, addr, None, addr, 1 << 30, None)
    assert rc == -1 and "NULL" in abi.last_error()
    rc = L.wr_softmax_ce_loss_grad(addr, 8, addr, 1000, 64, addr, 1, 1.0, addr, 0, addr, None, None, addr, 1 << 30, None)
    assert rc == -1 and "go together" in abi.last_error()
    rc = L.wr_softmax_ce_loss_grad(addr, 8, addr, 1000, 64, addr, 1, 1.0, addr, 0, addr, addr, None, addr, 64, None)
    assert rc < 0 and "workspace" in abi.last_error()


def test_wrappers_refuse_cpu_tensors():
    from whisprrec_amd import abi, hip_ops
    Q, E, t = torch.zeros(4, 64), torch.zeros(10, 64), torch.ones(4, dtype=torch.int64)
    with pytest.raises(abi.WhisprRecHipError, match="no CPU fallback"):
        hip_ops.softmax_ce_loss_grad(Q, E, t)
    with pytest.raises(abi.WhisprRecHipError, match="no CPU fallback"):
        hip_ops.softmax_ce_loss(Q.requires_grad_(True), E, t)
    assert hip_ops.softmax_ce_supports(64) and not hip_ops.softmax_ce_supports(48)
    assert hip_ops.softmax_ce_workspace_bytes(3706, 256, 64) > 0
    hip_ops.softmax_ce_release_workspaces()


# ------------------------------------------------------------------------------------------------ the models
def _argv(model, path, tmp, extra=()):
    return ["--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--dropout", "0.0", "--history_max", "20",
            "--model_name", model, "--runner_name", "HipRunner", "--dataset", "ml-100k", "--path", path, "--epoch", "1",
            "--batch_size", "1024", "--eval_batch_size", "512", "--optimizer", "Adam", "--lr", "1e-3", "--l2", "0.0",
            "--log_file", str(tmp / "log.txt"), "--model_path", str(tmp / "m.pt"), "--num_workers", "0", "--topk", "5,10",
            "--metric", "NDCG, HR", "--random_seed", "3407"] + list(extra)


@pytest.mark.parametrize("model", ["SASRec", "TiSASRec"])
def test_parser_takes_the_two_flags(model, tmp_path):
    from whisprrec_amd import main as launcher
    args, model_class, _, _ = launcher.build_args(_argv(model, "x/", tmp_path))
    assert (args.train_loss, args.softmax_native) == ("bpr", 0)
    assert model_class.extra_log_args[-2:] == ["train_loss", "softmax_native"]
    args = launcher.build_args(_argv(model, "x/", tmp_path, ["--train_loss", "softmax", "--softmax_native", "1"]))[0]
    assert (args.train_loss, args.softmax_native) == ("softmax", 1)
    with pytest.raises(SystemExit):
        launcher.build_args(_argv(model, "x/", tmp_path, ["--train_loss", "bce"]))


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from test_reader import _write_inter
    tmp = tmp_path_factory.mktemp("softmax_loss")
    return _write_inter(np.load(os.path.join(GOLD, "g8_reader.npz")), tmp), tmp


def _cpu_model(model, tiny, extra=()):
    from whisprrec_amd import main as launcher
    path, tmp = tiny
    args, model_class, reader_class, _ = launcher.build_args(_argv(model, path, tmp, extra))
    args.device = torch.device("cpu")
    corpus = reader_class(args).corpus()
    launcher.init_seed(args.random_seed)
    return model_class(args, corpus), corpus


@pytest.mark.parametrize("model", ["SASRec", "TiSASRec"])
def test_softmax_with_the_row_lazy_table_is_refused(model, tiny):
    with pytest.raises(ValueError, match="every item row gets a gradient every step"):
        _cpu_model(model, tiny, ["--train_loss", "softmax", "--emb_lazy", "1"])
    m, _ = _cpu_model(model, tiny, ["--train_loss", "softmax"])
    assert m.train_loss == "softmax" and m.softmax_native is False


def _cpu_batch(m, B=9, T=6, seed=5):
    rng = np.random.RandomState(seed)
    lengths = rng.randint(1, T + 1, B)
    lengths[0] = T
    valid = np.arange(T)[None, :] < lengths[:, None]
    t = torch.as_tensor
    return {"history_items": t(rng.randint(1, m.item_num, (B, T)) * valid), "lengths": t(lengths),
            "history_times": t((1000 + np.cumsum(rng.randint(0, 90, (B, T)), axis=1)) * valid),
            "user_id": t(rng.randint(1, m.user_num, B)), "pos_item": t(rng.randint(1, m.item_num, B)),
            "neg_items": t(rng.randint(1, m.item_num, (B, 1)))}


@pytest.mark.parametrize("model", ["SASRec", "TiSASRec"])
def test_bpr_predict_is_the_bpr_formula_bitwise_and_softmax_the_stock_lines(model, tiny, monkeypatch):
    """the item table's lookup is a HIP kernel, so on a CPU it is replaced by plain indexing; everything else runs as it is"""
    m, _ = _cpu_model(model, tiny)
    assert m.train_loss == "bpr"
    monkeypatch.setattr(m.item_embedding, "forward", lambda idx: m.item_embedding.weight[idx])
    m.eval()
    batch = _cpu_batch(m)
    with torch.no_grad():
        got = m.predict(batch)
        user_e, w = m.forward(batch), m.item_embedding.weight
        pos = (user_e * w[batch["pos_item"]]).sum(dim=1)
        neg = (user_e * w[batch["neg_items"].reshape(-1)]).sum(dim=1)
        want = -torch.log(1e-10 + torch.sigmoid(pos - neg)).mean()
        assert torch.equal(got, want)
        m.train_loss = "softmax"
        got = m.predict(dict(batch, neg_items=None))                        # neg_items is not read
        assert torch.equal(got, R.stock_lines(user_e, w, batch["pos_item"]))
    ref = R.softmax_ce_f64(user_e.numpy(), w.detach().numpy(), batch["pos_item"].numpy())[0]
    assert abs(float(got) - ref) / ref < 1e-5
