"""CPU checks for TiSASRec: the float64 restatements of tests/tisas_ref.py against the numbers recorded from the reference's own
TimeIntervalTransformerLayer (tests/golden/g15_tisasrec.npz), the torch-path block against the same numbers, the tolerances
against the fp32 floor, the interval and min_interval rules, the runner's time columns and the interface (launcher, C-ABI
argument errors) — nothing here needs a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tisas_ref as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# float64 against the reference's fp32 run of one block at B = 12, T = 20, D = 64 (g15), the figure of every array being
# max |a - b| / max |b|.  Measured: output 2.1e-7, gradients at most 2.7e-6 (time_k_tab, whose rows are sums of cancelling
# terms); pinned at 4 x that, rounded up to one digit.
G15_TOL_OUT, G15_TOL_GRAD = 9e-7, 2e-5
# the torch-path block runs the reference's ops in the reference's order: the same output bit for bit; the gradients agree up to
# the thread order of torch's CPU scatter-adds, which is fp32 noise of the size above (measured 3.4e-6, time_k_tab).
G15_TOL_SAME_OUT, G15_TOL_SAME_GRAD = 1e-7, 2e-5


@pytest.fixture(scope="module")
def g15():
    return np.load(os.path.join(GOLD, "g15_tisasrec.npz"))


def _f32(a):
    return np.asarray(a).astype(np.float32)


def _g15_inputs(g):
    hist, position, interval = (np.asarray(g[n], np.int64) for n in ("hist", "position", "interval"))
    sd = {n: _f32(g["sd__" + n]) for n in R.PARAMS}
    tabs = {n: _f32(g[n]) for n in ("item_tab", "pos_k_tab", "pos_v_tab", "time_k_tab", "time_v_tab")}
    return hist, position, interval, sd, tabs


KB, KW = "masked_attn_head.k_linear.bias", "masked_attn_head.k_linear.weight"


def _param_fig(name, got, ref_of):
    """the k_linear.bias gradient is mathematically zero (q . b_k is constant along a softmax row): it is measured absolutely,
    against max |g(k_linear.weight)|, as tests/sasblock_ref.py measures it"""
    if name == KB:
        return float(np.max(np.abs(np.asarray(got, np.float64) - ref_of(KB)))) / float(np.max(np.abs(ref_of(KW))))
    return R.rel_err(got, ref_of(name))


def _scatter(idx, grad, rows):
    out = np.zeros((rows, grad.shape[-1]), np.float64)
    np.add.at(out, idx.reshape(-1), grad.reshape(-1, grad.shape[-1]))
    return out


# ------------------------------------------------------------------------------------------------ g15
def test_g15_is_small_and_holds_the_rows_the_issue_names(g15):
    assert os.path.getsize(os.path.join(GOLD, "g15_tisasrec.npz")) <= os.path.getsize(os.path.join(GOLD, "g14_if4rec.npz"))
    assert g15["out"].shape == (12, 20, 64) and int(g15["heads"]) == 4 and int(g15["time_max"]) == 32
    assert list(g15["names"]) == R.PARAMS
    R_ = R.intervals(g15["times"], g15["min_interval"], 32)
    assert np.array_equal(R_, g15["interval"])                              # the integer rule is the recorded matrix
    n = g15["lengths"].astype(int)
    assert n.min() == 1 and n.max() == 20
    assert (R_[0][:n[0], :n[0]] == 0).all()                                 # equal timestamps
    off = ~np.eye(n[2], dtype=bool)
    assert (R_[2][:n[2], :n[2]][off] == 32).all()                           # every gap clamps
    assert 0 < (R_[4] < 32).mean() < 1


def test_restatement_reproduces_the_reference_layer(g15):
    hist, position, interval, sd, tabs = _g15_inputs(g15)
    ref = R.block_f64(tabs["item_tab"][hist], tabs["pos_k_tab"][position], tabs["pos_v_tab"][position], interval,
                      tabs["time_k_tab"], tabs["time_v_tab"], sd, 4, gout=_f32(g15["gout"]))
    fig = {"out": R.rel_err(g15["out"], ref["out"])}
    for n in R.PARAMS:
        fig[n] = _param_fig(n, g15["g__" + n], lambda m: ref["g"][m])
    fig["item_tab"] = R.rel_err(g15["g__item_tab"], _scatter(hist, ref["gx"], 30))
    fig["pos_k_tab"] = R.rel_err(g15["g__pos_k_tab"], _scatter(position, ref["gpos_k"], 21))
    fig["pos_v_tab"] = R.rel_err(g15["g__pos_v_tab"], _scatter(position, ref["gpos_v"], 21))
    fig["time_k_tab"] = R.rel_err(g15["g__time_k_tab"], ref["gtk"])
    fig["time_v_tab"] = R.rel_err(g15["g__time_v_tab"], ref["gtv"])
    worst = max((v, n) for n, v in fig.items() if n != "out")
    print(" ".join("%s %.1e" % (n.replace("masked_attn_head.", ""), v) for n, v in fig.items()))
    print("g15 restatement: out %.2e, worst gradient %.2e (%s)" % (fig["out"], worst[0], worst[1]))
    assert fig["out"] < G15_TOL_OUT, fig["out"]
    for n, v in fig.items():
        assert v < G15_TOL_GRAD, (n, v)


def test_torch_path_block_gives_the_reference_numbers(g15):
    from whisprrec_amd.tisasrec import _TiBlock
    hist, position, interval, sd, tabs = _g15_inputs(g15)
    blk = _TiBlock(64, 64, 4, 0.0)
    assert list(blk.state_dict().keys()) == R.PARAMS
    blk.load_state_dict({n: torch.from_numpy(sd[n]) for n in R.PARAMS})
    blk.train()
    leaves = {n: torch.from_numpy(v).clone().requires_grad_(True) for n, v in tabs.items()}
    it = torch.from_numpy(interval)
    out = blk(leaves["item_tab"][torch.from_numpy(hist)], leaves["pos_k_tab"][torch.from_numpy(position)],
              leaves["pos_v_tab"][torch.from_numpy(position)], leaves["time_k_tab"][it], leaves["time_v_tab"][it],
              torch.tril(torch.ones(1, 1, 20, 20, dtype=torch.int32)))
    (out * torch.from_numpy(_f32(g15["gout"]))).sum().backward()
    fig = {"out": R.rel_err(out.detach().numpy(), g15["out"])}
    for n, p in blk.named_parameters():
        fig[n] = _param_fig(n, p.grad.numpy(), lambda m: np.asarray(g15["g__" + m], np.float64))
    for n in tabs:
        fig[n] = R.rel_err(leaves[n].grad.numpy(), g15["g__" + n])
    print("g15 torch path: out %.2e, worst gradient %.2e" % (fig["out"], max(v for n, v in fig.items() if n != "out")))
    assert fig["out"] < G15_TOL_SAME_OUT, fig["out"]
    for n, v in fig.items():
        assert v < G15_TOL_SAME_GRAD, (n, v)


def test_wrong_variants_miss_the_tolerances():
    c = R.make_case(1, "spread")
    ref = R.case_f64(c)
    for wrong in ("no_time_k", "no_time_v", "mask_shift", "no_scale"):
        w = R.worst(R.figures(R.case_f64(c, wrong=wrong), ref))
        assert any(w[g] > R.TOL[g] for g in R.GROUPS), wrong


# ------------------------------------------------------------------------------------------------ floors
def test_tolerances_are_eight_floors():
    for g in R.GROUPS:
        assert 8 * R.FLOORS[g] <= R.TOL[g] < 20 * R.FLOORS[g], g


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=["x".join(map(str, s)) for s in R.SHAPES])
def test_floors_hold(shape, pattern):
    floors, _ = R.measure_floors([shape], [pattern])
    print("floor %s %s: " % (R.SHAPES[shape], pattern) + " ".join("%s %.2e" % (g, floors[g]) for g in R.GROUPS))
    for g in R.GROUPS:
        assert 4 * floors[g] < R.TOL[g], (g, floors[g])


# ------------------------------------------------------------------------------------------------ several visits per workgroup
_WALK = {}


def _walk(i, pattern):
    if (i, pattern) not in _WALK:
        c = R.make_case(i, pattern, R.WALK_SHAPES, R.WALK_SEED)
        _WALK[(i, pattern)] = (c, R.case_f64(c))
    return _WALK[(i, pattern)]


def _kernel_constant(name):
    import re
    import whisprrec_amd
    with open(os.path.join(os.path.dirname(os.path.abspath(whisprrec_amd.__file__)), "csrc", "wr_tiattn.hip")) as fh:
        return int(re.search(r"constexpr int %s = (\d+);" % name, fh.read()).group(1))


def test_walk_shapes_walk_and_leave_the_old_cases_alone():
    assert R.FWD_WG == _kernel_constant("kTiFwdWg") and R.BWD_WG == _kernel_constant("kTiBwdWg")
    assert all(B > R.BWD_WG and B % R.BWD_WG not in (0, R.BWD_WG - 1) for B, *_ in R.WALK_SHAPES)          # a ragged last visit
    assert any(B > 2 * R.BWD_WG for B, *_ in R.WALK_SHAPES) and any(B > R.FWD_WG for B, *_ in R.WALK_SHAPES)
    assert all(B <= 130 for B, *_ in R.SHAPES)
    c = R.make_case(1, "spread")                                            # the draws of an old case, as before
    rng = np.random.RandomState(9010)
    assert np.array_equal(c["q"], (rng.standard_normal((5, 7, 32)) * 0.7).astype(np.float32))
    assert not np.array_equal(R.make_case(0, "spread", R.WALK_SHAPES, R.WALK_SEED)["tk"][:, :4], R.make_case(1, "spread")["tk"][:, :4])


def test_walk_tolerances_are_eight_floors():
    from sasblock_ref import rule_of
    for g in R.GROUPS:
        assert 8 * R.WALK_FLOORS[g] <= R.WALK_TOL[g] <= 16 * R.WALK_FLOORS[g] and R.WALK_TOL[g] == rule_of(R.WALK_FLOORS[g]), g


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("shape", range(len(R.WALK_SHAPES)), ids=["x".join(map(str, s)) for s in R.WALK_SHAPES])
def test_walk_floors_hold(shape, pattern):
    c, ref = _walk(shape, pattern)
    floors = R.worst(R.figures(R.stock_fp32(c), ref))
    print("walk floor %s %s: " % (R.WALK_SHAPES[shape], pattern) + " ".join("%s %.2e" % (g, floors[g]) for g in R.GROUPS))
    for g in R.GROUPS:
        assert 4 * floors[g] < R.WALK_TOL[g], (g, floors[g])


@pytest.mark.parametrize("wrong", ["later_visits_dropped", "later_visits_stale"])
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("shape", range(len(R.WALK_SHAPES)), ids=["x".join(map(str, s)) for s in R.WALK_SHAPES])
def test_walk_mutants_land_five_tolerances_out(shape, pattern, wrong):
    """the table gradients of the first visits only; a later visit's out, gq, gk, gv those of the visit before"""
    c, ref = _walk(shape, pattern)
    fig = R.figures(R.walk_wrong(c, ref, wrong, R.BWD_WG), ref)
    margin = {n: v / R.WALK_TOL[R.GROUP_OF[n]] for n, v in fig.items()}
    print("walk mutant %s at %s %s: largest figure / tolerance %.1f (%s)" % (wrong, R.WALK_SHAPES[shape], pattern, max(margin.values()),
                                                                              max(margin, key=margin.get)))
    assert max(margin.values()) >= 5.0, margin


# ------------------------------------------------------------------------------------------------ the two rules
def test_interval_rule():
    from whisprrec_amd.tisasrec import interval_matrix
    tm = 512
    # equal timestamps: 0 everywhere; gaps that clamp; a quotient just below an integer where fp32 division rounds up
    gap, m = 300 * 65535 - 1, 65535
    assert int(np.floor(np.float32(gap) / np.float32(m))) == 300 and gap // m == 299
    times = np.asarray([[5, 5, 5], [0, 513 * 7, 512 * 7 - 1], [1000, 1000 + gap, 1000 + gap]], np.int64)
    scale = np.asarray([3, 7, m], np.int64)
    got = interval_matrix(torch.from_numpy(times), torch.from_numpy(scale), tm).numpy()
    assert got.dtype == np.int64 and np.array_equal(got, R.intervals(times, scale, tm))
    assert (got[0] == 0).all()
    assert got[1, 0, 1] == 512 and got[1, 1, 0] == 512 and got[1, 0, 2] == 511 and got[1, 1, 2] == 1
    assert got[2, 0, 1] == 299 and got[2, 1, 0] == 299 and got[2, 1, 2] == 0
    assert np.array_equal(got, got.transpose(0, 2, 1))


def test_min_interval_rule():
    from whisprrec_amd.tisasrec import user_min_intervals
    his = {1: [(3, 100)],                                       # one interaction
           2: [(3, 50), (4, 50), (5, 50)],                      # repeated timestamps only
           3: [(3, 10), (4, 10), (5, 17), (6, 40)],             # 7, not the 0 between the first two
           4: [(3, 0), (4, 1_000_000)],                         # capped
           6: [(1, 9), (2, 4), (3, 6)]}                         # unsorted input
    got = user_min_intervals(his, 8)
    assert got.dtype == np.int64 and got.tolist() == [65535, 65535, 65535, 7, 65535, 65535, 2, 65535]
    assert np.array_equal(got, R.min_intervals(his, 8))


# ------------------------------------------------------------------------------------------------ runner and interface
def _argv(path, tmp, extra=()):
    return ["--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--dropout", "0.0", "--history_max", "20",
            "--model_name", "TiSASRec", "--runner_name", "HipRunner", "--dataset", "ml-100k", "--path", path, "--epoch", "1",
            "--batch_size", "1024", "--eval_batch_size", "512", "--optimizer", "Adam", "--lr", "1e-3", "--l2", "0.0",
            "--log_file", str(tmp / "log.txt"), "--model_path", str(tmp / "m.pt"), "--num_workers", "0", "--topk", "5,10",
            "--metric", "NDCG, HR", "--random_seed", "3407"] + list(extra)


def test_parser_flags_exist(tmp_path):
    from whisprrec_amd import main as launcher, tisasrec
    args, model_class, reader_class, runner_class = launcher.build_args(_argv("x/", tmp_path))
    assert model_class is tisasrec.TiSASRec and reader_class.__name__ == "SeqReader"
    assert (args.time_max, args.ti_native, args.emb_lazy, args.history_max) == (512, 0, 0, 20)
    args2 = launcher.build_args(_argv("x/", tmp_path, ["--ti_native", "1", "--time_max", "64", "--emb_lazy", "1"]))[0]
    assert (args2.time_max, args2.ti_native, args2.emb_lazy) == (64, 1, 1)
    assert model_class.needs_history_times is True
    assert "time_max" in model_class.extra_log_args


def test_runner_time_columns_equal_the_per_sample_collate(tmp_path):
    from test_reader import _write_inter
    from whisprrec_amd import main as launcher
    g8 = np.load(os.path.join(GOLD, "g8_reader.npz"))
    path = _write_inter(g8, tmp_path)
    args, model_class, reader_class, runner_class = launcher.build_args(_argv(path, tmp_path))
    args.device = torch.device("cpu")
    corpus = reader_class(args).corpus()
    model = model_class(args, corpus)
    assert model.min_interval.dtype == torch.int64 and model.min_interval.shape == (model.user_num,)
    assert np.array_equal(model.min_interval.numpy(), R.min_intervals(corpus.user_his, model.user_num))
    assert "min_interval" in model.state_dict()
    run = runner_class(args)
    for phase in ("dev", "test"):
        ds = model_class.Dataset(model, corpus, phase)
        hist, lens = run._history_columns(ds, torch.device("cpu"))
        times = run._history_time_columns(ds, torch.device("cpu"))
        assert times.dtype == torch.int64 and times.shape == hist.shape
        assert run._history_time_columns(ds, torch.device("cpu")) is times           # built once per dataset
        rows = list(range(0, len(ds), max(len(ds) // 150, 1)))
        batch = ds.collate_batch([ds[i] for i in rows])
        w = batch["history_items"].shape[1]
        assert torch.equal(hist[rows][:, :w], batch["history_items"]) and not hist[rows][:, w:].any()
        assert torch.equal(times[rows][:, :w], batch["history_times"]) and not times[rows][:, w:].any()
        assert torch.equal(lens[rows], batch["lengths"])
        pad = torch.arange(hist.shape[1])[None, :] >= lens[:, None]
        assert not times[pad].any() and not hist[pad].any()                          # zero-padded past every row's length


def test_recommend_next_requires_times_and_users():
    from whisprrec_amd import runner

    class _Model:
        needs_history_times = True
        history_max, item_num, user_num = 5, 10, 3

        def eval_queries(self, *a, **k):
            raise AssertionError("not reached")

        def eval_items(self):
            return torch.zeros(10, 32)

    run = runner.HipRunner.__new__(runner.HipRunner)
    run.interest_topk_native = False
    for kw in ({}, {"users": [1]}, {"times": [[5, 6]]}):
        with pytest.raises(ValueError, match="times="):
            runner.HipRunner.recommend_next(run, _Model(), None, [[1, 2]], 3, **kw)


def test_c_abi_refuses_unsupported_shapes_with_the_numbers():
    from whisprrec_amd import abi
    L = abi.lib()
    assert L.wr_ti_attention_supported(64, 4, 20, 512) == 1 and L.wr_ti_attention_supported(32, 4, 64, 2048) == 1
    for D, H, T, tm in ((128, 4, 20, 512), (64, 8, 20, 512), (32, 8, 20, 512), (64, 4, 65, 512), (64, 4, 0, 512), (64, 4, 20, 2049),
                        (64, 3, 20, 512), (64, 4, 20, 0)):
        assert L.wr_ti_attention_supported(D, H, T, tm) == 0, (D, H, T, tm)
    assert L.wr_ti_attention_workspace_bytes(8, 65, 64, 4, 4096) == -5
    msg = abi.last_error()
    assert "T=65" in msg and "time_max=4096" in msg and "2048" in msg
    # the bound is independent of B and T: no B T T element anywhere
    a = L.wr_ti_attention_workspace_bytes(1, 1, 64, 4, 512)
    assert a == L.wr_ti_attention_workspace_bytes(1 << 20, 64, 64, 1, 512) == 256 * 2 * 513 * 64 * 4
    import ctypes
    keep = ctypes.create_string_buffer(96)                                  # nothing is dereferenced: both calls are refused
    addr = (ctypes.addressof(keep) + 15) // 16 * 16
    rc = L.wr_ti_attention_fwd(addr, addr, addr, addr, addr, 1, 20, 128, 4, addr, addr, 512, addr, None, None)
    assert rc == -5 and "D=128" in abi.last_error()
    rc = L.wr_ti_attention_fwd(None, addr, addr, addr, addr, 1, 20, 64, 4, addr, addr, 512, addr, None, None)
    assert rc == -1 and "NULL" in abi.last_error()
