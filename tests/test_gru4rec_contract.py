"""CPU checks for GRU4Rec (K27): the float64 restatement of tests/gru_ref.py against nn.GRU's own float64 autograd, the padded +
select form against the sort / pack / unsort form, the tolerances against the fp32 floor, the power of the four figures against
deliberately wrong results, and the interface (parser flags, MODELS, parameter names, the --emb_lazy refusal under softmax, C-ABI
argument errors) — nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_ref as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDS = ["x".join(map(str, s)) for s in R.SHAPES]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=IDS)
def test_restatement_equals_nn_gru_in_float64(shape, pattern):
    c = R.make_case(shape, pattern)
    fig = R.figures(R.stock(c, torch.float64), R.case_f64(c))
    for n, v in fig.items():                                   # the forward and all five gradients
        assert v < 1e-12, (n, v)


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=IDS)
def test_padded_select_equals_sort_pack_unsort_in_float64(shape, pattern):
    """what --gru_native 0 runs against ReChorus's form: a GRU is causal and the rows are left-aligned"""
    c = R.make_case(shape, pattern)
    padded, packed = R.stock(c, torch.float64), R.stock(c, torch.float64, packed=True)
    for n in R.GROUP_OF:
        assert R.rel_err(padded[n], packed[n]) < 1e-12, n
    T = c["x"].shape[1]
    assert not padded["gx"][np.arange(T)[None, :] >= c["lengths"][:, None]].any()


def test_restatement_ignores_the_padding_and_clamps_the_lengths():
    c = R.make_case(2, "mixed")
    ref = R.case_f64(c)
    d = dict(c)
    d["x"] = c["x"].copy()
    d["x"][np.arange(d["x"].shape[1])[None, :] >= c["lengths"][:, None]] = np.nan
    got = R.case_f64(d)
    for n in R.GROUP_OF:
        assert np.array_equal(got[n], ref[n]), n
    d = dict(c)
    d["lengths"] = c["lengths"].copy()
    d["lengths"][1], d["lengths"][2] = 10_000, 0                    # above T acts as T (row 1 is T already); 0: no step
    got = R.case_f64(d)
    assert np.array_equal(got["h"][1], ref["h"][1]) and not got["h"][2].any() and not got["gx"][2].any()


def test_wrong_variants_miss_the_tolerances():
    c = R.make_case(2, "mixed")                                      # B = 17: one full tile of 16 rows and one row more
    ref = R.case_f64(c)
    assert float(np.abs(c["bhh"][2 * 32:]).max()) > 0.1               # b_hn is not zero: its place is visible
    for wrong in R.WRONGS:
        w = R.worst(R.figures(R.case_f64(c, wrong=wrong), ref))
        assert any(w[g] > R.TOL[g] for g in R.GROUPS), (wrong, w)


# ------------------------------------------------------------------------------------------------ floors
def test_tolerances_are_eight_floors():
    for g in R.GROUPS:
        assert 8 * R.FLOORS[g] <= R.TOL[g] < 20 * R.FLOORS[g], g


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("shape", range(len(R.SHAPES)), ids=IDS)
def test_floors_hold(shape, pattern):
    floors, _ = R.measure_floors([shape], [pattern])
    print("floor %s %s: " % (R.SHAPES[shape], pattern) + " ".join("%s %.2e" % (g, floors[g]) for g in R.GROUPS))
    for g in R.GROUPS:
        assert 4 * floors[g] < R.TOL[g], (g, floors[g])


# ------------------------------------------------------------------------------------------------ several tiles per workgroup
WALK = [(i, pat) for i in range(len(R.WALK_SHAPES)) for pat in R.walk_patterns(i)]
WALK_IDS = ["%s-%s" % ("x".join(map(str, R.WALK_SHAPES[i])), pat) for i, pat in WALK]
_WALK = {}


def _walk(i, pattern):
    if (i, pattern) not in _WALK:
        c = R.make_case(i, pattern, R.WALK_SHAPES, R.WALK_SEED)
        _WALK[(i, pattern)] = (c, R.case_f64(c))
    return _WALK[(i, pattern)]


def _kernel_constant(name):
    import re
    import whisprrec_amd
    with open(os.path.join(os.path.dirname(os.path.abspath(whisprrec_amd.__file__)), "csrc", "wr_gru.hip")) as fh:
        return int(re.search(r"constexpr int %s = (\d+);" % name, fh.read()).group(1))


def test_walk_shapes_walk_and_leave_the_old_cases_alone():
    assert R.TILE == _kernel_constant("kGruRows")
    assert R.FWD_ROWS == R.TILE * _kernel_constant("kGruFwdWg") and R.BWD_ROWS == R.TILE * _kernel_constant("kGruBwdWg")
    assert all(B > R.BWD_ROWS for B, *_ in R.WALK_SHAPES) and sum(B % R.TILE != 0 for B, *_ in R.WALK_SHAPES) >= 3   # ragged last tiles
    assert any(B > 2 * R.BWD_ROWS for B, *_ in R.WALK_SHAPES) and any(B > R.FWD_ROWS for B, *_ in R.WALK_SHAPES)
    assert {(E, H) for _, _, E, H in R.WALK_SHAPES} == {(32, 32), (64, 64), (64, 32), (32, 64)}
    assert all(B <= 130 for B, *_ in R.SHAPES)
    c = R.make_case(1, "mixed")                                              # the draws of an old case, as before
    rng = np.random.RandomState(9112)
    assert np.array_equal(c["x"][1], (rng.standard_normal((5, 3, 32)) * 0.5).astype(np.float32)[1]) and c["lengths"][1] == 3
    for i, pat in WALK:                                                      # "mixed": a later tile's lengths are its own
        n = _walk(i, pat)[0]["lengths"]
        if pat == "mixed":
            assert n.min() == 1 and n.max() == R.WALK_SHAPES[i][1] and (n[R.BWD_ROWS:] != n[:len(n) - R.BWD_ROWS]).any()


def test_walk_tolerances_are_eight_floors():
    from sasblock_ref import rule_of
    for g in R.GROUPS:
        assert 8 * R.WALK_FLOORS[g] <= R.WALK_TOL[g] <= 16 * R.WALK_FLOORS[g] and R.WALK_TOL[g] == rule_of(R.WALK_FLOORS[g]), g


@pytest.mark.parametrize("shape,pattern", WALK, ids=WALK_IDS)
def test_walk_floors_hold(shape, pattern):
    c, ref = _walk(shape, pattern)
    floors = R.worst(R.figures(R.stock(c), ref))
    print("walk floor %s %s: " % (R.WALK_SHAPES[shape], pattern) + " ".join("%s %.2e" % (g, floors[g]) for g in R.GROUPS))
    for g in R.GROUPS:
        assert 4 * floors[g] < R.WALK_TOL[g], (g, floors[g])


@pytest.mark.parametrize("wrong", R.WALK_WRONGS)
@pytest.mark.parametrize("shape,pattern", WALK, ids=WALK_IDS)
def test_walk_mutants_land_five_tolerances_out(shape, pattern, wrong):
    """parameter gradients of the first tiles only; a later tile's h and gx, or its lengths, those of the tile before; a later
    tile started from the tile before's final state.  With every length equal ("ones", "full") the lengths of the tile before
    are the right ones: that mutant is no mutant there."""
    c, ref = _walk(shape, pattern)
    if wrong == "length_of_first_visit" and pattern != "mixed":
        assert np.array_equal(R.walk_wrong(c, ref, wrong, R.BWD_ROWS)["h"], ref["h"])
        return
    fig = R.figures(R.walk_wrong(c, ref, wrong, R.BWD_ROWS), ref)
    margin = {n: v / R.WALK_TOL[R.GROUP_OF[n]] for n, v in fig.items()}
    print("walk mutant %s at %s %s: largest figure / tolerance %.1f (%s)" % (wrong, R.WALK_SHAPES[shape], pattern, max(margin.values()),
                                                                              max(margin, key=margin.get)))
    assert max(margin.values()) >= 5.0, margin


# ------------------------------------------------------------------------------------------------ the interface
def _argv(path, tmp, extra=()):
    return ["--emb_size", "32", "--hidden_size", "64", "--history_max", "20", "--model_name", "GRU4Rec", "--runner_name",
            "HipRunner", "--dataset", "ml-100k", "--path", path, "--epoch", "1", "--batch_size", "1024", "--eval_batch_size", "512",
            "--optimizer", "Adam", "--lr", "1e-3", "--l2", "0.0", "--log_file", str(tmp / "log.txt"), "--model_path",
            str(tmp / "m.pt"), "--num_workers", "0", "--topk", "5,10", "--metric", "NDCG, HR", "--random_seed", "3407"] + list(extra)


def test_parser_flags_exist_and_the_model_is_registered(tmp_path):
    from whisprrec_amd import gru4rec, main as launcher
    assert launcher.MODELS["GRU4Rec"] is gru4rec.GRU4Rec
    args, model_class, reader_class, runner_class = launcher.build_args(
        ["--model_name", "GRU4Rec", "--dataset", "ml-100k", "--path", "x/", "--log_file", str(tmp_path / "l.txt"), "--model_path",
         str(tmp_path / "m.pt")])
    assert model_class is gru4rec.GRU4Rec and reader_class.__name__ == "SeqReader" and model_class.runner == "BaseRunner"
    assert (args.emb_size, args.hidden_size, args.gru_native, args.emb_lazy, args.train_loss, args.softmax_native) == \
        (64, 64, 0, 0, "bpr", 0)
    assert model_class.extra_log_args == ["emb_size", "hidden_size", "train_loss", "softmax_native"]
    args2 = launcher.build_args(_argv("x/", tmp_path, ["--gru_native", "1", "--emb_lazy", "1"]))[0]
    assert (args2.emb_size, args2.hidden_size, args2.gru_native, args2.emb_lazy) == (32, 64, 1, 1)
    with pytest.raises(SystemExit):
        launcher.build_args(_argv("x/", tmp_path, ["--gru_native", "2"]))
    assert gru4rec.bind(gru4rec.host.SequentialModel).__qualname__ == "GRU4Rec"


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from test_reader import _write_inter
    tmp = tmp_path_factory.mktemp("gru4rec")
    return _write_inter(np.load(os.path.join(GOLD, "g8_reader.npz")), tmp), tmp


def _cpu_model(tiny, extra=()):
    from whisprrec_amd import main as launcher
    path, tmp = tiny
    args, model_class, reader_class, _ = launcher.build_args(_argv(path, tmp, extra))
    args.device = torch.device("cpu")
    corpus = reader_class(args).corpus()
    launcher.init_seed(args.random_seed)
    return model_class(args, corpus), corpus


def test_model_constructs_with_the_stated_parameters(tiny):
    m, corpus = _cpu_model(tiny)
    E, H = 32, 64
    shapes = {n: tuple(p.shape) for n, p in m.named_parameters()}
    assert shapes == {"item_embedding.weight": (m.item_num, E), "rnn.weight_ih_l0": (3 * H, E), "rnn.weight_hh_l0": (3 * H, H),
                      "rnn.bias_ih_l0": (3 * H,), "rnn.bias_hh_l0": (3 * H,), "out.weight": (E, H), "out.bias": (E,)}
    assert m.gru_native is False and m.train_loss == "bpr" and m.emb_lazy is False
    assert not m.out.bias.detach().any()                                        # the linears' initialisation
    assert float(m.rnn.weight_hh_l0.detach().abs().max()) <= 1 / np.sqrt(H)     # nn.GRU's own: uniform(-1/sqrt(H), 1/sqrt(H))
    # the stock path's own ops on a CPU (the embedding lookup is a HIP kernel, so the rows are indexed here): the row at
    # lengths - 1 of the padded run, through `out`, is the float64 restatement
    rng = np.random.RandomState(5)
    B, T = 9, 6
    lengths = rng.randint(1, T + 1, B)
    lengths[:2] = [T, 1]
    hist = rng.randint(1, m.item_num, (B, T)) * (np.arange(T)[None, :] < lengths[:, None])
    with torch.no_grad():
        output, _ = m.rnn(m.item_embedding.weight[torch.from_numpy(hist)])
        got = m.out(output[torch.arange(B), torch.from_numpy(lengths) - 1, :])
    sd = {n: v.detach().numpy() for n, v in m.state_dict().items()}
    ref = R.gru_f64(sd["item_embedding.weight"][hist], lengths, sd["rnn.weight_ih_l0"], sd["rnn.weight_hh_l0"],
                    sd["rnn.bias_ih_l0"], sd["rnn.bias_hh_l0"])["h"] @ sd["out.weight"].astype(np.float64).T + sd["out.bias"]
    assert got.shape == (B, E) and R.rel_err(got.numpy(), ref) < R.TOL["h"]
    assert m.eval_items() is m.item_embedding.weight and m.training


def test_softmax_with_the_row_lazy_table_is_refused(tiny):
    with pytest.raises(ValueError, match="every item row gets a gradient every step"):
        _cpu_model(tiny, ["--train_loss", "softmax", "--emb_lazy", "1"])
    m, _ = _cpu_model(tiny, ["--train_loss", "softmax"])
    assert m.train_loss == "softmax" and m.softmax_native is False


def test_c_abi_refuses_unsupported_shapes_with_the_numbers():
    from whisprrec_amd import abi
    L = abi.lib()
    for E, H in ((32, 32), (32, 64), (64, 32), (64, 64)):
        assert L.wr_gru_supported(E, H, 1) == 1 and L.wr_gru_supported(E, H, 100_000) == 1
    for E, H, T in ((128, 64, 20), (64, 128, 20), (48, 64, 20), (64, 64, 0)):
        assert L.wr_gru_supported(E, H, T) == 0, (E, H, T)
    assert L.wr_gru_workspace_bytes(8, 20, 64, 128) == -5
    msg = abi.last_error()
    assert "E=64" in msg and "H=128" in msg
    # the bound is independent of B and T: 256 slabs of the parameter gradients
    assert L.wr_gru_workspace_bytes(1, 1, 64, 64) == L.wr_gru_workspace_bytes(1 << 20, 500, 64, 64) == \
        256 * (3 * 64 * 128 + 6 * 64) * 4
    keep = ctypes.create_string_buffer(96)                                  # nothing is dereferenced: every call is refused
    addr = (ctypes.addressof(keep) + 15) // 16 * 16
    rc = L.wr_gru_fwd(addr, addr, addr, addr, addr, addr, 4, 20, 128, 64, addr, None, None)
    assert rc == -5 and "E=128" in abi.last_error() and "H=64" in abi.last_error()
    rc = L.wr_gru_fwd(addr, addr, addr, addr, addr, addr, 4, 20, 64, 128, addr, None, None)
    assert rc == -5 and "E=64" in abi.last_error() and "H=128" in abi.last_error()
    rc = L.wr_gru_bwd(addr, addr, addr, addr, addr, addr, addr, addr, 4, 20, 64, 128, addr, addr, addr, addr, addr, addr, 1 << 30,
                      None)
    assert rc == -5 and "H=128" in abi.last_error()
    rc = L.wr_gru_fwd(None, addr, addr, addr, addr, addr, 4, 20, 64, 64, addr, None, None)
    assert rc == -1 and "NULL" in abi.last_error()
    rc = L.wr_gru_bwd(addr, addr, addr, addr, addr, addr, addr, addr, 4, 20, 64, 64, addr, addr, addr, addr, addr, addr, 16, None)
    assert rc != 0 and "workspace" in abi.last_error()


def test_host_wrappers_refuse_cpu_tensors():
    from whisprrec_amd import abi, hip_ops
    c = R.make_case(1, "mixed")
    t = {n: torch.from_numpy(v) for n, v in c.items()}
    with pytest.raises(abi.WhisprRecHipError, match="no CPU fallback"):
        hip_ops.gru_fwd(t["x"], t["lengths"], t["wih"], t["whh"], t["bih"], t["bhh"])
    with pytest.raises(abi.WhisprRecHipError, match="no CPU fallback"):
        hip_ops.gru_last(t["x"], t["lengths"], t["wih"], t["whh"], t["bih"], t["bhh"])
