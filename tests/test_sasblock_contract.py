"""CPU checks around wr_sasblock_fwd / wr_sasblock_bwd (K13): the float64 restatement the GPU test compares against equals
`_Block` in float64 under torch.autograd, alone and inside the whole model on the reference's golden batch; the tolerances
stand well above the fp32 floor of the stock block on the GPU test's own shapes; deliberately wrong blocks land above them;
the dropout mask generator has the right rate and independent streams; and argument errors are reported before any launch."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sasblock_ref as R  # noqa: E402
from conftest import rel_err  # noqa: E402
from whisprrec_amd import host  # noqa: E402

SEED = 0x5A5B10C


@pytest.fixture(scope="module")
def cases(g5):
    return [R.make_case(i, g5) for i in range(len(R.SHAPES))]


@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_restatement_equals_the_block_in_float64_under_autograd(cases, i):
    x, sd, g, heads = cases[i]
    for p in (0.0, 0.1):
        m1, m2 = R.masks_for(SEED + i, *x.shape, p)
        ref = R.block_f64(x, sd, heads, g, m1, m2)
        out, gx, gp = R.stock_fp32(x, sd, heads, g, m1, m2, dtype=torch.float64)
        fig = R.figures(out, gx, gp, ref)
        assert max(fig.values()) <= 1e-12, fig


def test_restatement_reproduces_the_golden_loss_and_gradient_inside_the_model(g5):
    """the whole model in float64 on the CPU, its block replaced by the restatement (forward and backward): g5's loss and
    gW_full at the bounds of tests/test_sasrec_embedding.py"""
    f = torch.float64
    sd = {k[4:]: torch.from_numpy(g5[k]).to(f) for k in g5.files if k.startswith("sd__")}
    W = sd["item_embedding.weight"].clone().requires_grad_(True)
    hist, lengths = torch.from_numpy(g5["hist"]), torch.from_numpy(g5["lengths"])
    pos, neg = torch.from_numpy(g5["pos"]), torch.from_numpy(g5["neg"]).reshape(-1)
    B, T = hist.shape
    bsd = {n: g5["sd__transformer_block.0." + n] for n in R.PARAMS}

    class Restated(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.x = x.detach().numpy()
            return torch.from_numpy(R.block_f64(ctx.x, bsd, 4)["out"])

        @staticmethod
        def backward(ctx, g):
            return torch.from_numpy(R.block_f64(ctx.x, bsd, 4, g.numpy())["gx"])

    x = W[hist] + sd["position_embedding.weight"][torch.arange(T)][None]
    x = Restated.apply(x) * (hist > 0).to(f)[:, :, None]
    user = x[torch.arange(B), lengths - 1, :]
    loss = -torch.log(1e-10 + torch.sigmoid((user * W[pos]).sum(1) - (user * W[neg]).sum(1))).mean()
    loss.backward()
    gW = W.grad.numpy().copy()
    gW[0] = 0.0                                                           # padding_idx = 0
    assert abs(float(loss.detach()) - float(g5["loss"][0])) / float(g5["loss"][0]) < 1e-4
    assert rel_err(gW, g5["gW_full"]) < 1e-4


def test_tolerances_stand_above_the_fp32_floor_of_the_stock_block(cases):
    """the stock fp32 `_Block` against the restatement on the GPU test's shapes: 4 x floor < TOL for each group of figures"""
    worst = {k: 0.0 for k in R.TOL}
    for i, (x, sd, g, heads) in enumerate(cases):
        for p in (0.0, 0.1):
            m1, m2 = R.masks_for(SEED + i, *x.shape, p)
            fig = R.figures(*R.stock_fp32(x, sd, heads, g, m1, m2), R.block_f64(x, sd, heads, g, m1, m2))
            print(R.fmt("floor B=%d T=%d D=%d h=%d p=%g" % (*R.SHAPES[i], p), fig))
            for k, v in R.worst(fig).items():
                worst[k] = max(worst[k], v)
    print("floor (largest): " + " ".join("%s %.2e" % kv for kv in worst.items()))
    for k in R.TOL:
        assert 4.0 * worst[k] < R.TOL[k], (k, worst[k], R.TOL[k])
        assert 8.0 * R.FLOORS[k] <= R.TOL[k] <= 16.0 * R.FLOORS[k]      # the 8 x rule of the recorded floors, not a loose bar


WRONG = ["no_scale", "mask_shift", "ln_no_eps", "ln_no_bias_grad", "drop_no_scale", "v_head", "relu_gate", "skip_seq"]


@pytest.mark.parametrize("wrong", WRONG)
def test_wrong_blocks_land_above_the_tolerances(cases, wrong):
    """missing 1/sqrt(d_k); causal mask shifted by one; LayerNorm without eps / without its bias gradient; dropout without
    the 1/(1-p) scale; one head's v gradient dropped; the ReLU gate ignored in the backward; one sequence missing from the
    weight-gradient sums — each exceeds TOL on at least one figure"""
    x, sd, g, heads = cases[0]
    if wrong == "ln_no_eps":
        x = x.copy()
        x[:, :, :] = x[:, :1, :1] * 1e-3                                  # nearly constant rows: var ~ eps, where eps matters
        x += np.random.RandomState(1).standard_normal(x.shape).astype(np.float32) * 1e-3
    m1, m2 = R.masks_for(SEED, *x.shape, 0.1)
    ref = R.block_f64(x, sd, heads, g, m1, m2)
    bad = R.block_f64(x, sd, heads, g, m1, m2, wrong=wrong + (":%r" % R.drop_scale(0.1) if wrong == "drop_no_scale" else ""))
    fig = R.figures(bad["out"], bad["gx"], bad["g"], ref)
    over = [n for n, v in fig.items() if v > R.TOL[R.group_of(n)]]
    assert over, fig
    clean = R.figures(ref["out"], ref["gx"], ref["g"], ref)
    assert all(v == 0.0 for v in clean.values())


# ------------------------------------------------------------------------------------------------ several visits, every form
LISTS = {"walk": (R.WALK_SHAPES, R.WALK_SEED, R.WALK_FLOORS, R.WALK_TOL), "form": (R.FORM_SHAPES, R.FORM_SEED, R.FORM_FLOORS, R.FORM_TOL)}
_LIST_REFS = {}


def _list_ref(which, i, p):
    """(inputs, masks, float64 result) of a case of WALK_SHAPES / FORM_SHAPES, computed once"""
    if (which, i, p) not in _LIST_REFS:
        shapes, seed = LISTS[which][:2]
        x, sd, g, heads = R.make_case(i, shapes=shapes, seed=seed)
        m1, m2 = R.masks_for(SEED + seed + i, *x.shape, p)
        _LIST_REFS[(which, i, p)] = ((x, sd, g, heads), (m1, m2), R.block_f64(x, sd, heads, g, m1, m2))
    return _LIST_REFS[(which, i, p)]


def _kernel_constant(source, name):
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(host.__file__)), "csrc", source)
    with open(path) as fh:
        return int(re.search(r"constexpr int %s = (\d+);" % name, fh.read()).group(1))


def test_walk_shapes_walk_and_the_new_lists_leave_the_old_cases_alone(g5):
    """every WALK shape has B above the backward's cap, one above forward launch 1's; the caps restated in sasblock_ref.py are the
    kernel's; FORM_SHAPES holds T = 24 and T = 25 at both D and a <32, 64> shape; SHAPES' data is what it was"""
    assert R.FWD_WG == _kernel_constant("wr_sasblock.hip", "kSasFwdWg") and R.BWD_WG == _kernel_constant("wr_sasblock.hip", "kSasBwdWg")
    assert all(B > R.BWD_WG and B % R.BWD_WG not in (0, R.BWD_WG - 1) for B, _, _, _ in R.WALK_SHAPES)      # a ragged last visit
    assert any(B > 2 * R.BWD_WG for B, _, _, _ in R.WALK_SHAPES)                                            # a few workgroups visit three
    assert any(B > R.FWD_WG for B, _, _, _ in R.WALK_SHAPES)
    assert any(B > R.BWD_WG and D == 32 and T > 24 for B, T, D, _ in R.WALK_SHAPES)
    assert {(D, T) for _, T, D, _ in R.FORM_SHAPES} >= {(32, 24), (32, 25), (64, 24), (64, 25), (32, 64)}
    assert all(B <= 130 for B, _, _, _ in R.SHAPES)
    x, sd, g, heads = R.make_case(2)
    rng = np.random.RandomState(7002)                                                                    # the draws of case 2, as before
    R.xavier_params(32, 2, rng)
    assert np.array_equal(x, (rng.standard_normal((5, 7, 32)) * np.sqrt(2.0 / (3706 + 32)) * np.sqrt(2.0)).astype(np.float32))
    assert not np.array_equal(R.make_case(2, shapes=R.FORM_SHAPES, seed=R.FORM_SEED)[1]["linear1.bias"], sd["linear1.bias"])


@pytest.mark.parametrize("which", ["walk", "form"])
def test_walk_and_form_tolerances_stand_above_the_fp32_floor_of_the_stock_block(which):
    shapes, seed, floors, tol = LISTS[which]
    worst = {k: 0.0 for k in tol}
    for i in range(len(shapes)):
        for p in (0.0, 0.1):
            (x, sd, g, heads), (m1, m2), ref = _list_ref(which, i, p)
            stock = R.stock_fp32(x, sd, heads, g, m1, m2)
            fig = R.figures(*stock, ref)
            print(R.fmt("%s floor B=%d T=%d D=%d h=%d p=%g" % (which, *shapes[i], p), fig, tol))
            for k, v in R.worst(fig).items():
                worst[k] = max(worst[k], v)
            if p == 0.1:                      # the restatement itself, in float64 under autograd
                f64 = R.figures(*R.stock_fp32(x, sd, heads, g, m1, m2, dtype=torch.float64), ref)
                assert max(f64.values()) <= 1e-12, f64
    print("%s floor (largest): " % which + " ".join("%s %.2e" % kv for kv in worst.items()))
    for k in tol:
        assert 4.0 * worst[k] < tol[k], (k, worst[k], tol[k])
        assert 8.0 * floors[k] <= tol[k] <= 16.0 * floors[k] and tol[k] == R.rule_of(floors[k])
        assert R.rule_of(R.FLOORS[k]) == R.TOL[k]


WALK_WRONG = ["later_visits_dropped", "later_visits_stale", "mask_of_first_visit"]


@pytest.mark.parametrize("wrong", WALK_WRONG)
@pytest.mark.parametrize("i", range(len(R.WALK_SHAPES)))
def test_walk_mutants_land_five_tolerances_out(i, wrong):
    """parameter gradients summed over each workgroup's first visit only; the output and gx of a later visit those of the visit
    before; the dropout mask of a later visit taken at the first visit's b — each exceeds 5 x WALK_TOL on some figure, at every
    walk shape"""
    (x, sd, g, heads), (m1, m2), ref = _list_ref("walk", i, 0.1)
    if wrong == "later_visits_dropped":
        bad = R.block_f64(x, sd, heads, g, m1, m2, wrong=wrong, first=R.BWD_WG)
    elif wrong == "later_visits_stale":
        bad = R.stale(ref, R.BWD_WG)
    else:
        src = R.first_visit_of(x.shape[0], R.BWD_WG)
        bad = R.block_f64(x, sd, heads, g, m1[src], m2[src])
    fig = R.figures(bad["out"], bad["gx"], bad["g"], ref)
    margin = {n: v / R.WALK_TOL[R.group_of(n)] for n, v in fig.items()}
    print("walk mutant %s at %s: largest figure / tolerance %.1f (%s)" % (wrong, R.WALK_SHAPES[i], max(margin.values()), max(margin, key=margin.get)))
    assert max(margin.values()) >= 5.0, margin
    if wrong == "later_visits_stale":         # and the per-visit figures say which side is wrong
        first, later = R.visit_figures(bad, ref, R.BWD_WG)["out"]
        assert first == 0.0 and later == fig["out"]


def test_walk_maximum_of_the_first_visits_only_misses_the_stored_maximum():
    """`max_of_first_visit`: the GPU test's case (x of sequence 2049 of (2051, 2, 64, 4) times 100) — a maximum folded over the
    first kSasFwdWg sequences misses the call's by far more than 5 x the 1e-5 the stored one is held to"""
    i = R.WALK_SHAPES.index((2051, 2, 64, 4))
    x, sd, g, heads = R.make_case(i, shapes=R.WALK_SHAPES, seed=R.WALK_SEED)
    x = x.copy()
    x[2049] *= 100.0
    ref = R.block_f64(x, sd, heads)
    bad = ref["seq_max"][:R.FWD_WG].max()
    assert ref["gmax"] == ref["seq_max"].max() and 10.0 < ref["gmax"] - bad < 30.0
    assert abs(bad - ref["gmax"]) > 5.0 * 1e-5 * abs(ref["gmax"])


# ------------------------------------------------------------------------------------------------ the mask generator
def test_mask_generator_rate_and_streams():
    n = 1 << 20
    for p in (0.1, 0.5):
        keep = R.keep_mask(SEED, 0, 1, n // 64, 64, p)
        q = 1.0 - R.drop_threshold(p) / 16777216.0
        assert abs(keep.mean() - (1.0 - p)) < 5.0 * np.sqrt(p * (1.0 - p) / n) + abs(q - (1.0 - p))
    a = R.keep_mask(SEED, 0, 16, 20, 64, 0.1)
    assert not np.array_equal(a, R.keep_mask(SEED, 1, 16, 20, 64, 0.1))          # the two sites differ
    assert not np.array_equal(a, R.keep_mask(SEED + 1, 0, 16, 20, 64, 0.1))      # and so do two seeds
    assert np.array_equal(a, R.keep_mask(SEED, 0, 16, 20, 64, 0.1))
    assert R.keep_mask(SEED, 0, 16, 20, 64, 0.0).all()                           # p = 0 keeps all
    assert R.masks_for(SEED, 4, 5, 32, 0.0) == (None, None)
    # the element index is (b T + t) D + d: a larger batch extends the stream, it does not reshuffle it
    assert np.array_equal(R.keep_mask(SEED, 0, 32, 20, 64, 0.1)[:16], a)


# ------------------------------------------------------------------------------------------------ interface
def _lib():
    from whisprrec_amd import abi
    assert os.path.exists(abi.LIB_PATH), "run __graft_entry__.build() first"    # a missing library is a failed build, not a skip
    return abi, abi.lib()


def test_supported_set_and_workspace():
    abi, L = _lib()
    for D in (32, 64):
        for h in (1, 2, 4):
            for T in (1, 20, 24, 25, 64):
                assert L.wr_sasblock_supported(D, D, h, T) == 1
    for D, F, h, T in ((48, 48, 4, 20), (128, 128, 4, 20), (64, 128, 4, 20), (64, 64, 3, 20), (64, 64, 8, 20), (32, 32, 8, 20),
                       (64, 64, 4, 65), (64, 64, 4, 0), (64, 64, 0, 20)):
        assert L.wr_sasblock_supported(D, F, h, T) == 0, (D, F, h, T)
    Bs, Ts = [1, 2, 96, 511, 512, 513, 2048, 4096, 65536], [1, 7, 20, 24, 25, 33, 64]
    for D in (32, 64):
        grid = np.array([[L.wr_sasblock_workspace_bytes(B, T, D, D, 4) for T in Ts] for B in Bs], dtype=np.int64)
        assert (grid > 0).all()
        assert (np.diff(grid, axis=0) >= 0).all() and (np.diff(grid, axis=1) >= 0).all()      # never decreases as B or T grow
    assert L.wr_sasblock_workspace_bytes(96, 20, 48, 48, 4) == -5 and "D=48" in abi.last_error()
    assert L.wr_sasblock_workspace_bytes(0, 20, 64, 64, 4) == -2


def test_argument_errors_are_reported_before_any_launch():
    """no GPU here: every one of these returns before a launch"""
    abi, L = _lib()
    buf = (ctypes.c_float * 4096)()
    a16 = (ctypes.addressof(buf) + 15) // 16 * 16
    ptrs = (ctypes.c_void_p * 14)(*([a16] * 14))
    pp = ctypes.addressof(ptrs)

    def fwd(x=a16, B=4, T=20, D=64, F=64, h=4, params=pp, p=0.1, out=a16, gmax=a16, ws=a16, ws_bytes=1 << 40):
        return L.wr_sasblock_fwd(x, B, T, D, F, h, params, p, 1, 1, out, gmax, ws, ws_bytes, None)

    def bwd(x=a16, g=a16, B=4, T=20, D=64, F=64, h=4, params=pp, p=0.1, gmax=a16, gx=a16, gp=a16, ws=a16, ws_bytes=1 << 40):
        return L.wr_sasblock_bwd(x, g, B, T, D, F, h, params, p, 1, 1, gmax, gx, gp, ws, ws_bytes, None)

    for call in (fwd, bwd):
        assert call(D=48, F=48) == -5 and "D=48" in abi.last_error()           # unsupported D
        assert call(h=8) == -5 and "n_heads=8" in abi.last_error()             # unsupported heads
        assert call(T=65) == -5 and "T=65" in abi.last_error()                 # unsupported T
        assert call(T=0) == -2 and "T=0" in abi.last_error()                   # T = 0
        assert call(B=0) == -2
        assert call(x=None) == -1 and "NULL" in abi.last_error()               # a NULL pointer
        assert call(params=None) == -1
        assert call(x=a16 + 4) == -4 and "aligned" in abi.last_error()         # a misaligned pointer
        assert call(ws_bytes=1024) == -3 and "workspace" in abi.last_error()   # a short workspace
        assert call(ws=None) == -3
        assert call(p=1.0) == -5 and "dropout" in abi.last_error()
    bad = (ctypes.c_void_p * 14)(*([a16] * 13 + [None]))
    assert fwd(params=ctypes.addressof(bad)) == -1 and "parameter 13" in abi.last_error()
    bad = (ctypes.c_void_p * 14)(*([a16] * 3 + [a16 + 4] + [a16] * 10))
    assert bwd(params=ctypes.addressof(bad)) == -4 and "parameter 3" in abi.last_error()
    assert bwd(gp=None) == -1


def test_model_accepts_the_flag_and_wrapper_refuses_cpu_tensors():
    from whisprrec_amd import abi, hip_ops
    from whisprrec_amd.sasrec import SASRec, _Block
    p = argparse.ArgumentParser()
    SASRec.parse_model_args(p)
    assert p.parse_args([]).block_native == 0
    assert p.parse_args(["--block_native", "1"]).block_native == 1
    from whisprrec_amd import main as launcher
    assert launcher.build_args(["--model_name", "SASRec", "--block_native", "1"])[0].block_native == 1
    args = argparse.Namespace(device="cpu", model_path="/tmp/wr_sas.pt", buffer=1, num_neg=1, test_all=1, emb_size=64, num_layers=2,
                              num_heads=4, dropout=0.1, history_max=20)
    m = SASRec(args, host.Corpus(13, 71, {}))
    assert m.block_native is False and not m._use_block_native(20)              # off by default
    blk = _Block(64, 64, 4, 0.1)
    assert [n for n, _ in blk.named_parameters()] == list(hip_ops.SASBLOCK_PARAMS) == R.PARAMS
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.sasrec_block(torch.zeros(2, 20, 64), blk, 4, 0.1, 1, True)
