"""CPU checks for IF4Rec: the float64 restatements of tests/if4rec_ref.py against the reference formula under autograd, the
torch-path model against the numbers recorded from the reference itself (tests/golden/g14_if4rec.npz), the tolerances against
the fp32 floor, the wrong variants against the tolerances, and the interface (launcher, C-ABI argument errors, wrappers, runner)
— nothing here needs a GPU."""
import argparse
import ctypes
import logging
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import if4rec_ref as R  # noqa: E402
from conftest import rel_err  # noqa: E402
from whisprrec_amd import host  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def _one_thread():
    """the floors are fp32 sums: one thread, so that they are the same figures on every machine"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def g14():
    return np.load(os.path.join(GOLD, "g14_if4rec.npz"))


@pytest.fixture(scope="module")
def cases():
    return [R.make_case(i) for i in range(len(R.CASES))]


@pytest.fixture(scope="module")
def refs(cases):
    return [R.pool_ref(c, g_out=c["g_out"]) for c in cases]


def torch_pool(c, dtype):
    """IF4Rec.py:87-103 as written on stock torch ops under autograd (the global-maximum shift included) -> the figures' arrays"""
    t = {k: torch.tensor(c[k], dtype=dtype, requires_grad=True) for k in ("item", "pos", "W1", "b1", "W2", "b2")}
    hist = torch.from_numpy(c["hist"])
    valid = (hist > 0).long()
    position = torch.arange(hist.shape[1])[None, :] * valid
    hp = F.embedding(hist, t["item"]) + F.embedding(position, t["pos"])
    hp.retain_grad()
    attn = F.linear(F.leaky_relu(F.linear(hp, t["W1"], t["b1"])), t["W2"], t["b2"])
    attn = attn.masked_fill(valid.unsqueeze(-1) == 0, -np.inf)
    attn = attn.transpose(-1, -2)
    attn = (attn - attn.max()).softmax(dim=-1)
    attn = attn.masked_fill(torch.isnan(attn), 0)
    out = (hp[:, None, :, :] * attn[:, :, :, None]).sum(-2)
    out.backward(torch.tensor(c["g_out"], dtype=dtype))
    return dict(out=out.detach().numpy(), g_hp=hp.grad.numpy(), g_item=t["item"].grad.numpy(), g_pos=t["pos"].grad.numpy(),
                gW1=t["W1"].grad.numpy(), gb1=t["b1"].grad.numpy(), gW2=t["W2"].grad.numpy(), gb2=t["b2"].grad.numpy())


# ------------------------------------------------------------------------------------------------ the restatements
def test_cases_hold_the_rows_the_issue_names(cases):
    assert len(cases) == 7
    for (B, T, D, A, K), c in zip(R.CASES, cases):
        assert c["hist"].shape == (B, T) and c["W1"].shape == (A, D) and c["W2"].shape == (K, A)
        if B >= 3:
            n_valid = (c["hist"] > 0).sum(axis=1)
            assert n_valid[0] == 1 and n_valid[1] == T and n_valid[B - 1] == 0
        if B >= 4 and T >= 3:
            assert c["hist"][2, 1] == 0 and c["hist"][2, 0] > 0 and c["hist"][2, 2] > 0        # an interior zero
    s = R.pool_ref(cases[R.SPREAD_CASE])["s"]
    assert 55 <= np.abs(s[np.isfinite(s)]).max() <= 65


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_pool_restatement_equals_the_reference_formula_in_float64_under_autograd(cases, refs, i):
    c = R.drop_zero_rows(cases[i])                  # autograd passes NaN through an all-zero row; the restatement passes 0
    got, ref = torch_pool(c, torch.float64), R.pool_ref(c, g_out=c["g_out"])
    for k, v in R.figures(got, ref).items():
        assert v <= 1e-12, (k, v)
    full = refs[i]                                  # ... and the all-zero row adds nothing and is finite
    for k in ("g_item", "g_pos", "gW1", "gb1", "gW2", "gb2"):
        assert np.isfinite(full[k]).all() and R.figure(full[k], ref[k]) <= 1e-14, k
    zero = ~(cases[i]["hist"] > 0).any(axis=1)
    assert (full["out"][zero] == 0).all() and (full["g_hp"][~(cases[i]["hist"] > 0)] == 0).all()


def test_floors_and_tolerance(cases):
    """FLOORS = the stock fp32 torch path against float64; TOL = 8 x the largest, rounded up to one digit; 4 x floor < TOL"""
    floors = {k: 0.0 for k in R.FIGURES}
    for c in cases:
        c = R.drop_zero_rows(c)
        fig = R.figures(torch_pool(c, torch.float32), R.pool_ref(c, g_out=c["g_out"]))
        for k, v in fig.items():
            floors[k] = max(floors[k], v)
    print("if4rec floors (fp32 torch vs float64): " + " ".join("%s=%.2e" % kv for kv in floors.items()))
    top = 8 * max(R.FLOORS.values())
    digit = 10.0 ** np.floor(np.log10(top))
    assert R.TOL == pytest.approx(np.ceil(top / digit - 1e-9) * digit, rel=1e-9)
    for k, v in floors.items():
        assert 4 * v < R.TOL, (k, v)


@pytest.mark.parametrize("wrong", R.WRONG_POOL)
def test_wrong_pooling_variants_land_above_the_tolerance(cases, refs, wrong):
    worst = 0.0
    for c, ref in zip(cases, refs):
        fig = R.figures(R.pool_ref(c, variant=wrong, g_out=c["g_out"]), ref)
        worst = max(worst, max(fig.values()))
    assert worst > 10 * R.TOL, (wrong, worst)


# ------------------------------------------------------------------------------------------------ several visits per workgroup
@pytest.fixture(scope="module")
def walk_cases():
    cases = [R.make_case(i, R.WALK_CASES, R.WALK_SEED) for i in range(len(R.WALK_CASES))]
    return [(c, R.pool_ref(c, g_out=c["g_out"])) for c in cases]


def _kernel_constant(name):
    import re
    import whisprrec_amd
    with open(os.path.join(os.path.dirname(os.path.abspath(whisprrec_amd.__file__)), "csrc", "wr_if4rec.hip")) as fh:
        return int(re.search(r"constexpr int %s = (\d+);" % name, fh.read()).group(1))


def test_walk_cases_walk_hold_their_rows_and_leave_the_old_cases_alone(cases, walk_cases):
    assert R.FWD_WG == _kernel_constant("kIpFwdWg") and R.BWD_WG == _kernel_constant("kIpBwdWg")
    G = R.BWD_WG
    assert all(B > G and B % G not in (0, G - 1) for B, *_ in R.WALK_CASES)                      # a ragged last visit
    assert any(B > 2 * G for B, *_ in R.WALK_CASES) and any(B > R.FWD_WG for B, *_ in R.WALK_CASES)
    assert all(B <= 130 for B, *_ in R.CASES)
    for (B, T, D, A, K), (c, _) in zip(R.WALK_CASES, walk_cases):
        n_valid = (c["hist"] > 0).sum(axis=1)
        assert c["hist"].shape == (B, T) and c["W1"].shape == (A, D) and c["W2"].shape == (K, A)
        assert n_valid[0] == 1 and n_valid[1] == T and n_valid[B - 1] == 0
        if T >= 3:
            assert c["hist"][2, 1] == 0 and c["hist"][2, 0] > 0 and c["hist"][2, 2] > 0            # an interior zero
        assert n_valid[G + 1] == 1 and (n_valid[G:] == 0).any()                                   # ... and on a later visit
        assert ((c["hist"] > 0)[G:] != (c["hist"] > 0)[:B - G]).any()
    c = cases[2]                                                                                 # the draws of an old case, as before
    rng = np.random.RandomState(1402)
    assert np.array_equal(c["item"], (rng.standard_normal((R.N_ITEMS, 32)) * 0.5).astype(np.float32))


def test_walk_floors_and_tolerance(walk_cases):
    """WALK_FLOORS = the stock fp32 torch path against float64 over WALK_CASES; WALK_TOL = 8 x the largest, rounded up to one
    digit; 4 x floor < WALK_TOL"""
    floors = {k: 0.0 for k in R.FIGURES}
    for c, _ in walk_cases:
        c = R.drop_zero_rows(c)
        ref = R.pool_ref(c, g_out=c["g_out"])
        fig = R.figures(torch_pool(c, torch.float32), ref)
        for k, v in fig.items():
            floors[k] = max(floors[k], v)
        for k, v in R.figures(torch_pool(c, torch.float64), ref).items():      # and the restatement holds at these sizes
            assert v <= 1e-12, (k, v)
    print("if4rec walk floors (fp32 torch vs float64): " + " ".join("%s=%.2e" % kv for kv in floors.items()))
    top = 8 * max(R.WALK_FLOORS.values())
    digit = 10.0 ** np.floor(np.log10(top))
    assert R.WALK_TOL == pytest.approx(np.ceil(top / digit - 1e-9) * digit, rel=1e-9)
    assert 8 * max(R.WALK_FLOORS.values()) <= R.WALK_TOL <= 16 * max(R.WALK_FLOORS.values())
    for k, v in floors.items():
        assert 4 * v < R.WALK_TOL, (k, v)


@pytest.mark.parametrize("wrong", R.WALK_WRONG)
@pytest.mark.parametrize("i", range(len(R.WALK_CASES)))
def test_walk_mutants_land_five_tolerances_out(walk_cases, i, wrong):
    """parameter and position gradients of the first visits only; a later visit's out and g_hp, or its history mask, those of the
    visit before — each exceeds 5 x WALK_TOL on some figure, at every walk case"""
    c, ref = walk_cases[i]
    fig = R.figures(R.walk_wrong(c, ref, wrong, R.BWD_WG), ref)
    print("walk mutant %s at %s: largest figure / tolerance %.1f (%s)" % (wrong, R.WALK_CASES[i], max(fig.values()) / R.WALK_TOL,
                                                                           max(fig, key=fig.get)))
    assert max(fig.values()) >= 5.0 * R.WALK_TOL, fig


@pytest.mark.parametrize("KQ", [2, 4])
@pytest.mark.parametrize("wrong", R.WRONG_RANK)
def test_wrong_rank_variants_change_judged_ranks(wrong, KQ):
    c = R.make_rank_case(64, 2100, 257, KQ)
    rank, margin = R.rank_ref(c)
    ok = margin > R.RANK_MARGIN
    assert ok.mean() > 0.9
    assert (R.rank_ref(c, variant=wrong)[0][ok] != rank[ok]).mean() > 0.05


def test_rank_restatement_on_a_tiny_example():
    c = dict(queries=np.array([[[1.0, 0.0], [0.0, 1.0]]], np.float32), items=np.array([[3, 0], [0, 2], [1, 1], [4, 4]], np.float32),
             target=np.array([1]), mask_ptr=np.array([0, 1]), mask_idx=np.array([3], np.int32), mask_row=np.array([0]))
    rank, _ = R.rank_ref(c)                     # scores: max(3,0)=3, max(0,2)=2, 1, (4 masked) -> the target (2) is second
    assert rank.tolist() == [2]


# ------------------------------------------------------------------------------------------------ the model against g14
def _args(**kw):
    base = dict(device="cpu", model_path="/tmp/wr_if4rec.pt", buffer=1, num_neg=1, test_all=1, history_max=20, emb_size=64, attn_size=8,
                K=2, add_pos=1, encoder_layer=1, n_head=8, encoder_dropout=0.0, add_multi=1, interest_native=0, block_native=0)
    base.update(kw)
    return argparse.Namespace(**base)


def _cpu_model(g14, **kw):
    """the torch-path model on the CPU: the row gather of HipEmbedding (K9, tested on its own) replaced by nn.Embedding"""
    from whisprrec_amd.if4rec import IF4Rec
    m = IF4Rec(_args(**kw), host.Corpus(40, 300, {}))
    assert list(m.state_dict().keys()) == [str(n) for n in g14["names"]]
    sd = {str(n): torch.from_numpy(g14["sd__" + str(n)]) for n in g14["names"]}
    if kw.get("K", 2) == 4:
        sd.update({k: torch.from_numpy(g14["k4__sd__" + k]) for k in ("W2.weight", "W2.bias")})
    m.load_state_dict(sd)
    emb = torch.nn.Embedding(300, 64)
    emb.weight = m.i_embeddings.weight
    m.i_embeddings = emb
    return m


def _feed(g14, rows=None):
    sel = slice(None) if rows is None else rows
    return {"history_items": torch.from_numpy(g14["history"][sel]), "lengths": torch.from_numpy(g14["lengths"][sel]),
            "pos_item": torch.from_numpy(g14["item_id"][sel, 0]), "neg_items": torch.from_numpy(g14["item_id"][sel, 1:]),
            "phase": "train", "batch_size": 96}


def test_g14_batch_covers_the_lengths(g14):
    lens = g14["lengths"]
    assert lens.min() == 1 and lens.max() == 20 and len(np.unique(lens)) > 10 and g14["history"].shape == (96, 20)
    assert g14["history"][5, 2] == 0 and g14["history"][5, 1] > 0 and g14["history"][5, 3] > 0    # the interior zero
    assert os.path.getsize(os.path.join(GOLD, "g14_if4rec.npz")) < 400 * 1024


@pytest.mark.parametrize("prefix, kw", [("", {}), ("k4__", dict(K=4, n_head=4))])
def test_torch_path_model_reproduces_the_reference(g14, prefix, kw):
    m = _cpu_model(g14, **kw)
    m.train()
    loss = m.predict(_feed(g14))
    loss.backward()
    assert rel_err(m.last_prediction.numpy(), g14[prefix + "pred"]) <= 2e-6
    assert abs(float(loss.detach()) - float(g14[prefix + "loss"][0])) <= 2e-6 * abs(float(g14[prefix + "loss"][0]))
    checked = 0
    for n, p in m.named_parameters():
        if prefix + "g__" + n in g14.files:
            assert rel_err(p.grad.numpy(), g14[prefix + "g__" + n]) <= 2e-5, n      # same ops as the reference, in another order
            checked += 1
    assert checked == sum(1 for _, p in m.named_parameters() if prefix == "" or p.numel() <= 2048)
    m.eval()
    with torch.no_grad():
        scores = m.full_predict(_feed(g14, g14["fp_rows"]))
    assert scores.shape == (4, 300) and rel_err(scores.numpy(), g14[prefix + "fp_scores"]) <= 2e-6


def test_model_floors(g14):
    """the stock fp32 model against its float64 self on g14's batch: every gradient outside the blocks' score path sits far below
    TOL, the score-path gradients (sums that cancel; if4rec_ref.SCORE_PATH) miss it on the stock path itself and get 8 x their own
    floor"""
    floor_qk, floor_rest = 0.0, 0.0
    for heads in (8, 4):
        grads = {}
        for dtype in (torch.float32, torch.float64):
            m = _cpu_model(g14, n_head=heads).to(dtype).train()
            m.predict(_feed(g14)).backward()
            grads[dtype] = {n: p.grad.double().numpy() for n, p in m.named_parameters()}
        for n, v in R.model_grad_figures(grads[torch.float32], grads[torch.float64]).items():
            if n.endswith(R.SCORE_PATH):
                floor_qk = max(floor_qk, v)
            else:
                floor_rest = max(floor_rest, v)
    print("if4rec model floors (fp32 torch vs float64 on g14): score path %.2e, every other gradient %.2e" % (floor_qk, floor_rest))
    assert 4 * floor_rest < R.TOL
    assert floor_qk > R.TOL                             # which is why these four are not held to TOL
    assert 4 * floor_qk < R.MODEL_QK_TOL == 1e-3 and 8 * R.MODEL_QK_FLOOR == pytest.approx(R.MODEL_QK_TOL)


def test_initialisation_is_xavier_normal_and_names_are_the_references():
    from whisprrec_amd.if4rec import IF4Rec
    torch.manual_seed(5)
    m = IF4Rec(_args(), host.Corpus(40, 300, {}))
    W = m.i_embeddings.weight.detach()
    std = float(np.sqrt(2.0 / (300 + 64)))
    assert W.shape == (300, 64) and abs(float(W.std()) - std) < 0.05 * std and float(W.abs().max()) > 3 * std   # normal, not uniform
    assert m.i_embeddings.padding_idx == -1
    assert all(float(b.detach().abs().max()) == 0.0 for n, b in m.named_parameters() if n.endswith("bias") and "layer_norm" not in n)
    names = list(m.state_dict().keys())
    assert names[:6] == ["i_embeddings.weight", "p_embeddings.weight", "W1.weight", "W1.bias", "W2.weight", "W2.bias"]
    assert "transformer_block.0.masked_attn_head.q_linear.weight" in names and m.p_embeddings.weight.shape == (21, 64)
    assert not hasattr(m, "eval_queries") and not getattr(m, "per_sample_feed", False)
    assert IF4Rec.extra_log_args == ["emb_size", "attn_size", "K", "encoder_layer", "n_head", "encoder_dropout", "add_pos", "add_multi"]


def test_launcher_knows_the_model_and_its_flags():
    from whisprrec_amd import main as launcher
    args, model_cls, reader_cls, _ = launcher.build_args(["--model_name", "IF4Rec", "--interest_native", "1", "--block_native", "1",
                                                          "--K", "4"])
    assert model_cls.__name__ == "IF4Rec" and reader_cls.__name__ == "SeqReader"
    assert args.interest_native == 1 and args.block_native == 1 and args.K == 4
    args = launcher.build_args(["--model_name", "IF4Rec"])[0]
    assert args.interest_native == 0 and args.block_native == 0
    assert (args.emb_size, args.attn_size, args.K, args.add_pos, args.encoder_layer, args.n_head, args.encoder_dropout,
            args.add_multi) == (64, 8, 2, 1, 1, 8, 0.1, 1)


# ------------------------------------------------------------------------------------------------ the C-ABI
def _lib():
    from whisprrec_amd import abi
    assert os.path.exists(abi.LIB_PATH), "run __graft_entry__.build() first"    # a missing library is a failed build, not a skip
    return abi, abi.lib()


def test_new_entries_are_bound_with_the_documented_argument_counts():
    from whisprrec_amd import abi
    want = {"wr_interest_pool_supported": 4, "wr_interest_pool_workspace_bytes": 5, "wr_interest_pool_fwd": 17,
            "wr_interest_pool_bwd": 25, "wr_rank_eval_multi_supported": 2, "wr_rank_eval_multi": 15}
    raw = ctypes.CDLL(abi.LIB_PATH)
    for name, n in want.items():
        assert len(abi.SIGNATURES[name][1]) == n and hasattr(raw, name), name
    assert len(abi.SIGNATURES["wr_rank_eval_multi"][1]) == len(abi.SIGNATURES["wr_rank_eval_rows"][1])   # KQ in, query_row out


def test_supported_sets_are_as_documented():
    abi, L = _lib()
    for D in (16, 32, 48, 64, 128, 256):
        for A in (0, 1, 8, 32, 33):
            for K in (0, 1, 2, 3, 8, 9):
                for T in (0, 1, 20, 64, 65):
                    want = D in (32, 64, 128) and 1 <= A <= 32 and 1 <= K <= 8 and 1 <= T <= 64
                    assert L.wr_interest_pool_supported(D, A, K, T) == int(want), (D, A, K, T)
    assert L.wr_interest_pool_workspace_bytes(2048, 64, 8, 2, 20) == 512 * (64 * 8 + 8 + 2 * 8 + 2 + 20 * 64) * 4
    assert L.wr_interest_pool_workspace_bytes(2048, 64, 8, 9, 20) == -5 and "K=9" in abi.last_error()
    assert L.wr_interest_pool_workspace_bytes(0, 64, 8, 2, 20) == -5
    from whisprrec_amd import hip_ops
    for D in (4, 8, 24, 64, 128, 252, 256, 6):
        for KQ in (0, 1, 2, 3, 4, 8):
            want = hip_ops.rank_eval_supports(D) and KQ in (1, 2, 4)
            assert L.wr_rank_eval_multi_supported(D, KQ) == int(want), (D, KQ)
            assert hip_ops.rank_eval_multi_supports(D, KQ) == bool(want)


def test_argument_errors_are_reported_before_any_launch():
    """no GPU here: every one of these returns before a launch"""
    abi, L = _lib()
    buf = (ctypes.c_float * 4096)()
    a16 = (ctypes.addressof(buf) + 15) // 16 * 16

    def fwd(item=a16, pos=a16, n_pos=21, D=64, hist=a16, B=4, T=20, W1=a16, A=8, K=2, out=a16):
        return L.wr_interest_pool_fwd(item, 300, pos, n_pos, D, hist, B, T, W1, a16, a16, a16, A, K, out, None, None)

    def bwd(item=a16, pos=a16, n_pos=21, D=64, hist=a16, B=4, T=20, W1=a16, A=8, K=2, out=a16, gpos=a16, ws=a16, ws_bytes=1 << 40):
        return L.wr_interest_pool_bwd(item, 300, pos, n_pos, D, hist, B, T, W1, a16, a16, a16, A, K, a16, out, a16, a16, a16, a16,
                                      gpos, None, ws, ws_bytes, None)

    for call in (fwd, bwd):
        assert call(item=None) == -1 and "NULL" in abi.last_error()
        assert call(hist=None) == -1 and call(W1=None) == -1 and call(out=None) == -1
        assert call(D=48) == -5 and "D=48" in abi.last_error()
        assert call(K=9) == -5 and call(K=0) == -5 and call(T=65) == -5 and call(A=33) == -5
        assert call(B=0) == -2 and call(n_pos=19) == -2 and call(item=a16 + 4) == -4 and call(pos=a16 + 4) == -4
    assert bwd(ws_bytes=1024) == -3 and bwd(ws=None) == -3
    assert bwd(gpos=None) == -1 and bwd(pos=None, n_pos=0) == -1 and "gpos goes with pos_tab" in abi.last_error()
    assert bwd(pos=None, n_pos=0, gpos=None, ws_bytes=1024) == -3 and "wr_interest_pool_bwd" in abi.last_error()

    def multi(Q=a16, nq=8, I=a16, n_items=10, D=64, KQ=2, et=a16, n=4, mrow=a16, ptr=a16, idx=a16, rank=a16, tsc=a16):
        return L.wr_rank_eval_multi(Q, nq, I, n_items, D, KQ, et, n, mrow, 5, ptr, idx, rank, tsc, None)

    assert multi(KQ=3) == -5 and "KQ=3" in abi.last_error()
    assert multi(KQ=8) == -5 and multi(KQ=0) == -5
    assert multi(Q=None) == -1 and multi(I=None) == -1 and multi(et=None) == -1 and multi(rank=None) == -1 and multi(tsc=None) == -1
    assert multi(D=256) == -5 and "D <= 252" in abi.last_error()
    assert multi(D=6) == -2 and multi(nq=7) == -2 and multi(n=-1) == -2
    assert multi(mrow=None) == -1 and multi(ptr=None) == -1 and "go together" in abi.last_error()
    assert multi(n=0) == 0


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from whisprrec_amd import abi, hip_ops
    item, pos = torch.zeros(30, 64), torch.zeros(21, 64)
    W1, b1, W2, b2 = torch.zeros(8, 64), torch.zeros(8), torch.zeros(2, 8), torch.zeros(2)
    hist = torch.ones(4, 20, dtype=torch.int64)
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.interest_pool_fwd(item, pos, hist, W1, b1, W2, b2)
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.interest_pool(item, pos, hist, W1, b1, W2, b2)
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.interest_pool_bwd(item, pos, hist, W1, b1, W2, b2, torch.zeros(4, 2, 64))
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.rank_eval_multi(torch.zeros(4, 2, 64), item, torch.zeros(4, dtype=torch.int64))
    assert hip_ops.interest_pool_supports(64, 8, 2, 20) and not hip_ops.interest_pool_supports(64, 8, 2, 65)


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


def _runner_and_dataset(K):
    from test_seq_eval_contract import _seq_corpus
    from whisprrec_amd import main as launcher, runner
    ds = host.SequentialModel.Dataset(_Interests(K), _seq_corpus(), "dev")
    args = launcher.build_args(["--model_name", "IF4Rec", "--runner_name", "HipRunner", "--seq_eval_native", "1"])[0]
    return runner.HipRunner(args), ds


def test_runner_accepts_a_model_with_the_interest_protocol():
    for K in (1, 2, 4):
        rn, ds = _runner_and_dataset(K)
        assert rn._seq_eval_ok(ds)


def test_runner_falls_back_with_one_warning_for_three_interests(caplog):
    rn, ds = _runner_and_dataset(3)
    with caplog.at_level(logging.WARNING):
        assert not rn._seq_eval_ok(ds) and not rn._seq_eval_ok(ds)
    msgs = [r.getMessage() for r in caplog.records if "seq_eval_native" in r.getMessage()]
    assert len(msgs) == 1 and "3 interests" in msgs[0]


def test_top_k_over_several_interests_is_refused_by_name():
    rn, ds = _runner_and_dataset(2)
    for call in (lambda: rn.recommend_rows(ds, 5), lambda: rn.recommend(ds.model, ds.corpus, [0, 1], 5),
                 lambda: rn.recommend_next(ds.model, ds.corpus, [[1, 2]], 5), lambda: rn.save_rec_results(ds, 5, "/tmp/never.csv")):
        with pytest.raises(NotImplementedError, match="top-K over several interests"):
            call()
