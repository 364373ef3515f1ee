"""CPU checks around ContraRec: the float64 restatements the GPU tests compare against (length-masked block, supervised
contrastive loss with its closed-form gradient) equal float64 torch autograd; the augmentations consume NumPy's global stream as
the reference does; the torch-path model reproduces the reference's losses, gradients and a 5-step Adam curve (g12); the
tolerances stand above the fp32 floor of the stock path and deliberately wrong variants land above them; and the new entry points
refuse bad arguments before any launch."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrarec_ref as C  # noqa: E402
import sasblock_ref as R  # noqa: E402
from conftest import rel_err  # noqa: E402
from whisprrec_amd import host  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_contrarec.npz")


@pytest.fixture(scope="module")
def g12():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def block_cases(g12):
    return [C.make_block_case(i, g12) for i in range(len(C.BLOCK_SHAPES))]


@pytest.fixture(scope="module")
def loss_cases():
    return [C.make_loss_case(i) for i in range(len(C.LOSS_SHAPES))]


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("i", range(len(C.BLOCK_SHAPES)))
def test_block_restatement_equals_the_block_in_float64_under_autograd(block_cases, i):
    x, sd, g, heads, lens = block_cases[i]
    ref = C.block_keys_f64(x, sd, heads, lens, g)
    fig = C.figures(*C.stock_block_fp32(x, sd, heads, g, lens, dtype=torch.float64), ref)
    assert max(fig.values()) <= 1e-12, fig


def _reference_formula_f64(F, labels, tau):
    """ContraLoss.forward (ContraRec.py:148-204) typed again, in float64 under autograd, the in-place sub_ included"""
    Ft = torch.as_tensor(F, dtype=torch.float64).clone().requires_grad_(True)
    B = Ft.shape[0] // 2
    features = torch.nn.functional.normalize(torch.stack([Ft[:B], Ft[B:]], dim=1), dim=-1)
    lab = torch.as_tensor(labels).contiguous().view(-1, 1)
    mask = torch.eq(lab, lab.transpose(0, 1)).double()
    contrast = torch.cat(torch.unbind(features, dim=1), dim=0)
    adc = torch.matmul(contrast, contrast.transpose(0, 1)) / tau
    logits_max, _ = torch.max(adc, dim=1, keepdim=True)
    adc.sub_(logits_max)
    logits = adc - logits_max.detach()
    mask = mask.repeat(2, 2)
    logits_mask = torch.scatter(torch.ones_like(mask), 1, torch.arange(2 * B).view(-1, 1), 0)
    mask = mask * logits_mask
    exp_logits = torch.exp(logits) * logits_mask
    log_prob = logits - torch.log(exp_logits.sum(1, keepdim=True) + 1e-10)
    loss = (-tau * (mask * log_prob).sum(1) / (mask.sum(1) + 1e-10)).mean()
    loss.backward()
    return float(loss.detach()), Ft.grad.numpy()


@pytest.mark.parametrize("i", range(len(C.LOSS_SHAPES)))
def test_loss_restatement_equals_the_reference_formula_in_float64_under_autograd(loss_cases, i):
    F, labels, tau = loss_cases[i]
    ref = C.supcon_f64(F, labels, tau)
    fig = C.loss_figures(*_reference_formula_f64(F, labels, tau), ref)
    assert max(fig.values()) <= 1e-9, fig
    fig = C.loss_figures(*C.stock_loss_fp32(F, labels, tau, dtype=torch.float64), ref)      # the model's torch path
    assert max(fig.values()) <= 1e-9, fig
    w = C.supcon_f64(F, labels, tau, weight=0.37)
    assert abs(w[0] - 0.37 * ref[0]) <= 1e-14 * abs(ref[0]) and rel_err(w[1], 0.37 * ref[1]) <= 1e-14


# ------------------------------------------------------------------------------------------------ floors and power
def test_block_tolerances_stand_above_the_fp32_floor(block_cases):
    worst = {k: 0.0 for k in C.BLOCK_TOL}
    for i, (x, sd, g, heads, lens) in enumerate(block_cases):
        fig = C.figures(*C.stock_block_fp32(x, sd, heads, g, lens), C.block_keys_f64(x, sd, heads, lens, g))
        print(C.block_fmt("floor B=%d T=%d D=%d h=%d" % C.BLOCK_SHAPES[i], fig))
        for k, v in C.worst(fig).items():
            worst[k] = max(worst[k], v)
    print("floor (largest): " + " ".join("%s %.2e" % kv for kv in worst.items()))
    for k in C.BLOCK_TOL:
        assert 4.0 * worst[k] < C.BLOCK_TOL[k], (k, worst[k])
        assert 8.0 * C.BLOCK_FLOORS[k] <= C.BLOCK_TOL[k] <= 16.0 * C.BLOCK_FLOORS[k]


def test_loss_tolerances_stand_above_the_fp32_floor(loss_cases):
    worst = {k: 0.0 for k in C.LOSS_TOL}
    for i, (F, labels, tau) in enumerate(loss_cases):
        fig = C.loss_figures(*C.stock_loss_fp32(F, labels, tau), C.supcon_f64(F, labels, tau))
        print(C.loss_fmt("floor B=%d D=%d tau=%g labels=%d" % C.LOSS_SHAPES[i], fig))
        for k in worst:
            worst[k] = max(worst[k], fig[k])
    for k in C.LOSS_TOL:
        assert 4.0 * worst[k] < C.LOSS_TOL[k], (k, worst[k])
        assert 8.0 * C.LOSS_FLOORS[k] <= C.LOSS_TOL[k] <= 16.0 * C.LOSS_FLOORS[k]


@pytest.mark.parametrize("wrong", C.BLOCK_WRONG)
def test_wrong_masks_land_above_the_tolerances(block_cases, wrong):
    """the causal mask, no mask, padded queries skipped: each exceeds 4 x TOL on a case with lengths below T"""
    caught = []
    for i, (x, sd, g, heads, lens) in enumerate(block_cases):
        if not (lens < C.BLOCK_SHAPES[i][1]).any():
            continue
        ref = C.block_keys_f64(x, sd, heads, lens, g)
        bad = C.block_keys_f64(x, sd, heads, lens, g, wrong=wrong)
        fig = C.figures(bad["out"], bad["gx"], bad["g"], ref)
        if any(v > 4.0 * C.BLOCK_TOL[C.group_of(n)] for n, v in fig.items()):
            caught.append(i)
    assert caught, wrong


# ------------------------------------------------------------------------------------------------ several visits, every form
SEED = 0x5A5B10C
LISTS = {"walk": (C.BLOCK_WALK_SHAPES, C.BLOCK_WALK_SEED, C.BLOCK_WALK_FLOORS, C.BLOCK_WALK_TOL),
         "form": (C.BLOCK_FORM_SHAPES, C.BLOCK_FORM_SEED, C.BLOCK_FORM_FLOORS, C.BLOCK_FORM_TOL)}
_LIST_REFS = {}


def _list_ref(which, i, p):
    """(inputs, masks, float64 result) of a case of BLOCK_WALK_SHAPES / BLOCK_FORM_SHAPES, computed once"""
    if (which, i, p) not in _LIST_REFS:
        shapes, seed = LISTS[which][:2]
        x, sd, g, heads, lens = C.make_block_case(i, shapes=shapes, seed=seed)
        m1, m2 = R.masks_for(SEED + seed + i, *x.shape, p)
        _LIST_REFS[(which, i, p)] = ((x, sd, g, heads, lens), (m1, m2), C.block_keys_f64(x, sd, heads, lens, g, m1=m1, m2=m2))
    return _LIST_REFS[(which, i, p)]


def test_block_walk_lengths_and_the_old_cases(block_cases):
    """the keyed lists are sasblock_ref's (tests/test_sasblock_contract.py checks that they walk); every case forces the lengths 1
    and T; the lengths met on a later visit are independent of those of the visit before; BLOCK_SHAPES' data is what it was"""
    assert C.BLOCK_WALK_SHAPES is R.WALK_SHAPES and C.BLOCK_FORM_SHAPES is R.FORM_SHAPES
    G = R.BWD_WG
    for which in ("walk", "form"):
        for i, (B, T, _, _) in enumerate(LISTS[which][0]):
            lens = _list_ref(which, i, 0.0)[0][4]
            assert lens.min() == 1 and lens.max() == T and lens.shape == (B,)
            if which == "walk":
                assert B > G and (lens[G:] != lens[:B - G]).any()
                if T >= 5 and B - G >= 500:     # enough pairs to tell: equal by chance in 1 of T, not in all
                    assert (lens[G:] == lens[:B - G]).mean() < 2.0 / T + 0.1
    x, sd, g, heads, lens = block_cases[2]
    rng = np.random.RandomState(7302)
    R.xavier_params(32, 2, rng)
    assert np.array_equal(x, (rng.standard_normal((5, 7, 32)) * np.sqrt(2.0 / (3706 + 32)) * np.sqrt(2.0)).astype(np.float32))
    assert np.array_equal(lens, C.make_lengths(5, 7, rng))


@pytest.mark.parametrize("which", ["walk", "form"])
def test_block_walk_and_form_tolerances_stand_above_the_fp32_floor(which):
    shapes, seed, floors, tol = LISTS[which]
    worst = {k: 0.0 for k in tol}
    for i in range(len(shapes)):
        for p in (0.0, 0.1):
            (x, sd, g, heads, lens), (m1, m2), ref = _list_ref(which, i, p)
            fig = C.figures(*C.stock_block_fp32(x, sd, heads, g, lens, m1=m1, m2=m2), ref)
            print(C.block_fmt("%s floor B=%d T=%d D=%d h=%d p=%g" % (which, *shapes[i], p), fig, tol))
            for k, v in C.worst(fig).items():
                worst[k] = max(worst[k], v)
            if p == 0.1:                      # the restatement with its masks, in float64 under autograd
                f64 = C.figures(*C.stock_block_fp32(x, sd, heads, g, lens, dtype=torch.float64, m1=m1, m2=m2), ref)
                assert max(f64.values()) <= 1e-12, f64
    print("%s floor (largest): " % which + " ".join("%s %.2e" % kv for kv in worst.items()))
    for k in tol:
        assert 4.0 * worst[k] < tol[k], (k, worst[k], tol[k])
        assert 8.0 * floors[k] <= tol[k] <= 16.0 * floors[k] and tol[k] == R.rule_of(floors[k])
        assert R.rule_of(C.BLOCK_FLOORS[k]) == C.BLOCK_TOL[k]


BLOCK_WALK_WRONG = ["later_visits_dropped", "later_visits_stale", "mask_of_first_visit", "length_of_first_visit"]


@pytest.mark.parametrize("wrong", BLOCK_WALK_WRONG)
@pytest.mark.parametrize("i", range(len(C.BLOCK_WALK_SHAPES)))
def test_block_walk_mutants_land_five_tolerances_out(i, wrong):
    """parameter gradients of the first visits only; a later visit's output and gx those of the visit before; its dropout mask, or
    its key length, that of the visit before — each exceeds 5 x BLOCK_WALK_TOL on some figure, at every walk shape"""
    (x, sd, g, heads, lens), (m1, m2), ref = _list_ref("walk", i, 0.1)
    src = R.first_visit_of(x.shape[0], R.BWD_WG)
    if wrong == "later_visits_dropped":
        bad = C.block_keys_f64(x, sd, heads, lens, g, wrong=wrong, m1=m1, m2=m2, first=R.BWD_WG)
    elif wrong == "later_visits_stale":
        bad = R.stale(ref, R.BWD_WG)
    elif wrong == "mask_of_first_visit":
        bad = C.block_keys_f64(x, sd, heads, lens, g, m1=m1[src], m2=m2[src])
    else:
        bad = C.block_keys_f64(x, sd, heads, lens[src], g, m1=m1, m2=m2)
    fig = C.figures(bad["out"], bad["gx"], bad["g"], ref)
    margin = {n: v / C.BLOCK_WALK_TOL[C.group_of(n)] for n, v in fig.items()}
    print("walk mutant %s at %s: largest figure / tolerance %.1f (%s)" % (wrong, C.BLOCK_WALK_SHAPES[i], max(margin.values()),
                                                                           max(margin, key=margin.get)))
    assert max(margin.values()) >= 5.0, margin


def test_block_walk_maximum_of_the_first_visits_only_misses_the_stored_maximum():
    """`max_of_first_visit` on the GPU test's case: x of sequence 2049 of (2051, 2, 64, 4) times 100"""
    i = C.BLOCK_WALK_SHAPES.index((2051, 2, 64, 4))
    x, sd, g, heads, lens = C.make_block_case(i, shapes=C.BLOCK_WALK_SHAPES, seed=C.BLOCK_WALK_SEED)
    x = x.copy()
    x[2049] *= 100.0
    ref = C.block_keys_f64(x, sd, heads, lens)
    bad = ref["seq_max"][:R.FWD_WG].max()
    assert ref["gmax"] == ref["seq_max"].max() and 10.0 < ref["gmax"] - bad < 30.0
    assert abs(bad - ref["gmax"]) > 5.0 * 1e-5 * abs(ref["gmax"])


@pytest.mark.parametrize("wrong", C.LOSS_WRONG)
def test_wrong_losses_land_above_the_tolerances(loss_cases, wrong):
    """each variant exceeds 4 x TOL on a listed shape; the single shift and the missing 1e-10 on a tau = 0.05 one"""
    caught = []
    for i, (F, labels, tau) in enumerate(loss_cases):
        fig = C.loss_figures(*C.supcon_f64(F, labels, tau, wrong=wrong), C.supcon_f64(F, labels, tau))
        if any(fig[k] > 4.0 * C.LOSS_TOL[k] for k in fig):
            caught.append(i)
    assert caught, wrong
    if wrong in ("single_shift", "no_eps"):
        assert any(C.LOSS_SHAPES[i][2] == 0.05 for i in caught), caught


# ------------------------------------------------------------------------------------------------ the model against g12
def _args(**kw):
    base = dict(device="cpu", model_path="/tmp/wr_contrarec.pt", buffer=1, num_neg=1, test_all=1, history_max=20, emb_size=64,
                gamma=0.5, beta_a=3, beta_b=3, ccc_temp=0.2)
    base.update(kw)
    return argparse.Namespace(**base)


def _cpu_model(g12):
    """the torch-path model on the CPU: the row gather of HipEmbedding (K9, tested on its own) replaced by nn.Embedding"""
    from whisprrec_amd.contrarec import ContraRec
    m = ContraRec(_args(), host.Corpus(40, 300, {}))
    assert list(m.state_dict().keys()) == [str(n) for n in g12["names"]]
    m.load_state_dict({str(n): torch.from_numpy(g12["sd__" + str(n)]) for n in g12["names"]})
    emb = torch.nn.Embedding(301, 64)
    emb.weight = m.item_embeddings.weight
    m.item_embeddings = emb
    return m


def _feed(g12):
    t = {k: torch.from_numpy(g12[k]) for k in ("hist", "hist_a", "hist_b", "lengths", "pos", "neg")}
    return {"history_items": t["hist"], "history_items_a": t["hist_a"], "history_items_b": t["hist_b"], "lengths": t["lengths"],
            "pos_item": t["pos"], "neg_items": t["neg"], "phase": "train", "batch_size": 96}


def test_g12_batch_covers_the_lengths(g12):
    lens = g12["lengths"]
    assert lens.min() == 1 and lens.max() == 20 and len(np.unique(lens)) > 10
    assert g12["hist"].shape == g12["hist_a"].shape == g12["hist_b"].shape == (96, 20)
    assert (g12["hist_a"] == 300).any()                                     # the mask token reaches the embedding's last row


def test_torch_path_model_reproduces_the_reference(g12):
    m = _cpu_model(g12)
    m.train()
    loss = m.predict(_feed(g12))
    loss.backward()
    ctc, ccc = (float(v) for v in m.last_losses)
    assert abs(ctc - float(g12["ctc"][0])) <= 2e-6 * abs(float(g12["ctc"][0]))
    assert abs(ccc - float(g12["ccc"][0])) <= 2e-6 * abs(float(g12["ccc"][0]))
    assert abs(float(loss.detach()) - float(g12["loss"][0])) <= 2e-6 * abs(float(g12["loss"][0]))
    for n, p in m.named_parameters():
        ref = g12["g__" + n]
        assert rel_err(p.grad.numpy(), ref) <= 2e-5, n                      # same ops as the reference, in another order
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    curve = []
    for _ in range(5):
        opt.zero_grad()
        step_loss = m.predict(_feed(g12))
        step_loss.backward()
        opt.step()
        curve.append(float(step_loss.detach()))
    assert np.abs(np.asarray(curve) - g12["adam_losses"]).max() <= 1e-5 * np.abs(g12["adam_losses"]).max()


def test_initialisation_is_xavier_uniform():
    from whisprrec_amd.contrarec import ContraRec
    torch.manual_seed(5)
    m = ContraRec(_args(), host.Corpus(40, 300, {}))
    W = m.item_embeddings.weight.detach()
    bound = float(np.sqrt(6.0 / (301 + 64)))
    assert W.shape == (301, 64) and float(W.abs().max()) <= bound and float(W.abs().max()) > 0.95 * bound
    assert abs(float(W.std()) - bound / np.sqrt(3.0)) < 0.05 * bound            # uniform, not normal
    assert all(float(b.detach().abs().max()) == 0.0 for n, b in m.named_parameters() if n.endswith("linear.bias"))
    assert m.item_embeddings.padding_idx == -1 and m.mask_token == 300


def test_augmentations_consume_the_global_stream_as_the_reference(g12):
    from whisprrec_amd.contrarec import ContraRec
    m = ContraRec(_args(), host.Corpus(40, 300, {}))
    ds = ContraRec.Dataset.__new__(ContraRec.Dataset)
    ds.model = m
    np.random.seed(2023)
    for seq, n, want in zip(g12["aug_in"], g12["aug_len"], g12["aug_out"]):
        got = ds.augment(seq[:n])
        assert np.array_equal(got, want[:n])


def test_feed_dict_adds_the_views_in_training_only():
    from whisprrec_amd.contrarec import ContraRec
    m = ContraRec(_args(test_all=0), host.Corpus(3, 300, {}))
    corpus = host.Corpus(3, 300, {ph: {"user_id": np.array([1, 1]), "item_id": np.array([5, 6]), "position": np.array([1, 2]),
                                       "neg_items": np.array([[7], [8]])} for ph in ("train", "dev")})
    corpus.user_his = {1: [(4, 0), (5, 1), (6, 2)]}
    tr, dv = ContraRec.Dataset(m, corpus, "train"), ContraRec.Dataset(m, corpus, "dev")
    np.random.seed(1)
    fd = tr[1]
    assert set(fd["history_items_a"]) <= {4, 5, 300} and len(fd["history_items_b"]) == 2
    assert "history_items_a" not in dv[1]


# ------------------------------------------------------------------------------------------------ interface
def _lib():
    from whisprrec_amd import abi
    assert os.path.exists(abi.LIB_PATH), "run __graft_entry__.build() first"    # a missing library is a failed build, not a skip
    return abi, abi.lib()


def test_launcher_knows_the_model_and_its_flags():
    from whisprrec_amd import main as launcher
    args, model_cls, reader_cls, _ = launcher.build_args(["--model_name", "ContraRec", "--block_native", "1", "--ccc_native", "1",
                                                          "--ccc_temp", "0.3"])
    assert model_cls.__name__ == "ContraRec" and reader_cls.__name__ == "SeqReader"
    assert args.block_native == 1 and args.ccc_native == 1 and args.ccc_temp == 0.3 and args.gamma == 1
    args = launcher.build_args(["--model_name", "ContraRec"])[0]
    assert args.block_native == 0 and args.ccc_native == 0


def test_supcon_supported_set_and_workspace():
    abi, L = _lib()
    assert [L.wr_supcon_supported(D) for D in (32, 64, 128, 16, 48, 256)] == [1, 1, 1, 0, 0, 0]
    for D in (32, 64, 128):
        for B in (1, 3, 64, 65, 256, 2048, 16384):
            nb = L.wr_supcon_workspace_bytes(B, D)
            assert nb > 0
            assert nb < 3 * (2 * B) ** 2 * 4 or B <= 256                    # below the torch path's three [2B, 2B] temporaries
    assert L.wr_supcon_workspace_bytes(16385, 64) == -2 and "B=16385" in abi.last_error()
    assert L.wr_supcon_workspace_bytes(0, 64) == -2
    assert L.wr_supcon_workspace_bytes(64, 48) == -5 and "D=48" in abi.last_error()


def test_argument_errors_are_reported_before_any_launch():
    """no GPU here: every one of these returns before a launch"""
    abi, L = _lib()
    buf = (ctypes.c_float * 4096)()
    a16 = (ctypes.addressof(buf) + 15) // 16 * 16

    def sup(F=a16, B=4, D=64, labels=a16, tau=0.2, loss=a16, gF=a16, ws=a16, ws_bytes=1 << 40):
        return L.wr_supcon_loss_grad(F, B, D, labels, tau, loss, 0, 1.0, gF, None, ws, ws_bytes, None)

    assert sup(D=48) == -5 and "D=48" in abi.last_error()
    assert sup(B=0) == -2 and sup(B=1 << 15) == -2
    assert sup(F=None) == -1 and sup(labels=None) == -1 and sup(loss=None) == -1
    assert sup(F=a16 + 4) == -4 and sup(gF=a16 + 4) == -4
    assert sup(tau=0.0) == -5 and sup(tau=float("nan")) == -5 and "tau" in abi.last_error()
    assert sup(ws_bytes=1024) == -3 and sup(ws=None) == -3

    ptrs = (ctypes.c_void_p * 14)(*([a16] * 14))
    pp = ctypes.addressof(ptrs)

    def fwd(x=a16, B=4, T=20, D=64, h=2, params=pp, out=a16, ws_bytes=1 << 40, key_len=a16):
        return L.wr_sasblock_fwd_keys(x, B, T, D, D, h, params, 0.0, 1, 0, out, a16, a16, ws_bytes, None, key_len, None)

    def bwd(x=a16, B=4, T=20, D=64, h=2, params=pp, out=a16, ws_bytes=1 << 40, key_len=a16):
        return L.wr_sasblock_bwd_keys(x, a16, B, T, D, D, h, params, 0.0, 1, 0, a16, out, a16, a16, ws_bytes, None, key_len, None)

    for call in (fwd, bwd):
        assert call(key_len=None) == -1 and "NULL" in abi.last_error()
        assert call(D=48) == -5 and call(T=65) == -5 and call(h=8) == -5
        assert call(B=0) == -2 and call(x=None) == -1 and call(params=None) == -1
        assert call(x=a16 + 4) == -4 and call(ws_bytes=1024) == -3
    assert "wr_sasblock_bwd_keys" in abi.last_error()


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from whisprrec_amd import abi, hip_ops
    from whisprrec_amd.sasrec import _Block
    blk = _Block(64, 64, 2, 0.0)
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.sasrec_block(torch.zeros(2, 20, 64), blk, 2, 0.0, 0, False, key_lengths=torch.tensor([3, 20]))
    with pytest.raises(abi.WhisprRecHipError):
        hip_ops.supcon_loss_grad(torch.zeros(8, 64), torch.zeros(4, dtype=torch.int64), 0.2)
