"""CPU checks for NARM, the whole-sequence GRU (K27) and the attention pooling (K28): the float64 restatements of
tests/narm_ref.py against torch's own float64 autograd and against gru_ref, the flag-off model against the sort / pack / unsort
form and against the restatement, the tolerances against the fp32 floors, the power of the figures against deliberately wrong
results, and the interface (parser flags, MODELS, parameter names, --num_layers, C-ABI argument errors) — nothing here needs a
GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_ref as G  # noqa: E402
import narm_ref as R  # noqa: E402
from sasblock_ref import rule_of  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEQ_IDS = [R.seq_id(k) for k in R.SEQ_CASES]
POOL_IDS = [R.pool_id(k) for k in R.POOL_CASES]
_SEQ, _POOL = {}, {}


def _seq(key):
    if key not in _SEQ:
        c = R.make_seq_case(*key)
        _SEQ[key] = (c, {wl: R.seq_case_f64(c, wl) for wl in (False, True)})
    return _SEQ[key]


def _pool(key):
    if key not in _POOL:
        c = R.make_pool_case(*key)
        _POOL[key] = (c, R.pool_case_f64(c))
    return _POOL[key]


def _pad(c, T):
    return np.arange(T)[None, :] >= np.clip(c["lengths"], 0, T)[:, None]


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("key", R.SEQ_CASES[:-1], ids=SEQ_IDS[:-1])
def test_gru_seq_restatement_equals_torch_in_float64(key):
    c, ref = _seq(key)
    for with_last in (False, True):
        for n, v in R.seq_figures(R.seq_stock(c, with_last, torch.float64), ref[with_last]).items():
            assert v < 1e-12, (n, with_last, v)
    T = c["x"].shape[1]
    assert not ref[False]["hs"][_pad(c, T)].any() and not ref[False]["gx"][_pad(c, T)].any()
    if key[1] == "mixed" and key[0] > 0:
        assert _pad(c, T).any()


@pytest.mark.parametrize("key", [(2, "mixed", False), (4, "full", False), (1, "ones", False)], ids=lambda k: R.seq_id(k))
def test_gru_seq_restatement_ties_to_gru_ref(key):
    """the states before each row's length are gru_ref's; no g_hs and a g_last is gru_ref's backward; so is a g_hs that holds
    g_last at [b, len_b - 1] and nothing else"""
    c, _ = _seq(key)
    last = G.case_f64(c)
    B, T, _ = c["x"].shape
    live = ~_pad(c, T)
    zero = dict(c, ghs=np.zeros_like(c["ghs"]))
    a = R.seq_case_f64(zero, with_last=True)
    assert np.array_equal(a["hs"][live], last["hs"][live])
    assert np.array_equal(a["hs"][np.arange(B), c["lengths"] - 1], last["h"])
    only = np.zeros_like(c["ghs"])
    only[np.arange(B), c["lengths"] - 1] = c["glast"]
    b = R.seq_case_f64(dict(c, ghs=only))
    for n in ("gx", "gwih", "gwhh", "gbih", "gbhh"):
        assert R.rel_err(a[n], last[n]) < 1e-14 and R.rel_err(b[n], last[n]) < 1e-14, n


@pytest.mark.parametrize("key", R.POOL_CASES, ids=POOL_IDS)
def test_pool_restatement_equals_torch_in_float64(key):
    c, ref = _pool(key)
    for n, v in R.pool_figures(R.pool_stock(c, torch.float64), ref).items():
        assert v < 1e-12, (n, v)
    T = c["hs"].shape[1]
    assert not ref["ghs"][_pad(c, T)].any()
    if key[1] == "mixed" and key[0] > 0:
        assert _pad(c, T).any() and np.abs(c["hs"][_pad(c, T)]).max() > 0.5       # padded positions, and values in them


def test_restatements_ignore_the_padding_and_clamp_the_lengths():
    c, ref = _seq((2, "mixed", False))
    T = c["x"].shape[1]
    d = dict(c, x=c["x"].copy(), ghs=c["ghs"].copy())
    d["x"][_pad(c, T)] = np.nan
    d["ghs"][_pad(c, T)] = np.nan
    got = R.seq_case_f64(d, with_last=True)
    for n in R.SEQ_GROUP_OF:
        assert np.array_equal(got[n], ref[True][n]), n
    p, pref = _pool((2, "mixed"))
    T = p["hs"].shape[1]
    d = dict(p, hs=p["hs"].copy(), lengths=p["lengths"].copy())
    d["hs"][_pad(p, T)] = np.nan
    d["lengths"][1], d["lengths"][2] = 10_000, -3                         # above T acts as T (row 1 is T already); below 0 as 0
    got = R.pool_case_f64(d)
    assert np.array_equal(got["c"][1], pref["c"][1]) and not got["c"][2].any() and not got["ghs"][2].any() and not got["ghg"][2].any()
    keep = np.arange(len(p["lengths"])) != 2
    assert np.array_equal(got["c"][keep], pref["c"][keep])


# ------------------------------------------------------------------------------------------------ power
def test_wrong_gru_seq_variants_miss_the_tolerances():
    for wrong in R.SEQ_WRONGS:
        hit = False
        for key in ((2, "mixed", False), (4, "mixed", False)):
            c, ref = _seq(key)
            w = R.seq_worst(R.seq_figures(R.seq_case_f64(c, wrong=wrong), ref[False]))
            hit = hit or any(w[g] > R.SEQ_TOL[g] for g in R.SEQ_GROUPS)
        assert hit, wrong


def test_wrong_pool_variants_miss_the_tolerances():
    for wrong in R.POOL_WRONGS:
        hit = False
        for key in ((2, "mixed"), (3, "mixed")):
            c, ref = _pool(key)
            w = R.pool_worst(R.pool_figures(R.pool_case_f64(c, wrong=wrong), ref))
            hit = hit or any(w[g] > R.POOL_TOL[g] for g in R.POOL_GROUPS)
        assert hit, wrong


# ------------------------------------------------------------------------------------------------ floors
def test_tolerances_are_eight_floors():
    for floors, tol in ((R.SEQ_FLOORS, R.SEQ_TOL), (R.POOL_FLOORS, R.POOL_TOL), (R.MODEL_FLOORS, R.MODEL_TOL)):
        for g in floors:
            assert tol[g] == rule_of(floors[g]) and 8 * floors[g] <= tol[g] <= 16 * floors[g], g


@pytest.mark.parametrize("key", R.SEQ_CASES, ids=SEQ_IDS)
def test_gru_seq_floors_hold(key):
    floors, _ = R.measure_seq_floors([key])
    print("floor gru_seq %s: " % R.seq_id(key) + " ".join("%s %.2e" % (g, floors[g]) for g in R.SEQ_GROUPS))
    for g in R.SEQ_GROUPS:
        assert 4 * floors[g] < R.SEQ_TOL[g], (g, floors[g])


@pytest.mark.parametrize("key", R.POOL_CASES, ids=POOL_IDS)
def test_pool_floors_hold(key):
    floors, _ = R.measure_pool_floors([key])
    print("floor pool %s: " % R.pool_id(key) + " ".join("%s %.2e" % (g, floors[g]) for g in R.POOL_GROUPS))
    for g in R.POOL_GROUPS:
        assert 4 * floors[g] < R.POOL_TOL[g], (g, floors[g])


def test_shapes_reach_the_kernels_other_paths():
    import re
    import whisprrec_amd
    csrc = os.path.join(os.path.dirname(os.path.abspath(whisprrec_amd.__file__)), "csrc")
    with open(os.path.join(csrc, "wr_narm.hip")) as fh:
        src = fh.read()
    assert R.POOL_ROWS == 4 * int(re.search(r"constexpr int kNarmWg = (\d+);", src).group(1))
    assert sum(B > R.POOL_ROWS and T <= 3 for B, T, _, _ in R.POOL_SHAPES) == 1
    assert {A for *_, A in R.POOL_SHAPES} == {16, 32, 64} and {H for _, _, H, _ in R.POOL_SHAPES} == {32, 64}
    assert R.SEQ_WALK_SHAPE[0] > G.BWD_ROWS and R.SEQ_WALK_SHAPE[1] <= 5


# ------------------------------------------------------------------------------------------------ the model
def _argv(path, tmp, model="NARM", extra=()):
    return ["--emb_size", "64", "--hidden_size", "64", "--history_max", "20", "--model_name", model, "--runner_name",
            "HipRunner", "--dataset", "ml-100k", "--path", path, "--epoch", "1", "--batch_size", "1024", "--eval_batch_size", "512",
            "--optimizer", "Adam", "--lr", "1e-3", "--l2", "0.0", "--log_file", str(tmp / "log.txt"), "--model_path",
            str(tmp / "m.pt"), "--num_workers", "0", "--topk", "5,10", "--metric", "NDCG, HR", "--random_seed", "3407"] + list(extra)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from test_reader import _write_inter
    tmp = tmp_path_factory.mktemp("narm")
    return _write_inter(np.load(os.path.join(GOLD, "g8_reader.npz")), tmp), tmp


_CORPUS = {}


def _cpu_model(tiny, model="NARM", extra=()):
    from whisprrec_amd import main as launcher
    path, tmp = tiny
    args, model_class, reader_class, _ = launcher.build_args(_argv(path, tmp, model, extra))
    args.device = torch.device("cpu")
    if "corpus" not in _CORPUS:
        _CORPUS["corpus"] = reader_class(args).corpus()
    launcher.init_seed(args.random_seed)
    m = model_class(args, _CORPUS["corpus"])
    # the embedding lookup is a HIP kernel: on a CPU the rows are indexed, with the padding row's gradient dropped as it is there
    m.item_embedding.forward = lambda idx: torch.nn.functional.embedding(idx, m.item_embedding.weight, padding_idx=0)
    return m


def _scaled(m, dtype=torch.float32):
    m = m.to(dtype)
    with torch.no_grad():
        m.item_embedding.weight.mul_(8)          # a scale at which the gates leave their linear range
    return m


def _feed(batch):
    return {k: torch.from_numpy(v) for k, v in batch.items()}


def _loss_and_grads(m, batch):
    m.zero_grad()
    loss = m.predict(_feed(batch))
    loss.backward()
    return float(loss.detach()), {n: p.grad.detach().numpy().copy() for n, p in m.named_parameters()}


def _packed_forward(m, history, lengths):
    """ReChorus's form: sort by length, pack_padded_sequence, both encoders, unsort; the attention mask is history > 0"""
    x = torch.nn.functional.embedding(history, m.item_embedding.weight)
    sort_len, sort_idx = torch.topk(lengths, k=len(lengths))
    packed = torch.nn.utils.rnn.pack_padded_sequence(x.index_select(0, sort_idx), sort_len.cpu(), batch_first=True)
    _, hidden_g = m.encoder_g(packed, None)
    output_l, _ = m.encoder_l(packed, None)
    output_l, _ = torch.nn.utils.rnn.pad_packed_sequence(output_l, batch_first=True, total_length=history.shape[1])
    unsort_idx = torch.topk(sort_idx, k=len(lengths), largest=False)[1]
    h_g, hs_l = hidden_g[-1].index_select(0, unsort_idx), output_l.index_select(0, unsort_idx)
    e = m.attention_out(torch.sigmoid(m.A1(h_g)[:, None, :] + m.A2(hs_l)))
    e = torch.where((history > 0)[:, :, None], e, torch.zeros_like(e))
    return m.out(torch.cat(((e * hs_l).sum(1), h_g), dim=1))


def test_flag_off_forward_equals_the_sort_pack_unsort_form(tiny):
    m = _scaled(_cpu_model(tiny), torch.float64)
    batch = R.model_batch(m.item_num)
    fd = _feed(batch)
    with torch.no_grad():
        got, ref = m.forward(fd).numpy(), _packed_forward(m, fd["history_items"], fd["lengths"]).numpy()
    assert got.shape == (64, 64) and R.rel_err(got, ref) < 1e-12
    m = _scaled(_cpu_model(tiny))
    with torch.no_grad():
        got32, ref32 = m.forward(fd).numpy(), _packed_forward(m, fd["history_items"], fd["lengths"]).numpy()
    err = max(R.rel_err(got32, got), R.rel_err(ref32, got))
    print("flag-off forward and sort / pack / unsort forward in fp32 against float64: %.2e" % err)
    assert err < R.POOL_TOL["c"]                    # both at the fp32 floor


def _model_floor(tiny, dims, wrong=None):
    E, H, A = dims
    m = _scaled(_cpu_model(tiny, extra=["--emb_size", str(E), "--hidden_size", str(H), "--attention_size", str(A)]))
    batch = R.model_batch(m.item_num)
    loss, grads = _loss_and_grads(m, batch)
    sd = {n: v.detach().numpy() for n, v in m.state_dict().items()}
    ref_loss, ref_grads = R.narm_f64(sd, batch, wrong=wrong)
    assert set(grads) == set(ref_grads)
    return R.model_figures(loss, grads, ref_loss, ref_grads)


@pytest.mark.parametrize("dims", R.MODEL_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_flag_off_model_equals_the_restatement(tiny, dims):
    """loss and every parameter's gradient of the flag-off fp32 model against float64: the model's floor, a quarter of MODEL_TOL
    at the most"""
    w, per = _model_floor(tiny, dims)
    print(R.model_fmt("flag-off fp32 against float64 %s" % (dims,), w), {n: "%.1e" % v for n, v in per.items()})
    for g in R.MODEL_GROUPS:
        assert 4 * w[g] < R.MODEL_TOL[g], (g, w[g], per)


def test_model_figures_see_a_wrong_pooling_gradient(tiny):
    w, per = _model_floor(tiny, R.MODEL_DIMS[0], wrong="no_sigma_prime")
    assert w["grad"] > R.MODEL_TOL["grad"], per


def test_model_is_registered_with_the_stated_parameters(tiny, tmp_path):
    from whisprrec_amd import main as launcher, narm
    assert launcher.MODELS["NARM"] is narm.NARM and narm.bind(narm.host.SequentialModel).__qualname__ == "NARM"
    args, model_class, reader_class, _ = launcher.build_args(
        ["--model_name", "NARM", "--dataset", "ml-100k", "--path", "x/", "--log_file", str(tmp_path / "l.txt"), "--model_path",
         str(tmp_path / "m.pt")])
    assert model_class is narm.NARM and reader_class.__name__ == "SeqReader" and model_class.runner == "BaseRunner"
    assert (args.emb_size, args.hidden_size, args.attention_size, args.gru_native, args.pool_native, args.emb_lazy, args.train_loss) \
        == (64, 64, 16, 0, 0, 0, "bpr")
    with pytest.raises(SystemExit):
        launcher.build_args(_argv("x/", tmp_path, extra=["--pool_native", "2"]))
    m = _cpu_model(tiny, extra=["--emb_size", "32", "--attention_size", "32"])
    E, H, A = 32, 64, 32
    gru = lambda p: {p + ".weight_ih_l0": (3 * H, E), p + ".weight_hh_l0": (3 * H, H), p + ".bias_ih_l0": (3 * H,),      # noqa: E731
                     p + ".bias_hh_l0": (3 * H,)}
    want = {"item_embedding.weight": (m.item_num, E), "A1.weight": (A, H), "A2.weight": (A, H), "attention_out.weight": (1, A),
            "out.weight": (E, 2 * H)}
    want.update(gru("encoder_g"))
    want.update(gru("encoder_l"))
    assert {n: tuple(p.shape) for n, p in m.named_parameters()} == want
    assert m.gru_native is False and m.pool_native is False and m.train_loss == "bpr" and m.emb_lazy is False
    assert float(m.encoder_l.weight_hh_l0.detach().abs().max()) <= 1 / np.sqrt(H)     # nn.GRU's own initialisation
    assert m.eval_items() is m.item_embedding.weight


def test_num_layers_one_leaves_gru4rec_as_it_is(tiny, tmp_path):
    from whisprrec_amd import main as launcher
    args = launcher.build_args(["--model_name", "GRU4Rec", "--dataset", "ml-100k", "--path", "x/", "--log_file",
                                str(tmp_path / "l.txt"), "--model_path", str(tmp_path / "m.pt")])[0]
    assert (args.num_layers, args.emb_size, args.hidden_size, args.gru_native, args.emb_lazy, args.train_loss, args.softmax_native) \
        == (1, 64, 64, 0, 0, "bpr", 0)
    keys = ["item_embedding.weight", "rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0", "out.weight",
            "out.bias"]
    one = _cpu_model(tiny, "GRU4Rec")
    assert list(one.state_dict()) == keys and one.num_layers == 1
    explicit = _cpu_model(tiny, "GRU4Rec", ["--num_layers", "1"])
    assert all(torch.equal(a, b) for a, b in zip(one.state_dict().values(), explicit.state_dict().values()))
    two = _cpu_model(tiny, "GRU4Rec", ["--num_layers", "2", "--emb_size", "32"])
    assert list(two.state_dict()) == keys[:5] + ["rnn.weight_ih_l1", "rnn.weight_hh_l1", "rnn.bias_ih_l1", "rnn.bias_hh_l1"] + keys[5:]
    assert tuple(two.rnn.weight_ih_l1.shape) == (192, 64) and two.rnn.dropout == 0
    with pytest.raises(ValueError, match="num_layers"):
        _cpu_model(tiny, "GRU4Rec", ["--num_layers", "0"])
    # two layers on a CPU: the row at lengths - 1 of the stacked run is gru_ref's last state of the second layer over the first's
    batch = R.model_batch(two.item_num, B=9, T=6)
    with torch.no_grad():
        got = two.forward(_feed(batch)).numpy()
    sd = {n: v.detach().numpy() for n, v in two.state_dict().items()}
    p = lambda layer: [sd["rnn.%s_l%d" % (n, layer)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]      # noqa: E731
    hs0 = R.gru_seq_f64(sd["item_embedding.weight"][batch["history_items"]], batch["lengths"], *p(0))["hs"]
    ref = G.gru_f64(hs0, batch["lengths"], *p(1))["h"] @ sd["out.weight"].astype(np.float64).T + sd["out.bias"]
    assert R.rel_err(got, ref) < G.TOL["h"]


# ------------------------------------------------------------------------------------------------ the C interface
def test_c_abi_refuses_unsupported_shapes_with_the_numbers():
    from whisprrec_amd import abi
    L = abi.lib()
    for H in (32, 64):
        for A in (16, 32, 64):
            assert L.wr_narm_pool_supported(H, A, 1) == 1 and L.wr_narm_pool_supported(H, A, 100_000) == 1
    for H, A, T in ((128, 16, 20), (64, 8, 20), (64, 48, 20), (48, 16, 20), (64, 16, 0)):
        assert L.wr_narm_pool_supported(H, A, T) == 0, (H, A, T)
    assert L.wr_narm_pool_workspace_bytes(8, 20, 128, 16) == -5
    assert "H=128" in abi.last_error() and "A=16" in abi.last_error()
    # the bound is independent of B and T: 256 slabs of the parameter gradients
    assert L.wr_narm_pool_workspace_bytes(1, 1, 64, 16) == L.wr_narm_pool_workspace_bytes(1 << 20, 500, 64, 16) == \
        R.POOL_ROWS * (2 * 16 * 64 + 16) * 4
    keep = ctypes.create_string_buffer(96)                                  # nothing is dereferenced: every call is refused
    addr = (ctypes.addressof(keep) + 15) // 16 * 16
    rc = L.wr_narm_pool_fwd(addr, addr, addr, addr, addr, addr, 4, 20, 64, 48, addr, None)
    assert rc == -5 and "H=64" in abi.last_error() and "A=48" in abi.last_error()
    rc = L.wr_narm_pool_bwd(addr, addr, addr, addr, addr, addr, addr, 4, 20, 128, 16, addr, addr, addr, addr, addr, addr, 1 << 30, None)
    assert rc == -5 and "H=128" in abi.last_error()
    rc = L.wr_narm_pool_fwd(None, addr, addr, addr, addr, addr, 4, 20, 64, 16, addr, None)
    assert rc == -1 and "NULL" in abi.last_error()
    rc = L.wr_narm_pool_bwd(addr, addr, addr, addr, addr, addr, addr, 4, 20, 64, 16, addr, addr, addr, addr, addr, addr, 16, None)
    assert rc != 0 and "workspace" in abi.last_error()
    rc = L.wr_gru_seq_fwd(addr, addr, addr, addr, addr, addr, 4, 20, 64, 128, addr, None)
    assert rc == -5 and "wr_gru_seq_fwd" in abi.last_error() and "H=128" in abi.last_error()
    rc = L.wr_gru_seq_bwd(addr, addr, addr, addr, addr, addr, addr, addr, None, 4, 20, 128, 64, addr, addr, addr, addr, addr, addr,
                          1 << 30, None)
    assert rc == -5 and "E=128" in abi.last_error()
    rc = L.wr_gru_seq_bwd(addr, addr, addr, addr, addr, addr, addr, None, None, 4, 20, 64, 64, addr, addr, addr, addr, addr, addr,
                          1 << 30, None)
    assert rc == -1 and "NULL" in abi.last_error()                          # g_hs is required, g_last is not


def test_host_wrappers_refuse_cpu_tensors():
    from whisprrec_amd import abi, hip_ops
    c = R.make_seq_case(1, "mixed")
    t = {n: torch.from_numpy(v) for n, v in c.items()}
    with pytest.raises(abi.WhisprRecHipError, match="no CPU fallback"):
        hip_ops.gru_seq(t["x"], t["lengths"], t["wih"], t["whh"], t["bih"], t["bhh"])
    p = {n: torch.from_numpy(v) for n, v in R.make_pool_case(1, "mixed").items()}
    with pytest.raises(abi.WhisprRecHipError, match="no CPU fallback"):
        hip_ops.narm_pool(p["hs"], p["hg"], p["lengths"], p["A1"], p["A2"], p["v"])
