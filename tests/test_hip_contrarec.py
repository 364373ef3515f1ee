"""GPU checks of ContraRec's native paths: the block kernels with a key-length mask (wr_sasblock_fwd_keys / _bwd_keys) and the
supervised contrastive loss (wr_supcon_loss_grad) against the float64 restatements of tests/contrarec_ref.py, under its
tolerances; then the model with both flags against its own torch path, on the reference's batch (g12), over a 2-epoch launcher
run on the committed ml-100k file, and through the device evaluation.  Figures are printed as `parity ...` lines."""
import gzip
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrarec_ref as C  # noqa: E402
from conftest import rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g12():
    return np.load(os.path.join(GOLD, "g12_contrarec.npz"))


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _block(sd, D, heads):
    from whisprrec_amd.sasrec import _Block
    blk = _Block(D, D, heads, 0.0)
    blk.load_state_dict({n: torch.as_tensor(sd[n]) for n in C.PARAMS})
    return blk.to(DEV)


def _run_block(x, sd, g, heads, lens, err=None, p=0.0, seed=0, stored_max=None):
    """stored_max: a list that receives the call's stored score maximum"""
    from whisprrec_amd import hip_ops
    blk = _block(sd, x.shape[2], heads)
    xt = _t(x).requires_grad_(True)
    out = hip_ops.sasrec_block(xt, blk, heads, p, seed, True, key_lengths=_t(lens, torch.int64), err_word=err)
    if stored_max is not None:
        stored_max.append(float(out.grad_fn.saved_tensors[1].item()))
    out.backward(_t(g))
    return out.detach(), xt.grad.detach(), {n: q.grad.detach() for n, q in blk.named_parameters()}


# ------------------------------------------------------------------------------------------------ the block with key_len
@pytest.mark.parametrize("i", range(len(C.BLOCK_SHAPES)))
def test_block_with_key_lengths_matches_float64_and_repeats_its_bits(g12, i):
    x, sd, g, heads, lens = C.make_block_case(i, g12)
    T = x.shape[1]
    assert lens.max() == T and (lens.min() == 1 or x.shape[0] == 1)
    ref = C.block_keys_f64(x, sd, heads, lens, g)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, gx, gp = _run_block(x, sd, g, heads, lens, err)
    fig = C.figures(out.cpu().numpy(), gx.cpu().numpy(), {n: v.cpu().numpy() for n, v in gp.items()}, ref)
    print(C.block_fmt("B=%d T=%d D=%d h=%d" % C.BLOCK_SHAPES[i], fig))
    assert int(err.item()) == 0
    for n, v in fig.items():
        assert v <= C.BLOCK_TOL[C.group_of(n)], (n, v)
    out2, gx2, gp2 = _run_block(x, sd, g, heads, lens)
    assert torch.equal(out, out2) and torch.equal(gx, gx2) and all(torch.equal(gp[n], gp2[n]) for n in gp)


def test_block_clamps_lengths_outside_the_range_and_reports_them(g12):
    """key_len 0 and T + 1 are clamped to 1 and T before they bound a loop: the result is that of the clamped lengths, bit
    for bit, and the error word is set"""
    x, sd, g, heads, lens = C.make_block_case(2, g12)
    T = x.shape[1]
    bad = lens.copy()
    bad[0], bad[1] = T + 1, 0
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, gx, gp = _run_block(x, sd, g, heads, bad, err)
    assert int(err.item()) == 1
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gx).all())
    good = lens.copy()
    good[0], good[1] = T, 1
    out2, gx2, gp2 = _run_block(x, sd, g, heads, good)
    assert torch.equal(out, out2) and torch.equal(gx, gx2) and all(torch.equal(gp[n], gp2[n]) for n in gp)


# ------------------------------------------------------------------------------------------------ several visits per workgroup
SEED = 0x5A5B10C
LISTS = {"walk": (C.BLOCK_WALK_SHAPES, C.BLOCK_WALK_SEED, C.BLOCK_WALK_TOL), "form": (C.BLOCK_FORM_SHAPES, C.BLOCK_FORM_SEED, C.BLOCK_FORM_TOL)}
MAX_SCALE, MAX_SEQ = 100.0, 2049      # as tests/test_hip_sasblock.py: x of a sequence of a second visit of forward launch 1, scaled
_LIST = {}


def _list_case(which, i, p=0.0, peak=False):
    """(inputs, masks' seed, float64 result) of a case of BLOCK_WALK_SHAPES / BLOCK_FORM_SHAPES, computed once"""
    key = (which, i, p, peak)
    if key not in _LIST:
        shapes, seed, _ = LISTS[which]
        x, sd, g, heads, lens = C.make_block_case(i, shapes=shapes, seed=seed)
        assert lens.max() == x.shape[1] and lens.min() == 1
        if peak:
            x = x.copy()
            x[MAX_SEQ] *= MAX_SCALE
        m1, m2 = C.R.masks_for(SEED + seed + i, *x.shape, p)
        _LIST[key] = ((x, sd, g, heads, lens), SEED + seed + i, C.block_keys_f64(x, sd, heads, lens, g, m1=m1, m2=m2))
    return _LIST[key]


def _assert_list_figures(which, tag, res, ref):
    tol = LISTS[which][2]
    out, gx, gp = res
    got = {"out": out.cpu().numpy(), "gx": gx.cpu().numpy()}
    fig = C.figures(got["out"], got["gx"], {n: v.cpu().numpy() for n, v in gp.items()}, ref)
    print(C.block_fmt("%s %s" % (which, tag), fig, tol))
    if which == "walk":
        print("parity sasblock_keys walk %s visits (b < %d | later): %s" % (tag, C.R.BWD_WG,
                                                                          C.R.visit_fmt(C.R.visit_figures(got, ref, C.R.BWD_WG))))
    for n, v in fig.items():
        assert v <= tol[C.group_of(n)], (tag, n, v, tol[C.group_of(n)])


@pytest.mark.parametrize("i", range(len(C.BLOCK_WALK_SHAPES)), ids=["x".join(map(str, s)) for s in C.BLOCK_WALK_SHAPES])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_block_walk_parity_with_float64(i, p):
    """B above kSasBwdWg (and, at B = 2051, above kSasFwdWg): a workgroup meets several sequences, each with its own key length"""
    (x, sd, g, heads, lens), seed, ref = _list_case("walk", i, p)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    res = _run_block(x, sd, g, heads, lens, err, p, seed)
    assert int(err.item()) == 0
    _assert_list_figures("walk", "B=%d T=%d D=%d h=%d p=%g" % (*C.BLOCK_WALK_SHAPES[i], p), res, ref)


@pytest.mark.parametrize("i", range(len(C.BLOCK_FORM_SHAPES)), ids=["x".join(map(str, s)) for s in C.BLOCK_FORM_SHAPES])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_block_form_parity_with_float64(i, p):
    """T = 24 | 25 at both D, T = 64 at D = 32: every <D, TM> form of the keyed kernels at its border"""
    (x, sd, g, heads, lens), seed, ref = _list_case("form", i, p)
    _assert_list_figures("form", "B=%d T=%d D=%d h=%d p=%g" % (*C.BLOCK_FORM_SHAPES[i], p), _run_block(x, sd, g, heads, lens, None, p, seed), ref)


def test_block_walk_global_maximum_found_on_a_later_visit():
    """as tests/test_hip_sasblock.py's: the call's largest score on sequence 2049 of (2051, 2, 64, 4), 10 - 30 above the rest"""
    i = C.BLOCK_WALK_SHAPES.index((2051, 2, 64, 4))
    (x, sd, g, heads, lens), seed, ref = _list_case("walk", i, 0.0, True)
    rest = np.delete(ref["seq_max"], MAX_SEQ).max()
    assert MAX_SEQ >= C.R.FWD_WG and int(ref["seq_max"].argmax()) == MAX_SEQ and 10.0 < ref["gmax"] - rest < 30.0
    stored = []
    res = _run_block(x, sd, g, heads, lens, stored_max=stored)
    print("parity sasblock_keys walk maximum: stored %.6f float64 %.6f (best of the other sequences %.6f)" % (stored[0], ref["gmax"], rest))
    assert abs(stored[0] - ref["gmax"]) <= 1e-5 * abs(ref["gmax"])
    _assert_list_figures("walk", "B=2051 maximum at b=%d" % MAX_SEQ, res, ref)


def test_block_walk_two_identical_calls_give_equal_bits():
    """the shape with the most visits (4 - 5 per workgroup of the backward), p = 0.1"""
    (x, sd, g, heads, lens), seed, _ = _list_case("walk", C.BLOCK_WALK_SHAPES.index((2051, 2, 64, 4)), 0.1)
    out, gx, gp = _run_block(x, sd, g, heads, lens, None, 0.1, seed)
    out2, gx2, gp2 = _run_block(x, sd, g, heads, lens, None, 0.1, seed)
    assert torch.equal(out, out2) and torch.equal(gx, gx2) and all(torch.equal(gp[n], gp2[n]) for n in gp)


def test_block_walk_bad_length_on_a_later_visit_is_clamped_and_reported():
    """key_len 0 and T + 1 at sequences b >= kSasBwdWg (the second visit of workgroups 1 and 2): the error word is set and the
    result is the restatement's with the clamped lengths"""
    i = C.BLOCK_WALK_SHAPES.index((1027, 5, 32, 2))
    (x, sd, g, heads, lens), _, _ = _list_case("walk", i)
    T, G = x.shape[1], C.R.BWD_WG
    bad, good = lens.copy(), lens.copy()
    bad[G + 1], bad[G + 2] = 0, T + 1
    good[G + 1], good[G + 2] = 1, T
    assert (bad[:G] >= 1).all() and (bad[:G] <= T).all()
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    res = _run_block(x, sd, g, heads, bad, err)
    assert int(err.item()) == 1
    _assert_list_figures("walk", "B=1027 clamped lengths", res, C.block_keys_f64(x, sd, heads, good, g))
    res2 = _run_block(x, sd, g, heads, good)
    assert torch.equal(res[0], res2[0]) and torch.equal(res[1], res2[1]) and all(torch.equal(res[2][n], res2[2][n]) for n in res[2])


# ------------------------------------------------------------------------------------------------ the loss
@pytest.mark.parametrize("i", range(len(C.LOSS_SHAPES)))
def test_supcon_matches_float64_and_repeats_its_bits(i):
    from whisprrec_amd import hip_ops
    F, labels, tau = C.make_loss_case(i)
    ref = C.supcon_f64(F, labels, tau)
    Ft, lt = _t(F), _t(labels)
    loss, gF = hip_ops.supcon_loss_grad(Ft, lt, tau)
    fig = C.loss_figures(float(loss.item()), gF.cpu().numpy(), ref)
    print(C.loss_fmt("B=%d D=%d tau=%g labels=%d" % C.LOSS_SHAPES[i], fig))
    for k in fig:
        assert fig[k] <= C.LOSS_TOL[k], (k, fig[k])
    only, none = hip_ops.supcon_loss_grad(Ft, lt, tau, grads=False)
    assert none is None and torch.equal(only, loss)                              # loss only: the same bits
    loss2, gF2 = hip_ops.supcon_loss_grad(Ft, lt, tau)
    assert torch.equal(loss, loss2) and torch.equal(gF, gF2)
    # weight and accumulation: loss_out = loss_in + weight * loss
    acc = torch.full((1,), 2.0, dtype=torch.float32, device=DEV)
    hip_ops.supcon_loss_grad(Ft, lt, tau, weight=0.5, loss=acc, grads=False)
    assert abs(float(acc.item()) - (2.0 + 0.5 * ref[0])) <= 4e-6 * (2.0 + abs(ref[0]))


def test_supcon_autograd_function_hands_back_the_kernel_gradient():
    from whisprrec_amd import hip_ops
    F, labels, tau = C.make_loss_case(2)
    Ft = _t(F).requires_grad_(True)
    (3.0 * hip_ops.supcon_loss(Ft, _t(labels), tau)).backward()
    ref = C.supcon_f64(F, labels, tau, weight=3.0)
    assert rel_err(Ft.grad.cpu().numpy(), ref[1]) <= C.LOSS_TOL["gF"]


def test_supcon_single_pair():
    """B = 1: each row's only other row is its positive; the exact loss is about tau * 1e-10 * e^{1/tau}, so it is checked
    absolutely"""
    from whisprrec_amd import hip_ops
    F = np.random.RandomState(3).standard_normal((2, 64)).astype(np.float32)
    loss, gF = hip_ops.supcon_loss_grad(_t(F), _t(np.array([7], np.int64)), 0.2)
    print("parity supcon B=1: loss %.3e (float64 %.3e)" % (float(loss.item()), C.supcon_f64(F, [7], 0.2)[0]))
    assert abs(float(loss.item())) < 1e-6 and bool(torch.isfinite(gF).all())


# ------------------------------------------------------------------------------------------------ the model
def _model(g12, **flags):
    import argparse
    from whisprrec_amd import host
    from whisprrec_amd.contrarec import ContraRec
    args = argparse.Namespace(device=DEV, model_path="/tmp/wr_contrarec_gpu.pt", buffer=1, num_neg=1, test_all=1, history_max=20,
                              emb_size=64, gamma=0.5, beta_a=3, beta_b=3, ccc_temp=0.2, **flags)
    m = ContraRec(args, host.Corpus(40, 300, {}))
    m.load_state_dict({str(n): torch.from_numpy(g12["sd__" + str(n)]) for n in g12["names"]})
    return m.to(DEV).train()


def _feed(g12):
    t = {k: _t(g12[k]) for k in ("hist", "hist_a", "hist_b", "lengths", "pos", "neg")}
    return {"history_items": t["hist"], "history_items_a": t["hist_a"], "history_items_b": t["hist_b"], "lengths": t["lengths"],
            "pos_item": t["pos"], "neg_items": t["neg"], "phase": "train", "batch_size": 96}


KB, KW = "masked_attn_head.k_linear.bias", "masked_attn_head.k_linear.weight"
MODEL_LOSS_TOL = 1e-5      # the north-star yardstick of conftest.rel_err: within 1e-5 relative
MODEL_GRAD_TOL = 5e-5      # the widest of contrarec_ref.BLOCK_TOL: every parameter gradient is a sum of such block terms


def test_native_model_matches_its_torch_path_and_the_reference_on_g12(g12):
    grads, losses = {}, {}
    for tag, flags in (("torch", dict(block_native=0, ccc_native=0)), ("native", dict(block_native=1, ccc_native=1))):
        m = _model(g12, **flags)
        loss = m.predict(_feed(g12))
        loss.backward()
        losses[tag] = (float(loss.detach()), float(m.last_losses[0]), float(m.last_losses[1]))
        grads[tag] = {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()}
        if tag == "native":
            m.check_key_lengths()
            assert m._block_native_ok == {20: True} and m._ccc_native_ok == {96: True}, "the kernels refused the golden shape"
    for k, nm in enumerate(("loss", "ctc", "ccc")):
        a, b, ref = losses["native"][k], losses["torch"][k], float(g12[nm][0])
        print("parity contrarec g12 %s: native %.7f torch %.7f reference %.7f (tol %.0e)" % (nm, a, b, ref, MODEL_LOSS_TOL))
        assert abs(a - b) <= MODEL_LOSS_TOL * abs(b) and abs(a - ref) <= MODEL_LOSS_TOL * abs(ref)
    worst = 0.0
    for n, ref in grads["torch"].items():
        scale = grads["torch"][n.replace(KB, KW)] if n.endswith(KB) else ref        # d loss / d b_k is zero on paper
        for other in (ref, g12["g__" + n]):
            fig = float(np.abs(grads["native"][n] - other).max()) / float(np.abs(scale).max())
            worst = max(worst, fig)
            assert fig <= MODEL_GRAD_TOL, (n, fig)
    print("parity contrarec g12 gradients: worst %.2e (tol %.0e)" % (worst, MODEL_GRAD_TOL))


def _write_ml100k(tmp):
    (tmp / "ml-100k").mkdir()
    with gzip.open(os.path.join(GOLD, "ml-100k.inter.gz"), "rb") as src, open(tmp / "ml-100k" / "ml-100k.inter", "wb") as dst:
        shutil.copyfileobj(src, dst)
    return str(tmp) + "/"


def _argv(path, tmp, extra):
    return ["--model_name", "ContraRec", "--runner_name", "HipRunner", "--dataset", "ml-100k", "--path", path, "--epoch", "2",
            "--batch_size", "1024", "--eval_batch_size", "2048", "--lr", "1e-3", "--l2", "0.0", "--emb_size", "64", "--history_max", "20",
            "--log_file", str(tmp / "log.txt"), "--model_path", str(tmp / "m.pt"), "--num_workers", "0", "--topk", "5,10",
            "--metric", "NDCG, HR", "--random_seed", "3407"] + extra


EPOCH_MARGIN = 4e-4


def test_two_epoch_launcher_run_native_against_torch_path(tmp_path):
    """`main`'s training for two epochs on tests/golden/ml-100k.inter.gz, --block_native 1 --ccc_native 1 against the torch path,
    same seed: the epoch losses agree within EPOCH_MARGIN (relative).

    The margin comes from the torch path alone: this command run again with its sums in another order.  Measured on an MI355X,
    relative to the plain torch run (epoch losses 1.8853989, 1.6177776), epoch 1 / epoch 2:
        the GEMMs on the other BLAS library (torch.backends.cuda.preferred_blas_library)   2.0e-6 / 2.5e-5
        every batch with its rows reversed (the sums over the batch run backwards)          2.0e-5 / 4.3e-5
        torch.use_deterministic_algorithms(True)                                            0 / 0 (no kernel of this step changes)
    The largest, 4.3e-5, is the floor; by DESIGN section 2's rule EPOCH_MARGIN = 8 x floor rounded up to one digit.  The bare
    floor is not used as the bound: two such runs are two draws of a diverging trajectory, and the three draws above already differ
    by a factor of two.  The native run measured 1.8e-5 / 5.7e-5 in the same session."""
    from whisprrec_amd import main as launcher
    path = _write_ml100k(tmp_path)
    curves = {}
    for tag, extra in (("torch", []), ("native", ["--block_native", "1", "--ccc_native", "1"])):
        args, model_class, reader_class, runner_class = launcher.build_args(_argv(path, tmp_path, extra))
        launcher.init_seed(args.random_seed)
        args.device = DEV
        corpus = reader_class(args).corpus()
        model = model_class(args, corpus).to(DEV)
        data = model_class.Dataset(model, corpus, "train")
        run = runner_class(args)
        curves[tag] = [run.fit(data, epoch=e + 1) for e in range(2)]
        if tag == "native":
            model.check_key_lengths()
            assert all(model._block_native_ok.values()) and all(model._ccc_native_ok.values())
    rel = np.abs(np.asarray(curves["native"]) / np.asarray(curves["torch"]) - 1.0)
    print("parity contrarec ml-100k epochs: torch %s native %s rel %s (margin %.0e)" % (curves["torch"], curves["native"], rel, EPOCH_MARGIN))
    assert curves["torch"][1] < curves["torch"][0]
    assert rel.max() <= EPOCH_MARGIN


def test_device_evaluation_equals_the_host_loop(tmp_path):
    """--seq_eval_native 1 on the small corpus: the metrics of the device ranking equal the host loop's, up to rows whose target
    is nearly tied with another item"""
    from test_reader import _write_inter
    from whisprrec_amd import main as launcher, runner
    g8 = np.load(os.path.join(GOLD, "g8_reader.npz"))
    path = _write_inter(g8, tmp_path)
    argv = _argv(path, tmp_path, ["--seq_eval_native", "1", "--block_native", "1", "--emb_size", "32"])
    args, model_class, reader_class, runner_class = launcher.build_args(argv)
    launcher.init_seed(args.random_seed)
    args.device = DEV
    corpus = reader_class(args).corpus()
    model = model_class(args, corpus).to(DEV)
    with torch.no_grad():
        model.item_embeddings.weight.mul_(30)                                   # scores spread: few near-ties
    ds = model_class.Dataset(model, corpus, "dev")
    run = runner_class(args)
    assert run._seq_eval_ok(ds)
    assert model.eval_items().shape[0] == corpus.n_items + 1                    # the mask-token column is ranked too
    pred = runner.BaseRunner(args).interface(ds).astype(np.float64)
    host_rank = np.argwhere((-pred).argsort(axis=1) == 0)[:, 1] + 1
    rank = run.rank_rows(ds)
    target, S = pred[:, 0], pred[:, 1:].copy()
    S[np.arange(len(ds)), np.asarray(ds.data["item_id"])] = np.nan
    fin = np.isfinite(S)
    ok = np.where(fin, np.abs(S - target[:, None]), np.inf).min(axis=1) > 1e-5 * np.abs(S[fin]).max()
    print("parity contrarec seq eval: n_eval %d rows kept %.4f ranks differing on kept rows %d" %
          (len(ds), ok.mean(), int((rank[ok] != host_rank[ok]).sum())))
    assert ok.mean() >= 0.9 and np.array_equal(rank[ok], host_rank[ok])
    dev_res = run.evaluate(ds, [5, 10], ["NDCG", "HR"])
    host_res = runner.BaseRunner.metrics_from_ranks(host_rank, [5, 10], ["NDCG", "HR"])
    for key in host_res:
        assert abs(host_res[key] - dev_res[key]) <= (~ok).sum() / len(ds), key
