"""wr_sasblock_fwd / wr_sasblock_bwd (K13) on the GPU against the float64 restatement of tests/sasblock_ref.py: parity of the
output, gx and every parameter gradient on every shape with and without dropout (the shapes at which a workgroup visits several
sequences and every <D, TM> form of the kernels included), bitwise reproducibility, the global score shift with its zeroed rows, the whole SASRec model with --block_native 1 against the reference's golden loss and gradient and
against --block_native 0 in the same process, and the launcher's end-to-end run.  Run with -rP for the `parity sasblock` lines."""
import argparse
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sasblock_ref as R  # noqa: E402
from conftest import load_golden, rel_err  # noqa: E402
from whisprrec_amd import host  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 0x5A5B10C


@functools.lru_cache(maxsize=None)
def _case(i):
    return R.make_case(i, load_golden("g5_sasrec_emb"))


@functools.lru_cache(maxsize=None)
def _reference(i, p):
    x, sd, g, heads = _case(i)
    m1, m2 = R.masks_for(SEED + i, *x.shape, p)
    return R.block_f64(x, sd, heads, g, m1, m2)


def _block(sd, D, heads, dev):
    from whisprrec_amd.sasrec import _Block
    blk = _Block(D, D, heads, 0.0)
    blk.load_state_dict({n: torch.from_numpy(np.asarray(sd[n])) for n in R.PARAMS})
    return blk.to(dev)


def _native(x, sd, heads, g, p, seed, training=True):
    """-> (out, gx, {name: grad}) of hip_ops.sasrec_block as numpy arrays"""
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    blk = _block(sd, x.shape[2], heads, dev)
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = hip_ops.sasrec_block(xt, blk, heads, p, seed, training)
    out.backward(torch.from_numpy(g).to(dev))
    return out.detach().cpu().numpy(), xt.grad.cpu().numpy(), {n: q.grad.cpu().numpy() for n, q in blk.named_parameters()}


def _assert_figures(tag, fig):
    print(R.fmt(tag, fig))
    for n, v in fig.items():
        assert v < R.TOL[R.group_of(n)], (tag, n, v, R.TOL[R.group_of(n)])


@pytest.mark.parametrize("i", range(len(R.SHAPES)))
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_parity_with_float64(i, p):
    x, sd, g, heads = _case(i)
    out, gx, gp = _native(x, sd, heads, g, p, SEED + i)
    _assert_figures("B=%d T=%d D=%d h=%d p=%g" % (*R.SHAPES[i], p), R.figures(out, gx, gp, _reference(i, p)))


@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_evaluation_mode_ignores_dropout(i):
    """training = 0 with p = 0.1 gives the bits of p = 0"""
    x, sd, g, heads = _case(i)
    a = _native(x, sd, heads, g, 0.1, SEED + i, training=False)
    b = _native(x, sd, heads, g, 0.0, SEED + i, training=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for n in R.PARAMS:
        assert np.array_equal(a[2][n], b[2][n]), n


@pytest.mark.parametrize("i", [0, 4, 5])
def test_two_identical_calls_give_equal_bits(i):
    x, sd, g, heads = _case(i)
    a = _native(x, sd, heads, g, 0.1, SEED + i)
    b = _native(x, sd, heads, g, 0.1, SEED + i)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for n in R.PARAMS:
        assert np.array_equal(a[2][n], b[2][n]), n
    c = _native(x, sd, heads, g, 0.1, SEED + i + 1)                      # and another seed is another mask
    assert not np.array_equal(a[0], c[0])


# ------------------------------------------------------------------------------------------------ several visits per workgroup
LISTS = {"walk": (R.WALK_SHAPES, R.WALK_SEED, R.WALK_TOL), "form": (R.FORM_SHAPES, R.FORM_SEED, R.FORM_TOL)}
MAX_SCALE = 100.0          # x of one late sequence times this: its best score lies 10 - 30 above every other sequence's
MAX_SEQ = 2049             # a sequence forward launch 1 reaches on a second visit (b >= R.FWD_WG)


@functools.lru_cache(maxsize=None)
def _list_case(which, i, peak=False):
    shapes, seed, _ = LISTS[which]
    x, sd, g, heads = R.make_case(i, shapes=shapes, seed=seed)
    if peak:
        x = x.copy()
        x[MAX_SEQ] *= MAX_SCALE
    return x, sd, g, heads


@functools.lru_cache(maxsize=None)
def _list_reference(which, i, p, peak=False):
    x, sd, g, heads = _list_case(which, i, peak)
    m1, m2 = R.masks_for(SEED + LISTS[which][1] + i, *x.shape, p)
    return R.block_f64(x, sd, heads, g, m1, m2)


def _native_with_max(x, sd, heads, g, p, seed):
    """-> (dict(out, gx), {name: grad}, the call's stored score maximum) of hip_ops.sasrec_block"""
    from whisprrec_amd import hip_ops
    dev = torch.device("cuda:0")
    blk = _block(sd, x.shape[2], heads, dev)
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = hip_ops.sasrec_block(xt, blk, heads, p, seed, True)
    gmax = float(out.grad_fn.saved_tensors[1].item())
    out.backward(torch.from_numpy(g).to(dev))
    return ({"out": out.detach().cpu().numpy(), "gx": xt.grad.cpu().numpy()}, {n: q.grad.cpu().numpy() for n, q in blk.named_parameters()},
            gmax)


def _assert_list_figures(which, tag, got, gp, ref):
    tol = LISTS[which][2]
    fig = R.figures(got["out"], got["gx"], gp, ref)
    print(R.fmt("%s %s" % (which, tag), fig, tol))
    if which == "walk":
        print("parity sasblock walk %s visits (b < %d | later): %s" % (tag, R.BWD_WG, R.visit_fmt(R.visit_figures(got, ref, R.BWD_WG))))
    for n, v in fig.items():
        assert v < tol[R.group_of(n)], (tag, n, v, tol[R.group_of(n)])


@pytest.mark.parametrize("i", range(len(R.WALK_SHAPES)), ids=["x".join(map(str, s)) for s in R.WALK_SHAPES])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_walk_parity_with_float64(i, p):
    """B above kSasBwdWg (and, at B = 2051, above kSasFwdWg): every workgroup of the backward visits several sequences"""
    x, sd, g, heads = _list_case("walk", i)
    got, gp, _ = _native_with_max(x, sd, heads, g, p, SEED + R.WALK_SEED + i)
    _assert_list_figures("walk", "B=%d T=%d D=%d h=%d p=%g" % (*R.WALK_SHAPES[i], p), got, gp, _list_reference("walk", i, p))


@pytest.mark.parametrize("i", range(len(R.FORM_SHAPES)), ids=["x".join(map(str, s)) for s in R.FORM_SHAPES])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_form_parity_with_float64(i, p):
    """T = 24 | 25 at both D: the last T of the TM = 24 kernels and the first of the TM = 64 ones; T = 64 at D = 32"""
    x, sd, g, heads = _list_case("form", i)
    got, gp, _ = _native_with_max(x, sd, heads, g, p, SEED + R.FORM_SEED + i)
    _assert_list_figures("form", "B=%d T=%d D=%d h=%d p=%g" % (*R.FORM_SHAPES[i], p), got, gp, _list_reference("form", i, p))


def test_walk_global_maximum_found_on_a_later_visit():
    """(2051, 2, 64, 4) with x of sequence 2049 scaled: the call's largest score sits on a sequence that forward launch 1 meets on
    a workgroup's second visit, 10 - 30 above every other sequence's (nothing underflows).  The stored maximum equals the
    restatement's to 1e-5 relative (BASELINE.json's yardstick); one folded from the first 2,048 sequences misses by the gap."""
    i = R.WALK_SHAPES.index((2051, 2, 64, 4))
    x, sd, g, heads = _list_case("walk", i, True)
    ref = _list_reference("walk", i, 0.0, True)
    rest = np.delete(ref["seq_max"], MAX_SEQ).max()
    assert MAX_SEQ >= R.FWD_WG and int(ref["seq_max"].argmax()) == MAX_SEQ and 10.0 < ref["gmax"] - rest < 30.0
    got, gp, gmax = _native_with_max(x, sd, heads, g, 0.0, SEED)
    print("parity sasblock walk maximum: stored %.6f float64 %.6f (best of the other sequences %.6f)" % (gmax, ref["gmax"], rest))
    assert abs(gmax - ref["gmax"]) <= 1e-5 * abs(ref["gmax"])
    _assert_list_figures("walk", "B=2051 maximum at b=%d" % MAX_SEQ, got, gp, ref)


def test_walk_two_identical_calls_give_equal_bits():
    """the shape with the most visits (4 - 5 per workgroup of the backward), p = 0.1"""
    i = R.WALK_SHAPES.index((2051, 2, 64, 4))
    x, sd, g, heads = _list_case("walk", i)
    a = _native(x, sd, heads, g, 0.1, SEED + i)
    b = _native(x, sd, heads, g, 0.1, SEED + i)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for n in R.PARAMS:
        assert np.array_equal(a[2][n], b[2][n]), n


def _with_shift(alt, ref, x, sd, heads, b, zr):
    """output [T, D] of sequence b alone under the WHOLE call's shift: the maximum comes from sequence 0, so sequence 0 alone
    already has it (`alt`); any other sequence is evaluated together with sequence 0"""
    if b == 0:
        assert alt["gmax"] == ref["gmax"]
        return alt["out"][0]
    both = R.block_f64(x[[0, b]], sd, heads, zero_below=150.0, zero_rows=zr[[0, b]])
    assert both["gmax"] == ref["gmax"]
    return both["out"][1]


def test_global_shift_zeroes_the_rows_far_below_the_maximum():
    """x[0] *= 60 on the first 8 sequences of g5: the call's maximum score (428 in float64) comes from sequence 0, and every
    score row more than 104 below it underflows in fp32 — 0 / 0 in the reference, zeroed by its isnan fill.  Rows more than
    150 below are zero in any fp32 evaluation, rows within 60 are ordinary; rows in between are decided by the denormal
    handling of exp and are left out, with every position that holds one."""
    x, sd, g, heads = _case(0)
    x, g = x[:8].copy(), g[:8].copy()
    x[0] *= 60.0
    ref = R.block_f64(x, sd, heads, g, zero_below=150.0)
    gap = ref["gap"]                                                      # [8, 4, 20]
    far, near = gap > 150.0, gap < 60.0
    between = ~(far | near)
    print("parity sasblock shift: max %.1f, rows far %d near %d between %d" % (ref["gmax"], far.sum(), near.sum(), between.sum()))
    # float64 quantities of fixed inputs: pinned, so that the case cannot drift silently
    assert gap.size == 640 and (int(far.sum()), int(near.sum()), int(between.sum())) == (624, 3, 13)
    assert between.sum() <= 0.05 * gap.size
    assert np.array_equal(ref["zero_rows"], far)
    out, gx, gp = _native(x, sd, heads, g, 0.0, SEED)
    scale = np.abs(ref["out"]).max()
    zeroed = far.all(axis=1)                                              # positions whose four heads are all zeroed: residual only
    assert zeroed.sum() == 148                                            # 7 x 20 of the other sequences, 8 of sequence 0
    e_zero = np.abs(out[zeroed] - ref["out"][zeroed]).max() / scale
    print("parity sasblock shift: out on %d zeroed positions %.2e (tol %.0e)" % (zeroed.sum(), e_zero, R.TOL["out"]))
    assert e_zero < R.TOL["out"]
    # The ordinary rows.  Only the block's output is visible, and LayerNorm mixes the four heads of a position, so a
    # position is compared as a whole.  Every position that holds an ordinary row here also holds rows in between; those are
    # left undecided: the output must match the restatement with each of them EITHER zeroed OR ordinary, at the usual bound.
    # Positions of sequence 0 where some heads are far and the others undecided hold no ordinary row: they are not compared.
    checked = 0
    for b, t in zip(*np.nonzero(near.any(axis=1))):
        und = np.nonzero(between[b, :, t])[0]
        best = np.inf
        for pick in range(1 << und.size):
            zr = np.zeros(gap.shape, bool)
            zr[b, und[[k for k in range(und.size) if pick >> k & 1]], t] = True
            alt = R.block_f64(x[b:b + 1], sd, heads, zero_below=150.0, zero_rows=zr[b:b + 1])
            best = min(best, np.abs(out[b, t] - _with_shift(alt, ref, x, sd, heads, b, zr)[t]).max() / scale)
        print("parity sasblock shift: position (%d, %d) with %d ordinary and %d undecided rows: %.2e (tol %.0e)"
              % (b, t, near[b, :, t].sum(), und.size, best, R.TOL["out"]))
        assert best < R.TOL["out"]
        checked += int(near[b, :, t].sum())
    assert checked == near.sum()
    assert np.isfinite(out).all() and np.isfinite(gx).all()
    for n in R.PARAMS:
        assert np.isfinite(gp[n]).all(), n


# ------------------------------------------------------------------------------------------------ the whole model
def _model(g5, dev, native, emb_size=64, heads=4):
    from whisprrec_amd.sasrec import SASRec
    args = argparse.Namespace(device=dev, model_path="/tmp/wr_sas.pt", buffer=1, num_neg=1, test_all=1, emb_size=emb_size,
                              num_layers=1, num_heads=heads, dropout=0.0, history_max=20, block_native=native)
    m = SASRec(args, host.Corpus(13, 71, {})).to(dev)
    fd = {"history_items": torch.from_numpy(g5["hist"]).to(dev), "lengths": torch.from_numpy(g5["lengths"]).to(dev),
          "pos_item": torch.from_numpy(g5["pos"]).to(dev), "neg_items": torch.from_numpy(g5["neg"]).to(dev)}
    return m, fd


def test_model_reproduces_the_reference_and_the_torch_path(g5):
    dev = torch.device("cuda:0")
    sd = {k[4:]: torch.from_numpy(g5[k]) for k in g5.files if k.startswith("sd__")}
    grads = {}
    for native in (1, 0):
        m, fd = _model(g5, dev, native)
        assert set(sd) == set(m.state_dict().keys())                      # parameter names and checkpoints are unchanged
        m.load_state_dict(sd)
        m.train()
        loss = m.predict(fd)
        loss.backward()
        assert m._use_block_native(20) == bool(native)
        assert abs(float(loss.detach()) - float(g5["loss"][0])) / float(g5["loss"][0]) < 1e-4
        gW = m.item_embedding.weight.grad.cpu().numpy()
        assert rel_err(gW, g5["gW_full"]) < 1e-4 and not gW[0].any()
        grads[native] = {n: q.grad.cpu().numpy() for n, q in m.named_parameters()}
    pre = "transformer_block.0."
    kw = np.abs(grads[0][pre + R.KW]).max()
    for n, ref in grads[0].items():
        short = n[len(pre):] if n.startswith(pre) else "gx"               # the embeddings' gradients are gx scattered
        if short == R.KB:
            err = np.abs(grads[1][n] - ref).max() / kw
        else:
            err = rel_err(grads[1][n], ref)
        print("parity sasblock model %s: %.2e (tol %.0e)" % (n, err, R.TOL[R.group_of(short)]))
        assert err < R.TOL[R.group_of(short)], n


def test_unsupported_emb_size_falls_back_with_a_warning_and_still_trains(g5, caplog):
    dev = torch.device("cuda:0")
    m, fd = _model(g5, dev, 1, emb_size=48, heads=4)
    m.train()
    with caplog.at_level(logging.WARNING):
        loss = m.predict(fd)
        loss.backward()
        m.predict(fd)
    assert sum("block_native" in r.getMessage() for r in caplog.records) == 1        # logged once
    assert np.isfinite(float(loss.detach())) and m.item_embedding.weight.grad.abs().sum() > 0
    assert m.transformer_block[0].linear1.weight.grad.abs().sum() > 0


def test_end_to_end_run_with_the_native_block_matches_the_reference_train_loop(tmp_path):
    """tests/test_reader.py's `sasrec` launcher run with --block_native 1: per-epoch training loss of the reference's
    BaseRunner.train (tests/golden/g9_end_to_end.npz) at that test's rtol 5e-5"""
    from test_reader import _write_inter
    from whisprrec_amd import main as launcher
    here = os.path.dirname(os.path.abspath(__file__))
    g8 = np.load(os.path.join(here, "golden", "g8_reader.npz"))
    g9 = np.load(os.path.join(here, "golden", "g9_end_to_end.npz"))
    path = _write_inter(g8, tmp_path)
    lr, l2, epochs = g9["sasrec_hp"]
    argv = ["--emb_size", "32", "--num_layers", "1", "--num_heads", "2", "--dropout", "0.0", "--history_max", "20", "--block_native", "1",
            "--model_name", "SASRec", "--runner_name", "BaseRunner", "--dataset", "ml-100k", "--path", path, "--epoch", str(int(epochs)),
            "--batch_size", "1024", "--eval_batch_size", "2048", "--optimizer", "Adam", "--lr", repr(float(lr)), "--l2", repr(float(l2)),
            "--log_file", str(tmp_path / "log.txt"), "--model_path", str(tmp_path / "m.pt"), "--num_workers", "0", "--topk", "10,20",
            "--metric", "NDCG, HR", "--random_seed", "3407"]
    args, model_class, reader_class, runner_class = launcher.build_args(argv)
    launcher.init_seed(args.random_seed)
    args.device = torch.device("cuda")
    corpus = reader_class(args).corpus()
    model = model_class(args, corpus).to(args.device)
    data = {ph: model_class.Dataset(model, corpus, ph) for ph in ("train", "dev")}
    run = runner_class(args)
    losses, devs = [], []
    for epoch in range(args.epoch):
        losses.append(run.fit(data["train"], epoch=epoch + 1))
        devs.append(run.evaluate(data["dev"], run.topk[:1], run.metrics))
    assert all(model._block_native_ok.values()) and model._block_native_ok
    dev_err = np.abs(np.asarray(losses) - g9["sasrec_loss"]) / np.abs(g9["sasrec_loss"])
    print("parity sasblock end to end: loss rel err per epoch " + " ".join("%.2e" % v for v in dev_err) + " (rtol 5e-05)")
    assert np.allclose(losses, g9["sasrec_loss"], rtol=5e-5, atol=0)
    dev = np.asarray([[d[k] for k in g9["sasrec_dev_keys"]] for d in devs])
    assert np.abs(dev - g9["sasrec_dev"]).max() <= 6.0 / len(data["dev"])
