"""Full-catalogue softmax loss (--train_loss softmax): the fused kernels (wr_softmax_ce_loss_grad, K26) against the stock path
(matmul, logits[:, 0] = -inf, F.cross_entropy under torch.autograd — what --softmax_native 0 runs).  Per shape, two things:
loss + gradients alone, and one SASRec training step (predict / backward / Adam) with the flag at 0 and at 1, D = 64, T = 20.
Device events, warm-up, the two arms alternating inside one timed loop, median and spread of --reps runs, the peak memory of a
call and of a warm step (above what stays allocated between steps: parameters, Adam's state, the native arm's workspace), and
the losses of both arms.  Where the stock arm cannot allocate, that is recorded instead of a time.
Writes profiles/softmax_loss_bench_n1.json and prints the same JSON line.

    python scripts/bench_softmax_loss.py [--reps 10] [--shapes all|small] [--out profiles/softmax_loss_bench_n1.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisprrec_amd import hip_ops  # noqa: E402

PEAK_TFLOPS = 157.3           # fp32 matrix peak of one MI355X
D, T = 64, 20
SHAPES = [(3_706, 256), (3_706, 2048), (100_000, 2048), (1_000_000, 2048)]      # n_items, B


def timed_pair(fns, reps, warmup=2):
    """the arms of `fns` (name -> callable) alternating: -> name -> (median, min, max) ms by device events"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}


def peak_of(fn, dev):
    """peak bytes allocated above what is live before the call"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return peak


def stock(Q, E, target):
    Q = Q.detach().requires_grad_(True)
    E = E.detach().requires_grad_(True)
    logits = Q @ E.t()
    logits[:, 0] = -float("inf")
    loss = F.cross_entropy(logits, target)
    gQ, gE = torch.autograd.grad(loss, [Q, E])
    return loss.detach(), gQ, gE


def _ms(row, key, t):
    row[key + "_ms"] = round(t[0], 3)
    row[key + "_ms_min_max"] = [round(t[1], 3), round(t[2], 3)]


def bench_op(n, B, reps, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    Q = torch.randn(B, D, device=dev, generator=g)
    E = torch.randn(n, D, device=dev, generator=g) * 0.1
    target = torch.randint(1, n, (B,), device=dev, generator=g)
    hip_ops.softmax_ce_release_workspaces()
    row = dict(n_items=n, B=B, D=D)
    row["native_peak_mb"] = round(peak_of(lambda: hip_ops.softmax_ce_loss_grad(Q, E, target, validate=False), dev) / 2**20, 1)
    row["workspace_mb"] = round(hip_ops.softmax_ce_workspace_bytes(n, B, D) / 2**20, 1)
    row["one_score_matrix_mb"] = round(B * n * 4 / 2**20, 1)
    gQ, gE = torch.empty_like(Q), torch.empty_like(E)
    arms = {"native": lambda: hip_ops.softmax_ce_loss_grad(Q, E, target, out=(gQ, gE), validate=False),
            "native_loss_only": lambda: hip_ops.softmax_ce_loss_grad(Q, E, target, grads=False, validate=False)}
    try:
        row["stock_peak_mb"] = round(peak_of(lambda: stock(Q, E, target), dev) / 2**20, 1)
        arms["stock"] = lambda: stock(Q, E, target)
        ts = timed_pair(arms, reps)
        ln = hip_ops.softmax_ce_loss_grad(Q, E, target, out=(gQ, gE), validate=False)[0]
        ls, sQ, sE = stock(Q, E, target)
        row.update(native_loss=float(ln[0]), stock_loss=float(ls),
                   gQ_rel_diff_vs_stock=float((gQ - sQ).abs().max() / sQ.abs().max()),
                   gE_rel_diff_vs_stock=float((gE - sE).abs().max() / sE.abs().max()))
        del sQ, sE
    except torch.OutOfMemoryError as e:          # record it, do not shrink the case
        arms.pop("stock", None)
        torch.cuda.empty_cache()
        ts = timed_pair(arms, reps)
        row.update(stock_ms=None, stock_peak_mb=None, stock_error=str(e).split("\n")[0][:300],
                   native_loss=float(hip_ops.softmax_ce_loss_grad(Q, E, target, grads=False, validate=False)[0][0]))
    for k, t in ts.items():
        _ms(row, k, t)
    # matrix-core work of the native call: scores in three passes, weights x rows in two
    flop = 5 * 2.0 * B * n * D
    row["native_tflops"] = round(flop / ts["native"][0] / 1e9, 1)
    row["native_share_of_fp32_matrix_peak"] = round(flop / ts["native"][0] / 1e9 / PEAK_TFLOPS, 3)
    if "stock" in ts:
        row["ratio_native_to_stock"] = round(ts["native"][0] / ts["stock"][0], 3)
    return row


class _Corpus:
    def __init__(self, n_users, n_items):
        self.n_users, self.n_items, self.user_his = n_users, n_items, {}


def _step_arm(n, B, native, dev):
    """a SASRec (1 layer, 4 heads, torch blocks) with Adam and one fixed batch -> a callable that runs one training step"""
    from whisprrec_amd.sasrec import SASRec
    args = argparse.Namespace(device=dev, model_path="", buffer=1, num_neg=1, test_all=1, history_max=T, emb_size=D, num_layers=1,
                              num_heads=4, dropout=0.1, block_native=0, emb_lazy=0, random_seed=1, train_loss="softmax",
                              softmax_native=native)
    torch.manual_seed(1)
    model = SASRec(args, _Corpus(1000, n)).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    g = torch.Generator(device=dev).manual_seed(2)
    lengths = torch.randint(1, T + 1, (B,), device=dev, generator=g)
    hist = torch.randint(1, n, (B, T), device=dev, generator=g) * (torch.arange(T, device=dev)[None, :] < lengths[:, None])
    batch = {"history_items": hist, "lengths": lengths, "pos_item": torch.randint(1, n, (B,), device=dev, generator=g),
             "neg_items": torch.randint(1, n, (B, 1), device=dev, generator=g), "batch_size": B, "phase": "train"}
    model._trusted_indices = True                # as inside HipRunner.fit: the epoch's columns are range-checked once
    state = {}

    def step():
        opt.zero_grad()
        loss = model.predict(batch)
        loss.backward()
        opt.step()
        state["loss"] = loss.detach()
        return loss

    return step, state, (model, opt)


def bench_step(n, B, reps, dev):
    row = dict(n_items=n, B=B, D=D, T=T, optimizer="Adam",
               native_workspace_mb_kept_between_steps=round(hip_ops.softmax_ce_workspace_bytes(n, B, D) / 2**20, 1))
    arms, states, keep = {}, {}, []
    for native, name in ((1, "native"), (0, "stock")):
        hip_ops.softmax_ce_release_workspaces()
        try:
            step, state, objs = _step_arm(n, B, native, dev)
            step()                                   # allocates Adam's state and the workspace, which persist
            row[name + "_first_step_loss"] = float(state["loss"])
            row[name + "_step_peak_mb"] = round(peak_of(step, dev) / 2**20, 1)      # a warm step: what a step needs on top
            arms[name], states[name] = step, state
            keep.append(objs)
        except torch.OutOfMemoryError as e:
            row.update({name + "_step_ms": None, name + "_step_peak_mb": None, name + "_error": str(e).split("\n")[0][:300]})
            torch.cuda.empty_cache()
    for k, t in timed_pair(arms, reps).items():
        _ms(row, k + "_step", t)
        row[k + "_last_step_loss"] = float(states[k]["loss"])
    if "native" in arms and "stock" in arms:
        row["step_ratio_native_to_stock"] = round(row["native_step_ms"] / row["stock_step_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="all", choices=["all", "small"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_loss_bench_n1.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shapes = SHAPES if a.shapes == "all" else [s for s in SHAPES if s[0] <= 100_000]
    ops, steps = [], []
    for n, B in shapes:
        for fn, rows in ((bench_op, ops), (bench_step, steps)):
            rows.append(fn(n, B, a.reps, dev))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            hip_ops.softmax_ce_release_workspaces()
            torch.cuda.empty_cache()
    res = {"bench": "softmax_loss", "device": torch.cuda.get_device_name(0), "reps": a.reps, "fp32_matrix_peak_tflops": PEAK_TFLOPS,
           "loss_and_gradients": ops, "sasrec_training_step": steps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
