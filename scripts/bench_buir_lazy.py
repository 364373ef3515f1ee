"""BUIR's row-lazy tables (--emb_lazy 1, K24) against the dense path (--emb_lazy 0), both under --buir_native 1, in one process.

One training step (zero_grad, predict, backward, optimizer step, target update) per arm; the --emb_lazy 0 arm is the baseline.
Shapes: 6,040 x 3,706 at B = 2,048 and 1M x 1M at B = 65,536 (scripts/bench_buir.py's two) and 1M x 1M at B = 2,048 (the bounded
lag is active there), D = 64; Adam and SGD (lr 1e-3, l2 0, momentum 0.995).  Steady state: --presteps training steps on fresh ids
come first, and every timed call draws fresh ids, so the rows carry the lags they have in training.  Device events, 3 warm-up
calls, [median, min, max] of --reps, the two arms alternating call by call.  Also: the parts of the lazy step (two gathers, loss
kernel, keys + sort, rotating window, two sparse steps) timed one by one in the same state; the peak of allocated memory over a
step above the resting level; behind() of both tables at the end.  Prints one JSON line, writes --out.

    python scripts/bench_buir_lazy.py [--reps 20] [--presteps 130] [--out profiles/buir_lazy_bench_n1.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisprrec_amd import hip_ops, host  # noqa: E402
from whisprrec_amd.buir import BUIR, BuirLazyOptimizer  # noqa: E402

D = 64
SHAPES = [(6040, 3706, 2048), (1_000_000, 1_000_000, 65536), (1_000_000, 1_000_000, 2048)]
LR = 1e-3


def stats(ts):
    return [round(float(np.median(ts)), 4), round(float(np.min(ts)), 4), round(float(np.max(ts)), 4)]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def make_model(n_users, n_items, opt, lazy, dev):
    torch.manual_seed(1)
    args = argparse.Namespace(device=dev, model_path="/tmp/wr_buir_lazy_bench.pt", buffer=1, num_neg=1, test_all=1, embedding_size=D,
                              momentum=0.995, buir_native=1, emb_lazy=lazy, optimizer=opt, lr=LR, l2=0.0)
    m = BUIR(args, host.Corpus(n_users, n_items, {})).to(dev).train()
    if lazy:
        assert isinstance(m.optimizer, BuirLazyOptimizer)
    else:
        m.optimizer = getattr(torch.optim, opt)(m.parameters(), lr=LR, weight_decay=0.0)
    return m


def bench(a, dev, n_users, n_items, B, opt):
    gen = torch.Generator(device=dev)
    gen.manual_seed(B + n_users)

    def feed():
        return {"user_id": torch.randint(0, n_users, (B,), generator=gen, device=dev),
                "pos_item": torch.randint(0, n_items, (B,), generator=gen, device=dev), "batch_size": B, "phase": "train"}

    def step(m):
        fd = feed()
        m.optimizer.zero_grad()
        loss = m.predict(fd)
        loss.backward()
        m.optimizer.step()
        return loss

    row = {"n_users": n_users, "n_items": n_items, "B": B, "D": D, "optimizer": opt}
    dense, lazy = make_model(n_users, n_items, opt, 0, dev), make_model(n_users, n_items, opt, 1, dev)
    for _ in range(a.presteps):
        step(lazy)
    for _ in range(3):
        step(dense)
        step(lazy)
    torch.cuda.synchronize()
    td, tl = [], []
    for _ in range(a.reps):                              # the arms alternate
        td.append(event_ms(lambda: step(dense))[0])
        tl.append(event_ms(lambda: step(lazy))[0])
    row["dense_step_ms"], row["lazy_step_ms"] = stats(td), stats(tl)
    row["lazy_over_dense"] = round(row["lazy_step_ms"][0] / row["dense_step_ms"][0], 3)

    # the parts of the lazy step, in the state the timed steps left: each part of a real step, step after step
    ut, it = lazy.optimizer.tables()
    W, b = lazy.predictor.weight.detach(), lazy.predictor.bias.detach()
    pos = torch.arange(B, device=dev)
    parts = {k: [] for k in ("gathers", "loss_kernel", "keys_sort", "window", "sparse_steps")}
    for _ in range(3 + a.reps):
        fd = feed()
        u, i = fd["user_id"], fd["pos_item"]
        ms, (ru, ri) = event_ms(lambda: (ut.gather(u, check=False), it.gather(i, check=False)))
        parts["gathers"].append(ms)
        ms, out = event_ms(lambda: hip_ops.buir_loss_grad(ru[0], ri[0], ru[1], ri[1], W, b, pos, pos))
        parts["loss_kernel"].append(ms)
        ms, (ou, oi) = event_ms(lambda: (ut._order([u], [out[1]], False), it._order([i], [out[2]], False)))
        parts["keys_sort"].append(ms)
        ms, _ = event_ms(lambda: (ut._window(B, ut.t + 1), it._window(B, it.t + 1)))
        parts["window"].append(ms)
        ms, _ = event_ms(lambda: (ut._apply(*ou, ut.t + 1), it._apply(*oi, it.t + 1)))
        parts["sparse_steps"].append(ms)
        ut.t, it.t = ut.t + 1, it.t + 1
    row["lazy_parts_ms"] = {k: stats(v[3:]) for k, v in parts.items()}
    row["max_lag"] = [ut._lag(B), it._lag(B)]

    for tag, m in (("dense", dense), ("lazy", lazy)):
        torch.cuda.synchronize()
        rest = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(3):
            step(m)
        torch.cuda.synchronize()
        row[tag + "_peak_above_rest_mb"] = round((torch.cuda.max_memory_allocated() - rest) / 2**20, 2)
    row["table_mb"] = round(max(n_users, n_items) * D * 4 / 2**20, 2)
    row["behind_at_end"] = [ut.behind(), it.behind()]
    row["steps_taken"] = ut.t
    lazy.eval()                                          # flushes; raises if an id left a table
    assert ut.behind() == 0 and it.behind() == 0
    print(json.dumps(row), file=sys.stderr, flush=True)
    del dense, lazy
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--presteps", type=int, default=130)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "buir_lazy_bench_n1.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "buir_lazy", "device": torch.cuda.get_device_name(0), "reps": a.reps, "presteps": a.presteps,
           "ms": "[median, min, max]",
           "note": "step = zero_grad + predict + backward + optimizer step + target update, --buir_native 1, fresh ids at every call; "
                   "dense = --emb_lazy 0 (the baseline), lazy = --emb_lazy 1; lazy_parts_ms: the parts of a lazy step timed one by "
                   "one (their sum leaves out autograd and the predictor's torch.optim step)",
           "rows": [bench(a, dev, *s, opt) for s in SHAPES for opt in ("Adam", "SGD")]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
