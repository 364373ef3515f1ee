"""BUIR's native path against its torch path, in the same process: one training step (predict + backward + Adam + target update)
with --buir_native 0 and 1; the loss and its gradients alone (K16, wr_buir_loss_grad, the dense table gradients included, against
torch ops + autograd); and the target update alone (K17, wr_ema_update, against torch's three launches per table).  Shapes:
6,040 x 3,706 at B = 2,048 and 1M x 1M at B = 65,536, D = 64.  Device events, warm-up, median of --reps runs, the two arms
interleaved shape by shape.  Prints one JSON line and writes it to --out.

    python scripts/bench_buir.py [--reps 20] [--out profiles/buir_bench_n1.json]
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
from whisprrec_amd.buir import BUIR  # noqa: E402

D = 64
SHAPES = [(6040, 3706, 2048), (1_000_000, 1_000_000, 65536)]


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return [round(float(np.median(ts)), 3), round(float(np.min(ts)), 3), round(float(np.max(ts)), 3)]


def make_model(n_users, n_items, native, dev):
    torch.manual_seed(1)
    args = argparse.Namespace(device=dev, model_path="/tmp/wr_buir_bench.pt", buffer=1, num_neg=1, test_all=1, embedding_size=D,
                              momentum=0.995, buir_native=native)
    return BUIR(args, host.Corpus(n_users, n_items, {})).to(dev).train()


def stock_loss_grads(m, fd):
    m.zero_grad(set_to_none=True)
    loss = m.predict(fd)
    loss.backward()
    return loss


def bench_shape(a, dev, n_users, n_items, B):
    rng = np.random.RandomState(B)
    fd = {"user_id": torch.from_numpy(rng.randint(0, n_users, size=B)).to(dev),
          "pos_item": torch.from_numpy(rng.randint(1, n_items, size=B)).to(dev), "batch_size": B, "phase": "train"}
    row = {"n_users": n_users, "n_items": n_items, "B": B, "D": D}
    for tag, native in (("torch", 0), ("native", 1)):
        m = make_model(n_users, n_items, native, dev)
        m.optimizer = torch.optim.Adam(m.parameters(), lr=1e-3)

        def step():
            m.optimizer.zero_grad()
            loss = m.predict(fd)
            loss.backward()
            m.optimizer.step()                       # the step post hook runs _update_target()
            return loss

        row[tag + "_step_ms"] = timed(step, a.reps)
        m.optimizer = None
        row[tag + "_loss_grad_ms"] = timed(lambda: stock_loss_grads(m, fd), a.reps)
        row[tag + "_update_target_ms"] = timed(m._update_target, a.reps)
        if native:
            assert m._buir_native_ok is True
            m.check_ids()
            W = (m.user_online.weight, m.item_online.weight, m.user_target.weight, m.item_target.weight, m.predictor.weight,
                 m.predictor.bias)
            w = [t.detach() for t in W]
            row["kernel_loss_grad_ms"] = timed(lambda: hip_ops.buir_loss_grad(*w, fd["user_id"], fd["pos_item"]), a.reps)
            row["kernel_loss_only_ms"] = timed(lambda: hip_ops.buir_loss_grad(*w, fd["user_id"], fd["pos_item"], grads=False), a.reps)
            row["workspace_mb"] = round(hip_ops.buir_workspace_bytes(B, D) / 2**20, 2)
        del m
        torch.cuda.empty_cache()
    for k in ("step", "loss_grad", "update_target"):
        row[k + "_ratio_native_to_torch"] = round(row["native_%s_ms" % k][0] / row["torch_%s_ms" % k][0], 3)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "buir_bench_n1.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "buir", "device": torch.cuda.get_device_name(0), "reps": a.reps, "ms": "[median, min, max]",
           "note": "step = zero_grad + predict + backward + torch.optim.Adam.step + target update; loss_grad = predict + backward "
                   "(dense table gradients included); kernel_* = wr_buir_loss_grad alone (per-sample row gradients)",
           "shapes": [bench_shape(a, dev, *s) for s in SHAPES]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
