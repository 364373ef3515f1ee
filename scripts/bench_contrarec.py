"""ContraRec's native paths against its torch path, in the same run: one training step (predict + backward + Adam) at B = 256
(the reference's usual batch) and 2,048, T = 20, D = 64, with --block_native / --ccc_native both off, each alone and both on; the
contrastive loss alone (forward + backward) at B in {256, 2,048, 4,096}; and the memory of the torch loss's temporaries against
the kernel's workspace.  Device events, warm-up, median of --reps runs.  Prints one JSON line and writes it to --out.

    python scripts/bench_contrarec.py [--reps 20] [--out profiles/contrarec_bench_n1.json]
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
from whisprrec_amd import hip_ops, host  # noqa: E402
from whisprrec_amd.contrarec import ContraRec, contra_loss  # noqa: E402

N_ITEMS, T, D, TAU = 3706, 20, 64, 0.2


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


def make_batch(B, dev, rng):
    lengths = rng.randint(1, T + 1, size=B)
    lengths[0] = T
    hist = np.zeros((3, B, T), np.int64)
    for v in range(3):
        for b in range(B):
            hist[v, b, :lengths[b]] = rng.randint(1, N_ITEMS + (v > 0), size=lengths[b])     # the views may hold the mask token
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return {"history_items": t(hist[0]), "history_items_a": t(hist[1]), "history_items_b": t(hist[2]), "lengths": t(lengths),
            "pos_item": t(rng.randint(1, N_ITEMS, size=B)), "neg_items": t(rng.randint(1, N_ITEMS, size=B)), "phase": "train",
            "batch_size": B}


def bench_step(a, dev):
    rows = []
    for B in (256, 2048):
        fd = make_batch(B, dev, np.random.RandomState(B))
        row = {"B": B, "T": T, "D": D}
        for tag, bn, cn in (("torch", 0, 0), ("block_native", 1, 0), ("ccc_native", 0, 1), ("native", 1, 1)):
            torch.manual_seed(1)
            args = argparse.Namespace(device=dev, model_path="/tmp/wr_contrarec_bench.pt", buffer=1, num_neg=1, test_all=1,
                                      history_max=T, emb_size=D, gamma=1.0, beta_a=3, beta_b=3, ccc_temp=TAU, block_native=bn,
                                      ccc_native=cn)
            m = ContraRec(args, host.Corpus(6040, N_ITEMS, {})).to(dev).train()
            opt = torch.optim.Adam(m.parameters(), lr=1e-3)

            def step():
                opt.zero_grad()
                loss = m.predict(fd)
                loss.backward()
                opt.step()
                return loss

            row[tag + "_step_ms"] = timed(step, a.reps)
            row[tag + "_step_peak_mb"] = round(peak_of(step, dev) / 2**20, 1)
            del m, opt
        row["step_ratio_native_to_torch"] = round(row["native_step_ms"][0] / row["torch_step_ms"][0], 3)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def stock_loss(Fm, labels):
    Fm = Fm.detach().requires_grad_(True)
    B = Fm.shape[0] // 2
    loss = contra_loss(F.normalize(torch.stack([Fm[:B], Fm[B:]], dim=1), dim=-1), labels, TAU)
    (g,) = torch.autograd.grad(loss, [Fm])
    return loss.detach(), g


def bench_loss(a, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for B in (256, 2048, 4096):
        Fm = torch.randn(2 * B, D, device=dev, generator=g)
        labels = torch.randint(1, N_ITEMS, (B,), device=dev, generator=g)
        hip_ops.supcon_release_workspaces()
        row = {"B": B, "D": D, "tau": TAU,
               "native_ms": timed(lambda: hip_ops.supcon_loss_grad(Fm, labels, TAU), a.reps),
               "native_loss_only_ms": timed(lambda: hip_ops.supcon_loss_grad(Fm, labels, TAU, grads=False), a.reps),
               "torch_ms": timed(lambda: stock_loss(Fm, labels), a.reps),
               "workspace_mb": round(hip_ops.supcon_workspace_bytes(B, D) / 2**20, 2),
               "torch_peak_mb": round(peak_of(lambda: stock_loss(Fm, labels), dev) / 2**20, 2),
               "one_score_matrix_mb": round((2 * B) ** 2 * 4 / 2**20, 2)}
        ln, gn = hip_ops.supcon_loss_grad(Fm, labels, TAU)
        ls, gs = stock_loss(Fm, labels)
        row.update(ratio_native_to_torch=round(row["native_ms"][0] / row["torch_ms"][0], 3),
                   loss_rel_diff_vs_torch=abs(float(ln[0]) - float(ls)) / abs(float(ls)),
                   grad_rel_diff_vs_torch=float((gn - gs).abs().max() / gs.abs().max()))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrarec_bench_n1.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "contrarec", "device": torch.cuda.get_device_name(0), "reps": a.reps, "ms": "[median, min, max]",
           "loss": bench_loss(a, dev), "step": bench_step(a, dev)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
