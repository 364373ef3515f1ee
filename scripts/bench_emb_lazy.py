"""The row-lazy item table (--emb_lazy, K22) against the dense path, in the same process.

Op level, per (n_items, B, id distribution), D = 64, positions per step = those of one SASRec step at T = 20 (B x 20 history
positions, about half of them padding, + B positives + B negatives):
  dense arm   zero [n_items, D] table + scatter_add_rows + adam_dense          (what one lookup's backward and Adam cost)
  sparse arm  RowLazyTable.step: keys, stable sort, window sweep, sparse step  (index work included)
  gather      gather_rows against RowLazyTable.gather at the same positions
in steady state: --presteps optimizer steps on fresh ids come first, every timed call draws fresh ids, so rows carry the lags
they have in training (a freshly flushed table would replay nothing).  Model level: one SASRec training step (zero_grad, predict,
backward, optimizer step) with --emb_lazy 0 and 1 at the same sizes, and the peak of allocated memory over a step.
Bytes per step are computed from the shapes (not counters), so that a time reads as a fraction of the HBM peak (8 TB/s).
Device events, warm-up, [median, min, max] of --reps, the arms interleaved shape by shape.  Prints one JSON line, writes --out.

    python scripts/bench_emb_lazy.py [--reps 20] [--out profiles/emb_lazy_bench_n1.json]
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
from whisprrec_amd.sasrec import SASRec  # noqa: E402

D, T = 64, 20
N_ITEMS = (3706, 100_000, 1_000_000)
BATCHES = (256, 2048)
HBM_PEAK = 8e12


def timed(fn, reps, warmup=3):
    """fn(i) with a fresh i per call"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ts = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(warmup + i)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return [round(float(np.median(ts)), 4), round(float(np.min(ts)), 4), round(float(np.max(ts)), 4)]


def draw_ids(n_items, shape, dist, gen, dev):
    if dist == "uniform":
        return torch.randint(1, n_items, shape, generator=gen, device=dev)
    # Zipf(1.0) on 1 .. n_items - 1 by inversion of its continuous envelope: P(id <= k) = ln k / ln n
    u = torch.rand(shape, generator=gen, device=dev, dtype=torch.float64)
    return torch.exp(u * float(np.log(n_items))).long().clamp_(1, n_items - 1)


def draw_batch(n_items, B, dist, gen, dev):
    """the feed of one SASRec training step"""
    lens = torch.randint(1, T + 1, (B,), generator=gen, device=dev)
    hist = draw_ids(n_items, (B, T), dist, gen, dev) * (torch.arange(T, device=dev)[None, :] < lens[:, None])
    return {"history_items": hist, "lengths": lens, "pos_item": draw_ids(n_items, (B,), dist, gen, dev),
            "neg_items": draw_ids(n_items, (B, 1), "uniform", gen, dev)}


def positions(fd):
    return torch.cat([fd["history_items"].reshape(-1), fd["pos_item"].reshape(-1), fd["neg_items"].reshape(-1)])


def bench_ops(a, dev, n_items, B, dist):
    gen = torch.Generator(device=dev)
    gen.manual_seed(n_items + B)
    n = B * (T + 2)
    row = {"n_items": n_items, "B": B, "ids": dist, "positions": n, "D": D}
    W = torch.randn(n_items, D, generator=gen, device=dev) * 0.1
    src = torch.randn(n, D, generator=gen, device=dev) * 0.01
    total = a.presteps + 2 * (a.reps + 3)
    ids = [positions(draw_batch(n_items, B, dist, gen, dev)) for _ in range(total)]
    # sparse arm first: its presteps put the table into steady state
    tab = hip_ops.RowLazyTable(W.clone(), "Adam", 1e-3, 0.0, padding_idx=0)
    for i in range(a.presteps):
        tab.step([ids[i]], [src], check=False)
    row["sparse_step_ms"] = timed(lambda i: tab.step([ids[a.presteps + i]], [src], check=False), a.reps)
    row["lazy_gather_ms"] = timed(lambda i: tab.gather(ids[a.presteps + a.reps + 3 + i], check=False), a.reps)
    tab.check()
    lag = tab._lag(n)
    row["max_lag"] = lag
    row["behind"] = tab.behind()
    uniq = int(torch.unique(ids[a.presteps]).numel())
    row["distinct_rows"] = uniq
    row["padding_positions"] = int((ids[a.presteps] == 0).sum())
    window = -(-n_items // lag) if lag else 0
    Wd, m, v, G = W.clone(), torch.zeros_like(W), torch.zeros_like(W), torch.empty_like(W)

    def dense(i):
        G.zero_()
        hip_ops.scatter_add_rows(G, ids[a.presteps + i], src, padding_idx=0)
        hip_ops.adam_dense(Wd, m, v, G, i + 1, 1e-3, 0.0)

    row["dense_step_ms"] = timed(dense, a.reps)
    row["gather_ms"] = timed(lambda i: hip_ops.gather_rows(Wd, ids[a.presteps + a.reps + 3 + i]), a.reps)
    rb = D * 4
    # dense: the table written once (zeros), the gradient rows read and their table rows read and written, then w, g, m, v read
    # and w, m, v written; sparse: ids and keys (8 + 4 B), the sort's pairs twice (4 + 8 B read and written), the gradient rows,
    # and w, m, v of the step's and the window's rows read and written
    row["dense_bytes"] = n_items * rb * 8 + n * (rb + 8) + 2 * uniq * rb
    row["sparse_bytes"] = n * (12 + 2 * 2 * 12 + 12 + rb) + 6 * rb * (uniq + window)
    row["gather_bytes"] = n * (8 + 2 * rb)
    row["lazy_gather_bytes"] = n * (8 + 4 + 4 * rb)
    for k in ("dense", "sparse"):
        row[k + "_hbm_fraction"] = round(row[k + "_bytes"] / (row[k + "_step_ms"][0] * 1e-3) / HBM_PEAK, 4)
    row["step_ratio_sparse_to_dense"] = round(row["sparse_step_ms"][0] / row["dense_step_ms"][0], 3)
    row["gather_ratio_lazy_to_plain"] = round(row["lazy_gather_ms"][0] / row["gather_ms"][0], 3)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def bench_model(a, dev, n_items, B):
    row = {"n_items": n_items, "B": B, "T": T, "ids": "uniform"}
    for flag in (0, 1):
        torch.manual_seed(1)
        gen = torch.Generator(device=dev)
        gen.manual_seed(n_items + B)
        args = argparse.Namespace(device=dev, model_path="/tmp/wr_emb_lazy_bench.pt", buffer=1, num_neg=1, test_all=1, emb_size=D,
                                  num_layers=1, num_heads=4, dropout=0.1, history_max=T, block_native=0, emb_lazy=flag,
                                  optimizer="Adam", lr=1e-3, l2=0.0)
        m = SASRec(args, host.Corpus(13, n_items, {})).to(dev).train()
        if m.optimizer is None:
            m.optimizer = torch.optim.Adam(m.parameters(), lr=1e-3)
        presteps = a.presteps if flag else 3
        fds = [draw_batch(n_items, B, "uniform", gen, dev) for _ in range(presteps + a.reps + 3)]

        def step(i):
            m.optimizer.zero_grad()
            m.predict(fds[i]).backward()
            m.optimizer.step()

        for i in range(presteps):
            step(i)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        tag = "lazy" if flag else "dense"
        row[tag + "_step_ms"] = timed(lambda i: step(presteps + i), a.reps)
        row[tag + "_peak_above_baseline_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2**20, 1)
        if flag:
            m.eval()                          # flushes: raises if an id left the table
        del m, fds
        torch.cuda.empty_cache()
    row["table_mb"] = round(n_items * D * 4 / 2**20, 1)
    row["step_ratio_lazy_to_dense"] = round(row["lazy_step_ms"][0] / row["dense_step_ms"][0], 3)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--presteps", type=int, default=130, help="optimizer steps before the timed ones (2 x MAX_LAG and a few)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emb_lazy_bench_n1.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "emb_lazy", "device": torch.cuda.get_device_name(0), "reps": a.reps, "presteps": a.presteps,
           "ms": "[median, min, max]",
           "note": "ops: dense = zero table + scatter_add_rows + adam_dense, sparse = RowLazyTable.step (keys, stable torch.sort, "
                   "window sweep, sparse step); fresh ids at every call, after `presteps` steps; bytes computed from the shapes, "
                   "hbm_fraction = bytes / median time / 8 TB/s.  model: one SASRec training step, Adam, T = 20, dropout 0.1",
           "ops": [bench_ops(a, dev, n, B, dist) for n in N_ITEMS for B in BATCHES for dist in ("uniform", "zipf")],
           "model": [bench_model(a, dev, n, B) for n in N_ITEMS for B in BATCHES]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
