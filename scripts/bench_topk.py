"""Top-K recommendation (wr_topk_recommend) against full-ranking evaluation (wr_rank_eval) at the same shape and against
the blocked torch code a user would otherwise write, per block of rows:
    torch.topk((U[u] @ I.T).masked_fill_(mask, -inf), k)
Device events, warm-up, median of --reps runs.  Prints one JSON line.

    python scripts/bench_topk.py [--reps 10] [--shapes all|small]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisprrec_amd import hip_ops  # noqa: E402

SHAPES = [  # n_users, n_items, D, k
    (100_000, 100_000, 64, 10), (100_000, 100_000, 64, 20), (100_000, 100_000, 64, 100), (100_000, 100_000, 64, 256),
    (20_000, 1_000_000, 64, 100), (6_040, 3_706, 64, 100),
]
CLICKS_PER_USER = 50      # masked (already clicked) items per user


def timed(fn, reps, warmup=2):
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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch_block", type=int, default=2048)
    ap.add_argument("--shapes", default="all", choices=["all", "small"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    shapes = SHAPES if a.shapes == "all" else [s for s in SHAPES if s[0] * s[1] <= 1e9]
    for n, n_items, D, k in shapes:
        U = torch.randn(n, D, device=dev, generator=g) * 0.3
        I = torch.randn(n_items, D, device=dev, generator=g) * 0.3
        users = torch.arange(n, device=dev)
        cu = torch.arange(n, device=dev).repeat_interleave(CLICKS_PER_USER)
        ci = torch.randint(0, n_items, (n * CLICKS_PER_USER,), device=dev, generator=g)
        ptr, idx = hip_ops.clicked_csr_from_pairs(cu, ci, n, n_items)
        targets = torch.randint(0, n_items, (n,), device=dev, generator=g)
        topk_ms = timed(lambda: hip_ops.topk_recommend(U, I, users, k, ptr, idx), a.reps)
        rank_ms = timed(lambda: hip_ops.rank_eval(U, I, users, targets, ptr, idx), a.reps)
        blk = a.torch_block
        rows_of = torch.repeat_interleave(torch.arange(n, device=dev), ptr[1:] - ptr[:-1])

        def torch_baseline():
            out = []
            for lo in range(0, n, blk):
                hi = min(n, lo + blk)
                s = U[users[lo:hi]] @ I.T
                mask = torch.zeros(hi - lo, n_items, dtype=torch.bool, device=dev)
                p0, p1 = int(ptr[lo]), int(ptr[hi])
                mask[rows_of[p0:p1] - lo, idx[p0:p1].long()] = True
                out.append(torch.topk(s.masked_fill_(mask, float("-inf")), k, dim=1))
            return out
        torch_ms = timed(torch_baseline, a.reps, warmup=1)
        # the same answers on the first rows (scores up to the fp32 rounding of the two GEMMs)
        _, sc = hip_ops.topk_recommend(U, I, users[:256], k, ptr, idx)
        s = U[:256] @ I.T
        mask = torch.zeros(256, n_items, dtype=torch.bool, device=dev)
        mask[rows_of[:int(ptr[256])], idx[:int(ptr[256])].long()] = True
        ref = torch.topk(s.masked_fill_(mask, float("-inf")), k, dim=1).values
        agree = float((sc - ref).abs().max() / ref.abs().max())
        flop = 2.0 * n * n_items * D
        rows.append(dict(n_users=n, n_items=n_items, D=D, k=k, topk_ms=round(topk_ms[0], 3),
                         topk_ms_min_max=[round(topk_ms[1], 3), round(topk_ms[2], 3)], rank_eval_ms=round(rank_ms[0], 3),
                         torch_ms=round(torch_ms[0], 3), topk_tflops=round(flop / topk_ms[0] / 1e9, 1),
                         rank_eval_tflops=round(flop / rank_ms[0] / 1e9, 1),
                         ratio_to_rank_eval=round(topk_ms[0] / rank_ms[0], 3),
                         ratio_to_torch=round(topk_ms[0] / torch_ms[0], 3), max_rel_score_diff_vs_torch=agree))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        del U, I, ptr, idx, rows_of
        torch.cuda.empty_cache()
    print(json.dumps({"bench": "topk", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
