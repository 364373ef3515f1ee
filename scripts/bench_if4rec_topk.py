"""Top-K over several interests (wr_topk_recommend_multi, K23) on synthetic tables, D = 64, KQ in {2, 4}, k in {10, 100}, on
(a) 6,040 rows x 3,706 items (ml-1m-shaped) and (b) 200,000 rows x 100,000 items; every row hides about 24 clicked items.
Three arms, wall time with a device synchronize, one warm-up call, then --reps timed calls; reported: median, min, max.
  torch   what a user writes without the kernel: per batch of --batch rows matmul(interests, items^T).max(1), the clicked items
          filled with -inf, torch.topk.  Not run where one batch's matrices exceed --limit_gib; the bytes are recorded instead.
  rows    hip_ops.topk_recommend_rows over the n KQ query rows at the same k: the same scan with KQ times the selection work and
          KQ lists per row — the yardstick of the new consumer.
  multi   hip_ops.topk_recommend_multi, without and with the winner-interest output.
Prints one JSON line.

    python scripts/bench_if4rec_topk.py [--reps 5] [--shapes a,b] [--out profiles/if4rec_topk_bench_n1.json]
"""
import argparse
import json
import os
import sys
from time import perf_counter

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisprrec_amd import hip_ops  # noqa: E402

D = 64
SHAPES = {"a": ("ml-1m-shaped", 6040, 3706), "b": ("200K x 100K", 200_000, 100_000)}
CLICKED = 24


def make_mask(rng, n, n_items):
    """CSR of CLICKED random items per row (ascending, duplicates dropped)"""
    s = np.sort(rng.randint(0, n_items, (n, CLICKED)), axis=1)
    keep = np.ones(s.shape, bool)
    keep[:, 1:] = s[:, 1:] != s[:, :-1]
    ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return ptr, s[keep].astype(np.int32), np.repeat(np.arange(n), keep.sum(axis=1))


def stats(ts):
    ts = np.asarray(ts)
    return {"median_s": round(float(np.median(ts)), 6), "min_s": round(float(ts.min()), 6), "max_s": round(float(ts.max()), 6),
            "all_s": [round(float(t), 6) for t in ts]}


def timed(fn, reps):
    fn()                                                    # warm-up: workspaces, code objects
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(perf_counter() - t0)
    return out


def torch_arm(Q, I, k, ptr, idx, row_of, batch):
    n = Q.shape[0]
    items = torch.empty((n, k), dtype=torch.int64, device=Q.device)
    scores = torch.empty((n, k), dtype=torch.float32, device=Q.device)
    It = I.t()
    for lo in range(0, n, batch):
        hi = min(n, lo + batch)
        S = torch.matmul(Q[lo:hi], It).max(1)[0]
        a, b = int(ptr[lo]), int(ptr[hi])
        S[row_of[a:b] - lo, idx[a:b]] = -float("inf")
        scores[lo:hi], items[lo:hi] = torch.topk(S, k, dim=1)
    return items, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--batch", type=int, default=2048, help="evaluation rows per batch of the torch arm")
    ap.add_argument("--limit_gib", type=float, default=16.0, help="the torch arm is not run when one batch needs more")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for tag in a.shapes.split(","):
        name, n, n_items = SHAPES[tag]
        rng = np.random.RandomState(7)
        I = torch.from_numpy((rng.standard_normal((n_items, D)) * 0.4).astype(np.float32)).to(dev)
        ptr_h, idx_h, row_h = make_mask(rng, n, n_items)
        ptr, idx, row_of = torch.from_numpy(ptr_h).to(dev), torch.from_numpy(idx_h).to(dev), torch.from_numpy(row_h).to(dev)
        mrow = torch.arange(n, dtype=torch.int64, device=dev)
        for KQ in (2, 4):
            Q = torch.from_numpy((rng.standard_normal((n, KQ, D)) * 0.4).astype(np.float32)).to(dev)
            qmat, mrow_q = Q.view(n * KQ, D), mrow.repeat_interleave(KQ).contiguous()
            for k in (10, 100):
                row = {"shape": name, "n": n, "n_items": n_items, "D": D, "KQ": KQ, "k": k, "clicked_per_row": CLICKED}
                # one batch of the torch arm: the [b, KQ, n_items] products, their maximum, topk's values and indices
                b = min(a.batch, n)
                torch_bytes = b * n_items * 4 * (KQ + 1) + b * k * 12
                row["torch_batch_bytes"] = torch_bytes
                if torch_bytes <= a.limit_gib * 2 ** 30:
                    row["torch"] = stats(timed(lambda: torch_arm(Q, I, k, ptr_h, idx, row_of, a.batch), a.reps))
                else:
                    row["torch"] = {"not_run": True, "why": "one batch exceeds --limit_gib %.0f" % a.limit_gib}
                row["rows"] = stats(timed(lambda: hip_ops.topk_recommend_rows(qmat, I, k, mrow_q, ptr, idx), a.reps))
                row["multi"] = stats(timed(lambda: hip_ops.topk_recommend_multi(Q, I, k, mrow, ptr, idx), a.reps))
                row["multi_with_interest"] = stats(timed(lambda: hip_ops.topk_recommend_multi(Q, I, k, mrow, ptr, idx,
                                                                                               with_interest=True), a.reps))
                row["workspace_bytes"] = {"rows": int(hip_ops.abi.lib().wr_topk_workspace_bytes(n * KQ, n_items, D, k)),
                                          "multi": int(hip_ops.abi.lib().wr_topk_multi_workspace_bytes(n, n_items, D, KQ, k))}
                if "median_s" in row["torch"]:
                    row["multi_over_torch"] = round(row["multi"]["median_s"] / row["torch"]["median_s"], 4)
                    ti, _ = torch_arm(Q, I, k, ptr_h, idx, row_of, a.batch)
                    mi, _ = hip_ops.topk_recommend_multi(Q, I, k, mrow, ptr, idx)
                    row["rows_with_torchs_list"] = round(float((ti == mi).all(dim=1).float().mean()), 4)   # rounding of two GEMMs apart
                row["multi_over_rows"] = round(row["multi"]["median_s"] / row["rows"]["median_s"], 4)
                row["rows_spread"] = round((row["rows"]["max_s"] - row["rows"]["min_s"]) / row["rows"]["median_s"], 4)
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
            del Q, qmat
        del I
        torch.cuda.empty_cache()
    out = {"bench": "if4rec_topk", "device": torch.cuda.get_device_name(0), "reps": a.reps, "torch_batch_rows": a.batch,
           "what": "top-K of max over KQ interests, wall seconds with a device synchronize, one warm-up call before the timed ones",
           "rows": rows}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
