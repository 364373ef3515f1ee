"""InfoNCE loss + gradient of one side of SGL's calc_ssl_loss: the fused kernels (wr_infonce_loss_grad) against the stock
path (the reference's formula in torch with torch.autograd.grad, what --ssl_native 0 runs), both forward + backward, and a
whole SGL fit() epoch on the ml-1m-shaped graph of BASELINE.json configs[2] with the flag at 0 and at 1.
Device events, warm-up, median of --reps runs.  Prints one JSON line.

    python scripts/bench_infonce.py [--reps 10] [--shapes all|small] [--epochs 3]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisprrec_amd import hip_ops  # noqa: E402

PEAK_TFLOPS = 157.3           # fp32 matrix peak of one MI355X
SHAPES = [  # rows, B, D, tau
    (6_040, 2048, 64, 0.2), (3_706, 2048, 64, 0.2), (100_000, 2048, 64, 0.2), (1_000_000, 2048, 64, 0.2),
]


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


def stock(A, Bm, idx, tau, weight):
    A = A.detach().requires_grad_(True)
    Bm = Bm.detach().requires_grad_(True)
    e1 = F.normalize(A[idx], dim=1)
    e2 = F.normalize(Bm[idx], dim=1)
    all2 = F.normalize(Bm, dim=1)
    v1 = torch.exp(torch.sum(e1 * e2, dim=1) / tau)
    v2 = torch.sum(torch.exp(e1.matmul(all2.T) / tau), dim=1)
    loss = -torch.sum(torch.log(v1 / v2)) * weight
    gA, gB = torch.autograd.grad(loss, [A, Bm])
    return loss.detach(), gA, gB


def bench_op(a, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    shapes = SHAPES if a.shapes == "all" else [s for s in SHAPES if s[0] <= 100_000]
    for n, B, D, tau in shapes:
        A = torch.randn(n, D, device=dev, generator=g) * 0.1
        Bm = A * 0.7 + torch.randn(n, D, device=dev, generator=g) * 0.05
        idx = torch.randint(0, n, (B,), device=dev, generator=g)
        hip_ops.infonce_release_workspaces()
        native_peak = peak_of(lambda: hip_ops.infonce_loss_grad(A, Bm, idx, tau, 0.05, validate=False), dev)
        gA, gB = torch.empty_like(A), torch.empty_like(Bm)
        native_ms = timed(lambda: hip_ops.infonce_loss_grad(A, Bm, idx, tau, 0.05, out=(gA, gB), validate=False), a.reps)
        fwd_ms = timed(lambda: hip_ops.infonce_loss_grad(A, Bm, idx, tau, 0.05, grads=False, validate=False), a.reps)
        # matrix-core work of the native passes: scores + softmax x rows in pass 1, the same again in pass 2
        flop = 4 * 2.0 * B * n * D
        row = dict(rows=n, B=B, D=D, tau=tau, native_ms=round(native_ms[0], 3),
                   native_ms_min_max=[round(native_ms[1], 3), round(native_ms[2], 3)], native_loss_only_ms=round(fwd_ms[0], 3),
                   native_tflops=round(flop / native_ms[0] / 1e9, 1),
                   native_share_of_fp32_matrix_peak=round(flop / native_ms[0] / 1e9 / PEAK_TFLOPS, 3),
                   native_peak_mb=round(native_peak / 2**20, 1),
                   workspace_mb=round(hip_ops.infonce_workspace_bytes(n, B, D) / 2**20, 1),
                   one_score_matrix_mb=round(B * n * 4 / 2**20, 1))
        try:
            stock_peak = peak_of(lambda: stock(A, Bm, idx, tau, 0.05), dev)
            stock_ms = timed(lambda: stock(A, Bm, idx, tau, 0.05), a.reps, warmup=1)
            ln, _, _ = hip_ops.infonce_loss_grad(A, Bm, idx, tau, 0.05, validate=False)
            ls, sA, sB = stock(A, Bm, idx, tau, 0.05)
            row.update(stock_ms=round(stock_ms[0], 3), stock_ms_min_max=[round(stock_ms[1], 3), round(stock_ms[2], 3)],
                       stock_peak_mb=round(stock_peak / 2**20, 1), ratio_to_stock=round(native_ms[0] / stock_ms[0], 3),
                       loss_rel_diff_vs_stock=abs(float(ln[0]) - float(ls)) / abs(float(ls)),
                       gB_rel_diff_vs_stock=float((gB - sB).abs().max() / sB.abs().max()))
            del sA, sB
        except torch.OutOfMemoryError as e:      # expected at a million rows: record it, do not shrink the case
            row.update(stock_ms=None, stock_peak_mb=None, ratio_to_stock=None, stock_error=str(e).split("\n")[0][:300])
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del A, Bm, gA, gB
        hip_ops.infonce_release_workspaces()
        torch.cuda.empty_cache()
    return rows


def bench_epoch(a, dev):
    """SGL fit() epochs through HipRunner on the ml-1m-shaped graph (tests/test_hip_config_shapes.py's generator)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_hip_config_shapes import ml1m_shaped_pairs
    from whisprrec_amd import host, runner
    from whisprrec_amd.sgl import SGL
    nU, nI, B = 6040, 3706, 2048
    uu, ii = ml1m_shaped_pairs()
    ptr = np.zeros(nU + 1, np.int64)
    np.cumsum(np.bincount(uu, minlength=nU), out=ptr[1:])
    sets = {u: set(ii[ptr[u]:ptr[u + 1]].tolist()) for u in range(nU)}
    empty = {"user_id": np.zeros(0, np.int64), "item_id": np.zeros(0, np.int64)}
    corpus = host.Corpus(nU, nI, {"train": {"user_id": uu, "item_id": ii}, "dev": empty, "test": empty}, sets,
                         {u: set() for u in sets})
    out = {"n_users": nU, "n_items": nI, "train_pairs": int(uu.size), "batch_size": B, "steps_per_epoch": -(-int(uu.size) // B)}
    for flag in (0, 1):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        random.seed(1); np.random.seed(1); torch.manual_seed(1)
        args = argparse.Namespace(device=dev, model_path="/tmp/wr_sgl_bench.pt", buffer=1, num_neg=1, test_all=1, embedding_size=64,
                                  gcn_layers=2, type="ED", reg_weight=1e-4, ssl_tau=0.2, ssl_weight=0.05, drop_ratio=0.1,
                                  ssl_native=flag, optimizer="Adam", lr=1e-3, l2=0.0, epoch=a.epochs, check_epoch=1, test_epoch=-1,
                                  early_stop=10, batch_size=B, eval_batch_size=2048, num_workers=0, pin_memory=0, topk="10",
                                  metric="NDCG", device_epoch_prep=1, hip_graphs=1)
        m = SGL(args, corpus).to(dev)
        ds = SGL.Dataset(m, corpus, "train")
        r = runner.HipRunner(args)
        secs, losses = [], []
        for e in range(a.epochs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses.append(float(r.fit(ds, epoch=e + 1)))
            torch.cuda.synchronize()
            secs.append(round(time.perf_counter() - t0, 3))
        out["ssl_native_%d" % flag] = {"epoch_seconds": secs, "epoch_seconds_best": min(secs), "losses": losses,
                                       "peak_mb": round(torch.cuda.max_memory_allocated(dev) / 2**20, 1)}
        print(json.dumps({"ssl_native": flag, **out["ssl_native_%d" % flag]}), file=sys.stderr, flush=True)
        del m, ds, r
        hip_ops.infonce_release_workspaces()
        torch.cuda.empty_cache()
    out["epoch_ratio_native_to_stock"] = round(out["ssl_native_1"]["epoch_seconds_best"] / out["ssl_native_0"]["epoch_seconds_best"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="all", choices=["all", "small"])
    ap.add_argument("--epochs", type=int, default=3, help="SGL fit() epochs per flag value (0 = skip the epoch measurement)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = bench_op(a, dev)
    res = {"bench": "infonce", "device": torch.cuda.get_device_name(0), "reps": a.reps, "fp32_matrix_peak_tflops": PEAK_TFLOPS,
           "rows": rows}
    if a.epochs > 0:
        res["sgl_epoch"] = bench_epoch(a, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
