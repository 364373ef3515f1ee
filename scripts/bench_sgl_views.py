"""SGL's per-epoch view construction, host (--views_native 0) against device (--views_native 1) in one process:
graph_construction() plus the first _graph('sub1') / _graph('sub2') — everything between "the epoch starts" and "both views
can be multiplied" — wall clock with a device sync, 3 warm-ups, median [min, max] of --reps, for ED and ND at ratio 0.1, on
  * the ml-1m-shaped graph of BASELINE.json configs[2] (1.41 M directed edges), and
  * a graph of about 10 M directed edges, where the host arm is run ONCE (no warm-up; it takes most of a minute),
and one SGL fit() epoch on the ml-1m shape with each flag value, for the share of the epoch the views take.
Writes profiles/sgl_views_bench_n1.json and prints it as one JSON line.

    python scripts/bench_sgl_views.py [--reps 10] [--big 1] [--epochs 3] [--out profiles/sgl_views_bench_n1.json]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisprrec_amd import host, runner  # noqa: E402
from whisprrec_amd.sgl import SGL  # noqa: E402

RATIO = 0.1


def log(**kw):
    print(json.dumps(kw), file=sys.stderr, flush=True)


def ml1m_corpus():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_hip_config_shapes import ml1m_shaped_pairs
    uu, ii = ml1m_shaped_pairs()
    return corpus_of(6040, 3706, uu, ii)


def big_corpus(n_users=100_000, n_items=50_000, draws=5_050_000):
    """distinct (user, item) pairs, about 50 per user: ~10 M directed edges"""
    rng = np.random.RandomState(0)
    keys = np.unique(rng.randint(0, n_users, draws).astype(np.int64) * n_items + rng.randint(0, n_items, draws))
    return corpus_of(n_users, n_items, keys // n_items, keys % n_items)


def corpus_of(nU, nI, uu, ii):
    order = np.lexsort((ii, uu))
    uu, ii = uu[order], ii[order]
    ptr = np.zeros(nU + 1, np.int64)
    np.cumsum(np.bincount(uu, minlength=nU), out=ptr[1:])
    sets = {u: set(ii[ptr[u]:ptr[u + 1]].tolist()) for u in range(nU)}
    empty = {"user_id": np.zeros(0, np.int64), "item_id": np.zeros(0, np.int64)}
    return host.Corpus(nU, nI, {"train": {"user_id": uu, "item_id": ii}, "dev": empty, "test": empty}, sets, {u: set() for u in sets})


def model_args(dev, kind, flag, **kw):
    base = dict(device=dev, model_path="/tmp/wr_sgl_views_bench.pt", buffer=1, num_neg=1, test_all=1, embedding_size=64, gcn_layers=2,
                type=kind, reg_weight=1e-4, ssl_tau=0.2, ssl_weight=0.05, drop_ratio=RATIO, ssl_native=1, views_native=flag,
                random_seed=0)
    base.update(kw)
    return argparse.Namespace(**base)


def build_views(m):
    m.graph_construction()
    m._graph("sub1")
    m._graph("sub2")
    torch.cuda.synchronize()


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(float(np.median(ts)), 3), "ms_min_max": [round(min(ts), 3), round(max(ts), 3)], "reps": reps, "warmup": warmup}


def bench_views(name, corpus, dev, reps, host_once):
    out = {"graph": name, "n_users": int(corpus.n_users), "n_items": int(corpus.n_items), "ratio": RATIO}
    for kind in ("ED", "ND"):
        row = {}
        for flag in (0, 1):
            random.seed(1)
            m = SGL(model_args(dev, kind, flag), corpus).to(dev)
            out["directed_edges"] = int(m._edges[0].size)
            once = host_once and flag == 0
            row["views_native_%d" % flag] = timed(lambda: build_views(m), 1 if once else reps, 0 if once else 3)
            if flag == 1:
                assert m._graphs["sub1"] == "device", "the device view builder refused this graph"
            log(graph=name, kind=kind, views_native=flag, **row["views_native_%d" % flag])
            del m
            torch.cuda.empty_cache()
        row["host_over_device"] = round(row["views_native_0"]["ms"] / row["views_native_1"]["ms"], 1)
        row["device_faster"] = row["views_native_1"]["ms"] < row["views_native_0"]["ms"]
        out[kind] = row
    if host_once:
        out["note"] = "views_native_0 was run once, without warm-up, on this graph"
    return out


def bench_epoch(corpus, dev, epochs):
    """SGL fit() epochs through HipRunner with each flag value (ED, device epoch preparation, captured step graph)"""
    B = 2048
    out = {"batch_size": B, "type": "ED"}
    for flag in (0, 1):
        random.seed(1); np.random.seed(1); torch.manual_seed(1)
        args = model_args(dev, "ED", flag, optimizer="Adam", lr=1e-3, l2=0.0, epoch=epochs, check_epoch=1, test_epoch=-1, early_stop=10,
                          batch_size=B, eval_batch_size=2048, num_workers=0, pin_memory=0, topk="10", metric="NDCG",
                          device_epoch_prep=1, hip_graphs=1)
        m = SGL(args, corpus).to(dev)
        ds = SGL.Dataset(m, corpus, "train")
        r = runner.HipRunner(args)
        secs, losses = [], []
        for e in range(epochs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            losses.append(float(r.fit(ds, epoch=e + 1)))
            torch.cuda.synchronize()
            secs.append(round(time.perf_counter() - t0, 4))
        out["views_native_%d" % flag] = {"epoch_seconds": secs, "epoch_seconds_best": min(secs), "losses": losses}
        log(epoch_views_native=flag, **out["views_native_%d" % flag])
        del m, ds, r
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--big", type=int, default=1, choices=[0, 1], help="0: skip the 10 M-edge graph")
    ap.add_argument("--epochs", type=int, default=3, help="SGL fit() epochs per flag value (0 = skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgl_views_bench_n1.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "sgl_views", "device": torch.cuda.get_device_name(0),
           "timed": "graph_construction() + first _graph('sub1') + _graph('sub2'), wall clock with a device sync",
           "baseline": "--views_native 0 in the same process on the same commit (the parent commit has the same host code)",
           "graphs": []}
    small = ml1m_corpus()
    res["graphs"].append(bench_views("ml-1m-shaped (BASELINE.json configs[2])", small, dev, a.reps, host_once=False))
    if a.epochs > 0:
        ep = bench_epoch(small, dev, a.epochs)
        for flag in (0, 1):
            views_s = res["graphs"][0]["ED"]["views_native_%d" % flag]["ms"] / 1e3
            ep["views_native_%d" % flag]["views_share_of_epoch"] = round(views_s / ep["views_native_%d" % flag]["epoch_seconds_best"], 3)
        ep["epoch_ratio_native_to_host"] = round(ep["views_native_1"]["epoch_seconds_best"] / ep["views_native_0"]["epoch_seconds_best"], 3)
        res["sgl_epoch_ml1m"] = ep
    if a.big:
        res["graphs"].append(bench_views("100 K users x 50 K items, ~50 distinct items per user", big_corpus(), dev, a.reps,
                                         host_once=True))
    res["device_faster_everywhere"] = all(g[k]["device_faster"] for g in res["graphs"] for k in ("ED", "ND"))
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
