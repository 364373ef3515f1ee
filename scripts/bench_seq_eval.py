"""HipRunner.evaluate of SASRec on a sequential dataset: the host loop (--seq_eval_native 0: per-sample collate, one
[B, n_items] matrix per batch, concatenation, copy to the host, Python masking loop, NumPy argsort) against the device path
(--seq_eval_native 1: histories by array work, queries in chunks, one wr_rank_eval_rows call), each with --block_native 0 and 1,
on two synthetic corpora: (a) ml-1m-shaped, 6,040 evaluation rows x 3,706 items, (b) 200,000 rows x 100,000 items.
Wall time around evaluate() with a device synchronize, one warm-up call (it also builds the caches: histories, mask CSR), then
--reps timed calls; reported: median, min, max.  The device path is also timed piece by piece (histories, queries, uploads,
rank kernel, read-back).  Where the host path's matrices would not fit (--host_limit_gib) it is not run and the bytes it would
need are recorded.  Prints one JSON line.

    python scripts/bench_seq_eval.py [--reps 5] [--corpora a,b] [--out profiles/seq_eval_bench_n1.json]
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
from whisprrec_amd import hip_ops, host, runner  # noqa: E402
from whisprrec_amd.sasrec import SASRec  # noqa: E402

T, D, HEADS, LAYERS = 20, 64, 4, 1
CORPORA = {"a": ("ml-1m-shaped", 6040, 3706), "b": ("200K x 100K", 200_000, 100_000)}
HIS_LEN = 25                                  # items per user: T history items and more before the evaluation row


def make_corpus(n_rows, n_items, seed=1):
    """one evaluation row per user: the last of HIS_LEN interactions is the target, the ones before it are training items"""
    rng = np.random.RandomState(seed)
    seq = rng.randint(1, n_items, (n_rows, HIS_LEN))
    times = list(range(HIS_LEN))
    his, tcs, rcs = {}, {}, {}
    for u, row in enumerate(seq.tolist()):
        his[u] = list(zip(row, times))
        tcs[u] = set(row[:-1])
        rcs[u] = {row[-1]}
    frame = {"user_id": np.arange(n_rows), "item_id": seq[:, -1].copy(), "position": np.full(n_rows, HIS_LEN - 1)}
    corpus = host.Corpus(n_rows, n_items, {"dev": frame}, tcs, rcs)
    corpus.user_his = his
    return corpus


def make_args(dev, block_native, seq_eval_native, eval_batch_size):
    return argparse.Namespace(device=dev, model_path="/tmp/wr_seq_eval_bench.pt", buffer=1, num_neg=1, test_all=1, emb_size=D,
                              num_layers=LAYERS, num_heads=HEADS, dropout=0.1, history_max=T, block_native=block_native,
                              random_seed=1, epoch=1, check_epoch=1, test_epoch=-1, early_stop=10, lr=1e-3, l2=0.0,
                              batch_size=2048, eval_batch_size=eval_batch_size, optimizer="Adam", num_workers=0, pin_memory=0,
                              topk="10,20", metric="NDCG, HR", seq_eval_native=seq_eval_native)


def stats(ts):
    ts = np.asarray(ts)
    return {"median_s": round(float(np.median(ts)), 5), "min_s": round(float(ts.min()), 5), "max_s": round(float(ts.max()), 5),
            "all_s": [round(float(t), 5) for t in ts]}


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(perf_counter() - t0)
    return out


def device_pieces(run, ds, reps):
    """rank_rows step by step, a synchronize after each piece"""
    model = ds.model
    dev = next(model.parameters()).device
    names = ("histories", "queries", "uploads", "rank_kernel", "read_back")
    ts = {k: [] for k in names}

    def lap(name, t0):
        torch.cuda.synchronize()
        ts[name].append(perf_counter() - t0)
        return perf_counter()

    for _ in range(reps):
        torch.cuda.synchronize()
        t = perf_counter()
        model.eval()
        run._history_columns(ds, dev)
        t = lap("histories", t)
        queries = run._row_queries(ds)
        t = lap("queries", t)
        ptr, idx = run._clicked_mask(ds.corpus, True, model.user_num, dev)
        et = torch.from_numpy(np.ascontiguousarray(ds.data["item_id"])).to(torch.int64).to(dev)
        mrow = torch.from_numpy(np.ascontiguousarray(ds.data["user_id"])).to(torch.int64).to(dev)
        items = model.eval_items().detach().contiguous()
        t = lap("uploads", t)
        rank, _ = hip_ops.rank_eval_rows(queries, items, et, mrow, ptr, idx)
        t = lap("rank_kernel", t)
        rank.cpu().numpy().astype(np.int64)
        lap("read_back", t)
    return {k: round(float(np.median(v)), 6) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--corpora", default="a,b")
    ap.add_argument("--eval_batch_size", type=int, default=2048)
    ap.add_argument("--host_limit_gib", type=float, default=16.0, help="the host path is not run above this many GiB")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for tag in a.corpora.split(","):
        name, n_rows, n_items = CORPORA[tag]
        t0 = perf_counter()
        corpus = make_corpus(n_rows, n_items)
        build_s = perf_counter() - t0
        # the host path holds the per-batch matrices, their concatenation on the device, its host copy and the
        # [n, 1 + n_items] result, then the argsort's int64 order: 4 float copies + 8 B per entry at the peak
        host_bytes = int(n_rows) * (1 + int(n_items)) * (4 * 4 + 8)
        for block_native in (0, 1):
            torch.manual_seed(1)
            model = SASRec(make_args(dev, block_native, 0, a.eval_batch_size), corpus).to(dev)
            ds = SASRec.Dataset(model, corpus, "dev")
            row = {"corpus": name, "n_eval": n_rows, "n_items": n_items, "D": D, "T": T, "heads": HEADS, "layers": LAYERS,
                   "block_native": block_native, "eval_batch_size": a.eval_batch_size, "corpus_build_s": round(build_s, 3)}
            res = {}
            if host_bytes <= a.host_limit_gib * 2 ** 30:
                run0 = runner.HipRunner(make_args(dev, block_native, 0, a.eval_batch_size))
                res[0] = run0.evaluate(ds, [10, 20], ["NDCG", "HR"])                        # warm-up
                row["seq_eval_native_0"] = stats(timed(lambda: run0.evaluate(ds, [10, 20], ["NDCG", "HR"]), a.reps))
            else:
                row["seq_eval_native_0"] = {"not_run": True, "bytes_needed": host_bytes,
                                            "score_matrix_bytes": int(n_rows) * int(n_items) * 4,
                                            "why": "the [n_eval, n_items] matrices of the host path exceed --host_limit_gib %.0f"
                                                   % a.host_limit_gib}
            run1 = runner.HipRunner(make_args(dev, block_native, 1, a.eval_batch_size))
            assert run1._seq_eval_ok(ds), "the device path refused the benchmark's shape"
            first = timed(lambda: res.__setitem__(1, run1.evaluate(ds, [10, 20], ["NDCG", "HR"])), 1)[0]   # builds the caches
            if block_native:
                assert model._block_native_ok and all(model._block_native_ok.values()), "the block kernels refused the shape"
            row["seq_eval_native_1"] = stats(timed(lambda: run1.evaluate(ds, [10, 20], ["NDCG", "HR"]), a.reps))
            row["seq_eval_native_1"]["first_call_s"] = round(first, 4)                       # histories + mask CSR built here
            row["seq_eval_native_1"]["pieces_median_s"] = device_pieces(run1, ds, a.reps)
            if 0 in res:
                row["metrics_max_abs_diff"] = float(max(abs(res[0][k] - res[1][k]) for k in res[0]))
                row["ratio_device_to_host"] = round(row["seq_eval_native_1"]["median_s"] / row["seq_eval_native_0"]["median_s"], 5)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del model, ds, run1
            torch.cuda.empty_cache()
        del corpus
    out = {"bench": "seq_eval", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "what": "HipRunner.evaluate(dev rows, topk 10,20, NDCG+HR) of SASRec, wall seconds with a device synchronize; one "
                   "warm-up call before the timed ones", "rows": rows}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
