"""One SASRec training step (zero_grad / predict / backward / Adam step) with the transformer block on stock torch ops
(--block_native 0) and on the fused HIP kernels (--block_native 1, wr_sasblock.hip), in the same process on the same batch.
Device events around each step, warm-up, --reps timed steps per round, --rounds rounds interleaved between the two paths;
reported per path: median, min, max over all timed steps and the spread of the round medians.  Prints one JSON line.

    python scripts/bench_sasblock.py [--reps 30] [--rounds 5] [--warmup 10] [--out profiles/sasblock_bench_n1.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisprrec_amd import host  # noqa: E402
from whisprrec_amd.sasrec import SASRec  # noqa: E402

N_ITEMS, T, D, HEADS = 3706, 20, 64, 4
BATCHES = (2048, 4096)


def make(dev, native, B, dropout, seed=1):
    torch.manual_seed(seed)
    args = argparse.Namespace(device=dev, model_path="/tmp/wr_sas_bench.pt", buffer=1, num_neg=1, test_all=1, emb_size=D, num_layers=1,
                              num_heads=HEADS, dropout=dropout, history_max=T, block_native=native, random_seed=seed)
    m = SASRec(args, host.Corpus(6040, N_ITEMS, {})).to(dev)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    rng = np.random.RandomState(seed)
    lengths = rng.randint(1, T + 1, B)
    hist = rng.randint(1, N_ITEMS, (B, T)) * (np.arange(T)[None, :] < lengths[:, None])
    fd = {"history_items": torch.from_numpy(hist).to(dev), "lengths": torch.from_numpy(lengths).to(dev),
          "pos_item": torch.from_numpy(rng.randint(1, N_ITEMS, B)).to(dev), "neg_items": torch.from_numpy(rng.randint(1, N_ITEMS, (B, 1))).to(dev)}

    def step():
        opt.zero_grad()
        loss = m.predict(fd)
        loss.backward()
        opt.step()
        return loss

    return m, step


def timed(step, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for B in BATCHES:
        paths = {flag: make(dev, flag, B, a.dropout) for flag in (0, 1)}
        assert paths[1][0]._use_block_native(T), "the block kernels refused the benchmark's shape"
        first = {flag: float(paths[flag][1]().detach()) for flag in (0, 1)}     # same init, same batch: losses must agree (dropout aside)
        for flag in (0, 1):
            for _ in range(a.warmup):
                paths[flag][1]()
        torch.cuda.synchronize()
        ts = {0: [], 1: []}
        for _ in range(a.rounds):                                              # interleaved: drift hits both paths alike
            for flag in (0, 1):
                ts[flag].append(timed(paths[flag][1], a.reps))
        row = {"B": B, "T": T, "D": D, "heads": HEADS, "n_items": N_ITEMS, "dropout": a.dropout, "first_loss": first}
        for flag in (0, 1):
            allt = np.concatenate(ts[flag])
            meds = [float(np.median(r)) for r in ts[flag]]
            row["block_native_%d" % flag] = {"step_ms_median": round(float(np.median(allt)), 4), "step_ms_min": round(float(allt.min()), 4),
                                             "step_ms_max": round(float(allt.max()), 4),
                                             "round_medians_ms": [round(v, 4) for v in meds],
                                             "round_median_spread_ms": round(max(meds) - min(meds), 4)}
        row["ratio_native_to_stock"] = round(row["block_native_1"]["step_ms_median"] / row["block_native_0"]["step_ms_median"], 3)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del paths
        torch.cuda.empty_cache()
    res = {"bench": "sasblock", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "warmup": a.warmup,
           "what": "one SASRec training step: zero_grad / predict / backward / Adam step, device events", "rows": rows}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
