"""ContraRec's augmented views on the device (--aug_native 1, wr_seq_augment) against the host path, in the same run:
  kernel   hip_ops.seq_augment alone at B in {256, 2,048}, T in {20, 50} (device events);
  host     the same batch through the reference's per-sample path: Dataset._get_feed_dict x B + collate_batch (CPU timer);
  epoch    one HipRunner.fit() epoch of ContraRec on a synthetic ml-1m-shaped sequential corpus (6,040 users, 3,706 items, about a
           million interactions, T = 20, B = 256, --block_native 1 --ccc_native 1) with the flag on, and with the flag off — the
           parent's path, the DataLoader loop — over --off_batches batches of a random subset of the training rows, scaled to the
           epoch's number of batches.  Host clock around fit(), which ends in a device-to-host read of the losses.
3 warm-up calls and the median [min, max] of --reps for the first two; --epoch_reps fits per arm, alternating, for the third.
Prints one JSON line and writes it to --out.

    python scripts/bench_contrarec_aug.py [--reps 20] [--out profiles/contrarec_aug_bench_n1.json]
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisprrec_amd import hip_ops, host  # noqa: E402
from whisprrec_amd import main as launcher  # noqa: E402

N_USERS, N_ITEMS, N_INTER = 6041, 3707, 1_000_209       # ids start at 1, as the reader numbers them


def stats(ts):
    return [round(float(np.median(ts)), 4), round(float(np.min(ts)), 4), round(float(np.max(ts)), 4)]


def timed_device(fn, reps, warmup=3):
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
    return stats(ts)


def timed_host(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def synthetic_corpus(rng, n_inter=N_INTER):
    """ml-1m's shape: every user has at least 20 interactions, the counts are long-tailed, the items popularity-skewed; the last
    two interactions of a user are held out (leave one out), the rest are training rows"""
    n_u = N_USERS - 1
    extra = rng.lognormal(mean=4.0, sigma=1.1, size=n_u)
    counts = 20 + np.floor(extra * (n_inter - 20 * n_u) / extra.sum()).astype(np.int64)
    pop = 1.0 / np.arange(1, N_ITEMS) ** 0.8
    pop /= pop.sum()
    his, clicked, frame = {}, {}, {"user_id": [], "item_id": [], "position": []}
    for u, c in enumerate(counts.tolist(), start=1):
        c = min(c, N_ITEMS - 1)
        items = rng.choice(N_ITEMS - 1, size=c, replace=False, p=pop) + 1
        his[u] = list(zip(items.tolist(), range(c)))
        clicked[u] = set(items[:c - 2].tolist())
        frame["user_id"].append(np.full(c - 2, u, np.int64))
        frame["item_id"].append(items[:c - 2].astype(np.int64))
        frame["position"].append(np.arange(c - 2, dtype=np.int64))
    train = {k: np.concatenate(v) for k, v in frame.items()}
    empty = {k: np.zeros(0, np.int64) for k in frame}
    corpus = host.Corpus(N_USERS, N_ITEMS, {"train": train, "dev": empty, "test": empty}, clicked, {u: set() for u in clicked})
    corpus.user_his = his
    return corpus


def build(corpus, dev, T, B, aug_native):
    argv = ["--model_name", "ContraRec", "--runner_name", "HipRunner", "--batch_size", str(B), "--lr", "1e-3", "--l2", "0.0",
            "--emb_size", "64", "--history_max", str(T), "--num_workers", "0", "--block_native", "1", "--ccc_native", "1",
            "--aug_native", str(aug_native), "--model_path", "/tmp/wr_contrarec_aug_bench.pt", "--log_file", "/tmp/wr_contrarec_aug_bench.txt"]
    args, model_class, _, runner_class = launcher.build_args(argv)
    launcher.init_seed(args.random_seed)
    args.device = dev
    model = model_class(args, corpus).to(dev)
    return model, model_class.Dataset(model, corpus, "train"), runner_class(args)


def bench_batch(a, corpus, dev):
    """the views of one batch: the kernel alone against the per-sample host path that also slices, pads and stacks the batch"""
    rows_out = []
    for T in (20, 50):
        model, data, run = build(corpus, dev, T, 256, 1)
        data.actions_before_epoch()
        hist, lens = run._history_columns(data, dev)
        for B in (256, 2048):
            idx = np.random.RandomState(B + T).randint(0, len(data), size=B)
            rows = torch.from_numpy(idx).to(dev)
            out = (torch.empty((B, hist.shape[1]), dtype=torch.int64, device=dev), torch.empty((B, hist.shape[1]), dtype=torch.int64, device=dev))
            row = {"B": B, "T": T, "table_rows": len(data),
                   "kernel_ms": timed_device(lambda: hip_ops.seq_augment(hist, lens, rows, model.mask_token, 3, 3, 3407, 1, out=out), a.reps),
                   "kernel_with_alloc_ms": timed_device(lambda: hip_ops.seq_augment(hist, lens, rows, model.mask_token, 3, 3, 3407, 1), a.reps),
                   "host_feed_and_collate_ms": timed_host(lambda: data.collate_batch([data[int(i)] for i in idx]), a.reps)}
            row["host_us_per_row"] = round(row["host_feed_and_collate_ms"][0] * 1e3 / B, 2)
            row["ratio_host_to_kernel"] = round(row["host_feed_and_collate_ms"][0] / row["kernel_ms"][0], 1)
            rows_out.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        del model, data, run
    return rows_out


def bench_epoch(a, corpus, dev):
    T, B = 20, 256
    on_model, on_data, on_run = build(corpus, dev, T, B, 1)
    off_model, off_data, off_run = build(corpus, dev, T, B, 0)
    assert on_model.per_sample_feed is False and off_model.per_sample_feed is True
    n = len(on_data)
    n_batches = -(-n // B)
    # the parent's path over a fixed number of batches: a random subset of the training rows, same Dataset class and loop
    keep = np.sort(np.random.RandomState(5).permutation(n)[:a.off_batches * B])
    sub = copy.copy(off_data)
    sub.data = {k: v[keep] for k, v in off_data.data.items()}
    on_ts, off_ts, losses = [], [], {"on": [], "off": []}
    for e in range(a.epoch_reps + 1):                       # the first round of each arm is the warm-up
        for tag in ("off", "on"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = off_run.fit(sub, epoch=e + 1) if tag == "off" else on_run.fit(on_data, epoch=e + 1)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if e > 0:
                (off_ts if tag == "off" else on_ts).append(dt)
            losses[tag].append(round(float(loss), 5))
            print("epoch rep %d %s: %.2f s loss %.4f" % (e, tag, dt, loss), file=sys.stderr, flush=True)
    scale = n_batches / float(a.off_batches)
    off_scaled = [t * scale for t in off_ts]
    res = {"T": T, "B": B, "train_rows": n, "batches_per_epoch": n_batches, "flags": "--block_native 1 --ccc_native 1",
           "aug_native_1_epoch_s": stats(on_ts), "aug_native_1_ms_per_batch": round(float(np.median(on_ts)) * 1e3 / n_batches, 3),
           "aug_native_0_is": "the parent commit's path (DataLoader loop), timed over %d batches of a random %d-row subset of the "
                              "training rows and scaled by %d / %d to the epoch" % (a.off_batches, keep.size, n_batches, a.off_batches),
           "aug_native_0_window_s": stats(off_ts), "aug_native_0_epoch_s_scaled": stats(off_scaled),
           "aug_native_0_ms_per_batch": round(float(np.median(off_ts)) * 1e3 / a.off_batches, 3),
           "ratio_off_to_on": round(float(np.median(off_scaled)) / float(np.median(on_ts)), 3),
           "ratio_off_to_on_spread": [round(min(off_scaled) / max(on_ts), 3), round(max(off_scaled) / min(on_ts), 3)],
           "epoch_losses": losses, "timed_rounds_per_arm": a.epoch_reps, "warmup_rounds_per_arm": 1}
    on_model.check_key_lengths()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--epoch_reps", type=int, default=3)
    ap.add_argument("--off_batches", type=int, default=200)
    ap.add_argument("--interactions", type=int, default=N_INTER)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrarec_aug_bench_n1.json"))
    a = ap.parse_args()
    if a.off_batches < 200:
        raise SystemExit("--off_batches must be at least 200")
    dev = torch.device("cuda:0")
    corpus = synthetic_corpus(np.random.RandomState(0), a.interactions)
    res = {"bench": "contrarec_aug", "device": torch.cuda.get_device_name(0), "reps": a.reps, "ms": "[median, min, max]",
           "corpus": {"users": N_USERS - 1, "items": N_ITEMS - 1, "interactions": int(sum(len(h) for h in corpus.user_his.values()))},
           "batch": bench_batch(a, corpus, dev), "epoch": bench_epoch(a, corpus, dev)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
