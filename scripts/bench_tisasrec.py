"""TiSASRec's native attention against its torch path, in the same process.  At the ml-1m shape (6,040 users x 3,706 items, D = 64,
4 heads, time_max 512, one block), T in {20, 50} and B in {256, 2,048}: one training step (predict + backward + Adam) with
--ti_native 0 (the reference's own ops: two gathered [B, T, T, D] arrays) and 1 (wr_tiattn.hip, K25) and its peak memory; the
attention alone, forward + backward, from projected q, k, v to the gradients of q, k, v and both time tables (ti_attention_torch
with the interval matrix and the two gathers under autograd against hip_ops.ti_attention).  Timestamps: sessions of a few items
some seconds apart, separated by gaps of days, scaled by per-user minimum intervals — intervals on row 0, on the last row and in
between.  Device events, warm-up, the two arms alternated repetition by repetition, [median, min, max] of --reps runs.  Prints
one JSON line and writes it to --out.

    python scripts/bench_tisasrec.py [--reps 20] [--out profiles/tisasrec_bench_n1.json]
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
from whisprrec_amd.tisasrec import TiSASRec, interval_matrix, ti_attention_torch  # noqa: E402

N_USERS, N_ITEMS, D, HEADS, TIME_MAX = 6040, 3706, 64, 4, 512
SHAPES = [(20, 256), (20, 2048), (50, 256), (50, 2048)]        # (T, B)


class Corpus:
    def __init__(self, user_his):
        self.n_users, self.n_items, self.user_his = N_USERS, N_ITEMS, user_his


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    return [round(float(np.median(ts)), 3), round(float(np.min(ts)), 3), round(float(np.max(ts)), 3)]


def alternated(fns, reps, warmup=3):
    """{tag: [median, min, max] ms} of the functions, run in turn inside every repetition"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {tag: [] for tag in fns}
    for _ in range(reps):
        for tag, fn in fns.items():
            ts[tag].append(once(fn))
    return {tag: stats(v) for tag, v in ts.items()}


def make_model(dev, T, ti_native):
    torch.manual_seed(1)
    rng = np.random.RandomState(2)
    his = {u: [(1, int(t)) for t in np.cumsum(rng.randint(1, 600, 4))] for u in range(N_USERS)}      # scales of 1 .. 599 s
    args = argparse.Namespace(device=dev, model_path="/tmp/wr_tisasrec_bench.pt", buffer=1, num_neg=1, test_all=1, history_max=T,
                              emb_size=D, num_layers=1, num_heads=HEADS, dropout=0.1, time_max=TIME_MAX, ti_native=ti_native,
                              emb_lazy=0, random_seed=1)
    return TiSASRec(args, Corpus(his)).to(dev)


def feed(dev, T, B):
    rng = np.random.RandomState(100 * T + B)
    lens = rng.randint(1, T + 1, size=B)
    valid = np.arange(T)[None, :] < lens[:, None]
    hist = rng.randint(1, N_ITEMS, size=(B, T)) * valid
    # sessions: 70 % of the gaps are seconds, the rest days
    gaps = np.where(rng.random_sample((B, T)) < 0.7, rng.randint(0, 120, (B, T)), rng.randint(86400, 30 * 86400, (B, T)))
    times = (978_300_000 + np.cumsum(gaps, axis=1)) * valid
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return {"history_items": t(hist), "history_times": t(times), "lengths": t(lens), "user_id": t(rng.randint(0, N_USERS, B)),
            "pos_item": t(rng.randint(1, N_ITEMS, size=B)), "neg_items": t(rng.randint(1, N_ITEMS, size=(B, 1))), "batch_size": B,
            "phase": "train"}


def bench_shape(a, dev, T, B):
    fd = feed(dev, T, B)
    row = {"T": T, "B": B, "D": D, "heads": HEADS, "time_max": TIME_MAX, "gathered_array_mb": round(B * T * T * D * 4 / 2**20, 1)}
    models = {"torch": make_model(dev, T, 0).train(), "native": make_model(dev, T, 1).train()}
    for m in models.values():
        m.optimizer = torch.optim.Adam(m.parameters(), lr=1e-3)

    def step_of(m):
        def step():
            m.optimizer.zero_grad()
            loss = m.predict(fd)
            loss.backward()
            m.optimizer.step()
        return step

    for tag, res in alternated({tag: step_of(m) for tag, m in models.items()}, a.reps).items():
        row[tag + "_step_ms"] = res
    for tag, m in models.items():                 # peak memory of one step beyond what is allocated before it
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step_of(m)()
        torch.cuda.synchronize()
        row[tag + "_step_peak_mb"] = round((torch.cuda.max_memory_allocated() - before) / 2**20, 2)
    assert models["native"]._ti_native_ok == {T: True}
    models["native"].check_train_extras()

    # the attention alone: q, k, v as the projections leave them, the model's tables, the batch's timestamps and scales
    m = models["native"]
    gen = torch.Generator(device=dev).manual_seed(3)
    q, k, v, g_out = (torch.randn(B, T, D, device=dev, generator=gen) * s for s in (0.5, 0.5, 0.5, 1.0))
    leaves = [t.requires_grad_(True) for t in (q, k, v)] + [m.time_k_embedding.weight, m.time_v_embedding.weight]
    times, scale = fd["history_times"], m.min_interval[fd["user_id"]]
    mask = torch.tril(torch.ones(1, 1, T, T, dtype=torch.int32, device=dev))

    def clear():
        for t in leaves:
            t.grad = None

    def attn_torch():
        clear()
        R = interval_matrix(times, scale, TIME_MAX)
        emb = torch.nn.functional.embedding          # nn.Embedding's lookup and backward, as in the model
        ti_attention_torch(q, k, v, emb(R, leaves[3]), emb(R, leaves[4]), mask, HEADS).backward(g_out)

    def attn_native():
        clear()
        hip_ops.ti_attention(q, k, v, times, scale, leaves[3], leaves[4], HEADS, TIME_MAX).backward(g_out)

    for tag, res in alternated({"torch": attn_torch, "native": attn_native}, a.reps).items():
        row[tag + "_attn_fwd_bwd_ms"] = res
    clear()
    row["attn_workspace_mb"] = round(hip_ops.ti_attention_workspace_bytes(B, T, D, HEADS, TIME_MAX) / 2**20, 2)
    for key in ("step", "attn_fwd_bwd"):
        row[key + "_ratio_native_to_torch"] = round(row["native_%s_ms" % key][0] / row["torch_%s_ms" % key][0], 3)
    row["step_peak_ratio_native_to_torch"] = round(row["native_step_peak_mb"] / row["torch_step_peak_mb"], 4)
    print(json.dumps(row), file=sys.stderr, flush=True)
    del models
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tisasrec_bench_n1.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "tisasrec", "device": torch.cuda.get_device_name(0), "reps": a.reps, "ms": "[median, min, max]",
           "note": "step = zero_grad + predict + backward + torch.optim.Adam.step, dropout 0.1, one block; the torch arm is the "
                   "reference layer's own ops (two gathered [B, T, T, D] arrays); attn_fwd_bwd = from projected q, k, v to the "
                   "gradients of q, k, v and both time tables, interval matrix and gathers included in the torch arm; the arms "
                   "alternate inside every repetition; peak_mb = peak allocation of one step beyond the model and optimizer "
                   "state; the native arm's kernel workspace (attn_workspace_mb) is allocated once, at the first step, and is not in it",
           "shapes": [bench_shape(a, dev, T, B) for T, B in SHAPES]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
