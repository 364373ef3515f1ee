"""IF4Rec's native paths against its torch path, in the same process.  At the ml-1m shape (6,040 users x 3,706 items, T = 20,
D = 64, A = 8, K = 2, one block of 4 heads) and B = 256, 2,048, 4,096: one training step (predict + backward + Adam) with
--interest_native 0 and 1 and its peak memory; the interest pooling alone, forward + backward (K18 against torch ops + autograd,
the dense table gradients included).  Then `evaluate` over 6,040 rows x 3,706 items with --seq_eval_native 0 (host loop over
full_predict) and 1 (wr_rank_eval_multi, K19), and the device ranking of 200,000 rows against 100,000 items (interests in chunks
of eval_batch_size + one wr_rank_eval_multi call), which has no host counterpart worth waiting for.  Device events, warm-up, the
two arms alternated repetition by repetition, [median, min, max] of --reps runs.  Prints one JSON line and writes it to --out.

    python scripts/bench_if4rec.py [--reps 10] [--out profiles/if4rec_bench_n1.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisprrec_amd import hip_ops, host, runner  # noqa: E402
from whisprrec_amd import main as launcher  # noqa: E402
from whisprrec_amd.if4rec import IF4Rec  # noqa: E402

N_USERS, N_ITEMS, T, D, A, K, HEADS = 6040, 3706, 20, 64, 8, 2, 4
BATCHES = [256, 2048, 4096]


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


def make_model(dev, n_items=N_ITEMS, **kw):
    torch.manual_seed(1)
    base = dict(device=dev, model_path="/tmp/wr_if4rec_bench.pt", buffer=1, num_neg=1, test_all=1, history_max=T, emb_size=D,
                attn_size=A, K=K, add_pos=1, encoder_layer=1, n_head=HEADS, encoder_dropout=0.0, add_multi=1, interest_native=0,
                block_native=0, random_seed=1)
    base.update(kw)
    return IF4Rec(argparse.Namespace(**base), host.Corpus(N_USERS, n_items, {})).to(dev)


def histories(rng, n, n_items):
    lens = rng.randint(1, T + 1, size=n)
    hist = rng.randint(1, n_items, size=(n, T)) * (np.arange(T)[None, :] < lens[:, None])
    return hist.astype(np.int64), lens.astype(np.int64)


def bench_batch(a, dev, B):
    rng = np.random.RandomState(B)
    hist, lens = histories(rng, B, N_ITEMS)
    fd = {"history_items": torch.from_numpy(hist).to(dev), "lengths": torch.from_numpy(lens).to(dev),
          "pos_item": torch.from_numpy(rng.randint(1, N_ITEMS, size=B)).to(dev),
          "neg_items": torch.from_numpy(rng.randint(1, N_ITEMS, size=(B, 1))).to(dev), "batch_size": B, "phase": "train"}
    row = {"B": B, "T": T, "D": D, "A": A, "K": K, "n_head": HEADS}
    models = {"torch": make_model(dev).train(), "native": make_model(dev, interest_native=1).train()}
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
    assert models["native"]._interest_native_ok == {T: True}
    models["native"].check_history_ids()

    g_out = torch.randn(B, K, D, device=dev)

    def pool_of(m):
        def pool():
            m.zero_grad(set_to_none=True)
            m.add_multi, keep = 0, m.add_multi          # the pooling alone: forward() without the blocks
            try:
                out = m.forward(fd)
            finally:
                m.add_multi = keep
            out.backward(g_out)
        return pool

    for tag, res in alternated({tag: pool_of(m) for tag, m in models.items()}, a.reps).items():
        row[tag + "_pool_fwd_bwd_ms"] = res
    row["pool_workspace_mb"] = round(hip_ops.interest_pool_workspace_bytes(B, D, A, K, T) / 2**20, 2)
    for k in ("step", "pool_fwd_bwd"):
        row[k + "_ratio_native_to_torch"] = round(row["native_%s_ms" % k][0] / row["torch_%s_ms" % k][0], 3)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def eval_corpus(rng):
    """6,040 users with a history of 20 items and one dev row each"""
    his, dev_u, dev_i, clicked = {}, [], [], {}
    for u in range(1, N_USERS):
        seq = rng.randint(1, N_ITEMS, size=T + 1)
        his[u] = [(int(i), t) for t, i in enumerate(seq)]
        clicked[u] = set(int(i) for i in seq[:T]) - {int(seq[T])}
        dev_u.append(u)
        dev_i.append(int(seq[T]))
    frame = {"user_id": np.asarray(dev_u), "item_id": np.asarray(dev_i), "position": np.full(len(dev_u), T)}
    corpus = host.Corpus(N_USERS, N_ITEMS, {"dev": frame}, train_clicked_set=clicked,
                         residual_clicked_set={u: set() for u in clicked})
    corpus.user_his = his
    return corpus


def bench_evaluate(a, dev):
    corpus = eval_corpus(np.random.RandomState(7))
    model = make_model(dev, interest_native=1).eval()
    ds = IF4Rec.Dataset(model, corpus, "dev")
    fns = {}
    for tag, flag in (("host", "0"), ("device", "1")):
        args = launcher.build_args(["--model_name", "IF4Rec", "--runner_name", "HipRunner", "--seq_eval_native", flag,
                                    "--eval_batch_size", "2048"])[0]
        run = runner.HipRunner(args)
        if flag == "1":
            assert run._seq_eval_ok(ds)
        fns[tag] = (lambda r: lambda: r.evaluate(ds, [5, 10], ["NDCG", "HR"]))(run)
    row = {"rows": len(ds), "n_items": N_ITEMS, "K": K, "D": D}
    for tag, res in alternated(fns, max(a.reps // 2, 3), warmup=1).items():
        row["evaluate_%s_ms" % tag] = res
    row["evaluate_ratio_device_to_host"] = round(row["evaluate_device_ms"][0] / row["evaluate_host_ms"][0], 4)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def bench_rank_large(a, dev, n=200_000, n_items=100_000):
    rng = np.random.RandomState(9)
    model = make_model(dev, n_items=n_items, interest_native=1).eval()
    hist, lens = histories(rng, n, n_items)
    hist, lens = torch.from_numpy(hist).to(dev), torch.from_numpy(lens).to(dev)
    target = torch.from_numpy(rng.randint(1, n_items, size=n)).to(dev)
    args = launcher.build_args(["--model_name", "IF4Rec", "--runner_name", "HipRunner", "--seq_eval_native", "1",
                                "--eval_batch_size", "8192"])[0]
    run = runner.HipRunner(args)
    items = model.eval_items().detach().contiguous()
    state = {}

    def interests():
        state["q"] = run._interests_of(model, hist, lens)

    def rank():
        state["rank"] = hip_ops.rank_eval_multi(state["q"], items, target)[0]

    row = {"rows": n, "n_items": n_items, "K": K, "D": D, "eval_batch_size": 8192}
    row["interests_ms"] = alternated({"x": interests}, max(a.reps // 2, 3), warmup=1)["x"]
    row["rank_eval_multi_ms"] = alternated({"x": rank}, max(a.reps // 2, 3), warmup=1)["x"]
    row["rank_tflops"] = round(2.0 * n * K * n_items * D / (row["rank_eval_multi_ms"][0] * 1e-3) / 1e12, 2)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "if4rec_bench_n1.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "if4rec", "device": torch.cuda.get_device_name(0), "reps": a.reps, "ms": "[median, min, max]",
           "note": "step = zero_grad + predict + backward + torch.optim.Adam.step, torch blocks (4 heads) in both arms; pool_fwd_bwd = "
                   "forward() without the blocks + backward, dense table gradients included; the arms alternate inside every "
                   "repetition; peak_mb = peak allocation of one step beyond the model and optimizer state",
           "steps": [bench_batch(a, dev, B) for B in BATCHES], "evaluate": bench_evaluate(a, dev),
           "rank_large": bench_rank_large(a, dev)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
