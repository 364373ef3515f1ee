"""GRU4Rec's native recurrence against its stock path, in the same process.  At the ml-1m shape (6,040 users x 3,706 items,
E = H = 64), T in {20, 50} and B in {256, 2,048}, lengths uniform in [1, T]:
  * the GRU alone, forward + backward, from x [B, T, E] to gx and the four parameter gradients: `padded` (nn.GRU over the padded
    batch + the row at lengths - 1, what --gru_native 0 runs), `native` (hip_ops.gru_last, wr_gru.hip, K27) and `packed` (ReChorus's
    sort / pack_padded_sequence / unsort form, whose pack reads the lengths on the host);
  * one training step (zero_grad / predict / backward / Adam) with --gru_native 0 and 1, and its peak memory.
Device events, warm-up, the arms alternated repetition by repetition in --rounds rounds of --reps repetitions: [median, min, max]
over all repetitions and the spread [min, max] of the rounds' medians.  Prints one JSON line and writes it to --out.

    python scripts/bench_gru4rec.py [--reps 10] [--rounds 3] [--out profiles/gru4rec_bench_n1.json]
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
from whisprrec_amd.gru4rec import GRU4Rec  # noqa: E402

N_USERS, N_ITEMS, E, H = 6040, 3706, 64, 64
SHAPES = [(20, 256), (20, 2048), (50, 256), (50, 2048)]        # (T, B)


class Corpus:
    def __init__(self):
        self.n_users, self.n_items, self.user_his = N_USERS, N_ITEMS, {}


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(fns, reps, rounds, warmup=3):
    """{tag: {"ms": [median, min, max], "round_medians": [min, max]}} of the functions, run in turn inside every repetition"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {tag: [[] for _ in range(rounds)] for tag in fns}
    for r in range(rounds):
        for _ in range(reps):
            for tag, fn in fns.items():
                ts[tag][r].append(once(fn))
    out = {}
    for tag, per_round in ts.items():
        flat, med = np.concatenate(per_round), [float(np.median(v)) for v in per_round]
        out[tag] = {"ms": [round(float(np.median(flat)), 3), round(float(flat.min()), 3), round(float(flat.max()), 3)],
                    "round_medians": [round(min(med), 3), round(max(med), 3)]}
    return out


def make_model(dev, T, gru_native):
    torch.manual_seed(1)
    args = argparse.Namespace(device=dev, model_path="/tmp/wr_gru4rec_bench.pt", buffer=1, num_neg=1, test_all=1, history_max=T,
                              emb_size=E, hidden_size=H, gru_native=gru_native, emb_lazy=0, random_seed=1)
    return GRU4Rec(args, Corpus()).to(dev)


def feed(dev, T, B):
    rng = np.random.RandomState(100 * T + B)
    lens = rng.randint(1, T + 1, size=B)
    hist = rng.randint(1, N_ITEMS, size=(B, T)) * (np.arange(T)[None, :] < lens[:, None])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return {"history_items": t(hist), "lengths": t(lens), "user_id": t(rng.randint(0, N_USERS, B)),
            "pos_item": t(rng.randint(1, N_ITEMS, size=B)), "neg_items": t(rng.randint(1, N_ITEMS, size=(B, 1))), "batch_size": B,
            "phase": "train"}


def bench_shape(a, dev, T, B):
    fd = feed(dev, T, B)
    row = {"T": T, "B": B, "E": E, "H": H, "mean_length": round(float(fd["lengths"].float().mean()), 2)}
    models = {"padded": make_model(dev, T, 0).train(), "native": make_model(dev, T, 1).train()}
    for m in models.values():
        m.optimizer = torch.optim.Adam(m.parameters(), lr=1e-3)

    def step_of(m):
        def step():
            m.optimizer.zero_grad()
            loss = m.predict(fd)
            loss.backward()
            m.optimizer.step()
        return step

    for tag, res in alternated({tag: step_of(m) for tag, m in models.items()}, a.reps, a.rounds).items():
        row[tag + "_step"] = res
    for tag, m in models.items():                 # peak memory of one step beyond what is allocated before it
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step_of(m)()
        torch.cuda.synchronize()
        row[tag + "_step_peak_mb"] = round((torch.cuda.max_memory_allocated() - before) / 2**20, 2)
    assert models["native"]._gru_native_ok == {T: True}

    # the recurrence alone: x as the embedding lookup leaves it (zero rows past the length), the model's GRU
    rnn = models["native"].rnn
    params = [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0]
    gen = torch.Generator(device=dev).manual_seed(3)
    lengths = fd["lengths"]
    x = (torch.randn(B, T, E, device=dev, generator=gen) * 0.3 * (fd["history_items"] > 0)[:, :, None]).requires_grad_(True)
    g_last = torch.randn(B, H, device=dev, generator=gen)
    rows = torch.arange(B, device=dev)

    def clear():
        for t in [x] + params:
            t.grad = None

    def gru_padded():
        clear()
        rnn(x)[0][rows, lengths - 1, :].backward(g_last)

    def gru_native():
        clear()
        hip_ops.gru_last(x, lengths, *params).backward(g_last)

    def gru_packed():
        clear()
        sort_len, sort_idx = torch.topk(lengths, k=B)
        packed = torch.nn.utils.rnn.pack_padded_sequence(x.index_select(0, sort_idx), sort_len.cpu(), batch_first=True)
        hidden = rnn(packed, None)[1]
        unsort_idx = torch.topk(sort_idx, k=B, largest=False)[1]
        hidden[-1].index_select(0, unsort_idx).backward(g_last)

    arms = {"padded": gru_padded, "native": gru_native, "packed": gru_packed}
    try:
        gru_packed()
        torch.cuda.synchronize()
    except Exception as e:                        # recorded, not hidden: the third arm is optional
        row["packed_gru_fwd_bwd"] = "did not run: %s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])
        del arms["packed"]
    for tag, res in alternated(arms, a.reps, a.rounds).items():
        row[tag + "_gru_fwd_bwd"] = res
    clear()
    row["gru_workspace_mb"] = round(hip_ops.gru_workspace_bytes(B, T, E, H) / 2**20, 2)
    row["hs_mb"] = round(B * T * H * 4 / 2**20, 2)
    for key in ("step", "gru_fwd_bwd"):
        row[key + "_ratio_native_to_padded"] = round(row["native_" + key]["ms"][0] / row["padded_" + key]["ms"][0], 3)
    row["step_peak_ratio_native_to_padded"] = round(row["native_step_peak_mb"] / row["padded_step_peak_mb"], 4)
    print(json.dumps(row), file=sys.stderr, flush=True)
    del models
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru4rec_bench_n1.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"bench": "gru4rec", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds,
           "ms": "[median, min, max] over rounds x reps; round_medians = [min, max] of the rounds' medians",
           "note": "step = zero_grad + predict + backward + torch.optim.Adam.step (BPR loss); padded = nn.GRU over the padded batch "
                   "+ the row at lengths - 1 (--gru_native 0); native = hip_ops.gru_last (--gru_native 1); packed = sort / "
                   "pack_padded_sequence / unsort, with its host read of the lengths; gru_fwd_bwd = from x [B, T, E] to gx and the "
                   "four parameter gradients; lengths uniform in [1, T]; the arms alternate inside every repetition; peak_mb = peak "
                   "allocation of one step beyond the model and optimizer state; the native arm's kernel workspace "
                   "(gru_workspace_mb) is allocated once, at the first step, and is not in it",
           "shapes": [bench_shape(a, dev, T, B) for T, B in SHAPES]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
