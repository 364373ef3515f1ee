"""NARM's native paths against its stock paths, in the same process.  At the ml-1m shape (6,040 users x 3,706 items, E = H = 64,
A = 16), T in {20, 50} and B in {256, 2,048}, lengths uniform in [1, T]:
  * the attention pooling alone (20 warm-up calls per arm: both arms are a few small launches, and the first shape measured
    colder with 3), forward + backward, from hs [B, T, H] and h_g to their gradients and those of A1, A2 and v:
    `stock` (the torch ops of --pool_native 0) and `native` (hip_ops.narm_pool, wr_narm.hip, K28);
  * both recurrences, forward + backward, from x [B, T, E] to gx and the eight parameter gradients, with a gradient on the global
    encoder's last state and on every state of the local one: `stock` (two nn.GRU over the padded batch) and `native`
    (hip_ops.gru_last + hip_ops.gru_seq, wr_gru.hip, K27);
  * one training step (zero_grad / predict / backward / Adam) with both flags off and both on, and its peak memory;
  * one row for GRU4Rec --num_layers 2 (T = 20, B = 2,048): the training step with --gru_native 0 and 1.
Device events, warm-up, the arms alternated repetition by repetition in --rounds rounds of --reps repetitions: [median, min, max]
over all repetitions and the spread [min, max] of the rounds' medians.  Prints one JSON line and writes it to --out.

--parent_lib PATH: also the `gru_last_ab` key — bench_gru4rec.py's "GRU forward + backward alone" native arm timed in fresh
processes that load the library at PATH (a build of the parent commit) and this tree's library in turn, --ab_runs times each;
`within_parent_spread` says per shape whether every run's median of this build lies inside [min, max] of the medians of the
parent's own rounds.

    python scripts/bench_narm.py [--reps 10] [--rounds 3] [--parent_lib PATH] [--out profiles/narm_bench_n1.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from whisprrec_amd import abi  # noqa: E402

N_USERS, N_ITEMS, E, H, A = 6040, 3706, 64, 64, 16
SHAPES = [(20, 256), (20, 2048), (50, 256), (50, 2048)]        # (T, B)


def ab_child(a):
    """the native arm of bench_gru4rec.py's GRU-alone rows with the library at a.ab_child -> one JSON line"""
    import ctypes
    abi.LIB_PATH = a.ab_child
    exported = ctypes.CDLL(a.ab_child)
    abi.SIGNATURES = {k: v for k, v in abi.SIGNATURES.items() if hasattr(exported, k)}      # a parent build lacks the new exports
    from whisprrec_amd import hip_ops
    from bench_gru4rec import alternated, feed
    dev = torch.device("cuda:0")
    rows = []
    for T, B in SHAPES:
        fd = feed(dev, T, B)
        torch.manual_seed(1)
        rnn = torch.nn.GRU(E, H, batch_first=True).to(dev)
        params = [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0]
        gen = torch.Generator(device=dev).manual_seed(3)
        x = (torch.randn(B, T, E, device=dev, generator=gen) * 0.3 * (fd["history_items"] > 0)[:, :, None]).requires_grad_(True)
        g_last = torch.randn(B, H, device=dev, generator=gen)

        def gru_native():
            for t in [x] + params:
                t.grad = None
            hip_ops.gru_last(x, fd["lengths"], *params).backward(g_last)

        rows.append(dict(T=T, B=B, **alternated({"native_gru_fwd_bwd": gru_native}, a.reps, a.rounds)["native_gru_fwd_bwd"]))
    print(json.dumps(rows))


def gru_last_ab(a):
    this = os.path.join(ROOT, "whisprrec_amd", "libwhisprrec_hip.so")
    runs = {"parent": [], "this": []}
    for _ in range(a.ab_runs):
        for tag, lib in (("parent", a.parent_lib), ("this", this)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab_child", lib, "--reps", str(a.reps), "--rounds",
                                  str(a.rounds)], check=True, capture_output=True, text=True, timeout=300).stdout
            runs[tag].append(json.loads(out.strip().splitlines()[-1]))
    verdict = []
    for i, (T, B) in enumerate(SHAPES):
        pm, tm = [r[i]["ms"][0] for r in runs["parent"]], [r[i]["ms"][0] for r in runs["this"]]
        lo, hi = min(r[i]["round_medians"][0] for r in runs["parent"]), max(r[i]["round_medians"][1] for r in runs["parent"])
        verdict.append({"T": T, "B": B, "parent_medians_ms": pm, "this_medians_ms": tm, "parent_round_medians_spread_ms": [lo, hi],
                        "within_parent_spread": bool(lo <= min(tm) and max(tm) <= hi)})
    return {"what": "hip_ops.gru_last forward + backward alone (bench_gru4rec.py's native_gru_fwd_bwd), fresh processes alternating "
                    "between a build of the parent commit and this one", "runs": runs, "per_shape": verdict}


class Corpus:
    def __init__(self):
        self.n_users, self.n_items, self.user_his = N_USERS, N_ITEMS, {}


def make_model(cls, dev, T, native, **extra):
    torch.manual_seed(1)
    args = argparse.Namespace(device=dev, model_path="/tmp/wr_narm_bench.pt", buffer=1, num_neg=1, test_all=1, history_max=T,
                              emb_size=E, hidden_size=H, attention_size=A, gru_native=native, pool_native=native, emb_lazy=0,
                              random_seed=1, **extra)
    return cls(args, Corpus()).to(dev)


def step_rows(models, fd, a, row, suffix=""):
    from bench_gru4rec import alternated
    for m in models.values():
        m.train()
        m.optimizer = torch.optim.Adam(m.parameters(), lr=1e-3)

    def step_of(m):
        def step():
            m.optimizer.zero_grad()
            loss = m.predict(fd)
            loss.backward()
            m.optimizer.step()
        return step

    for tag, res in alternated({tag: step_of(m) for tag, m in models.items()}, a.reps, a.rounds).items():
        row[tag + "_step" + suffix] = res
    for tag, m in models.items():                 # peak memory of one step beyond what is allocated before it
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step_of(m)()
        torch.cuda.synchronize()
        row[tag + "_step_peak_mb" + suffix] = round((torch.cuda.max_memory_allocated() - before) / 2**20, 2)


def bench_shape(a, dev, T, B):
    from bench_gru4rec import alternated, feed
    from whisprrec_amd import hip_ops
    from whisprrec_amd.narm import NARM
    fd = feed(dev, T, B)
    lengths = fd["lengths"]
    row = {"T": T, "B": B, "E": E, "H": H, "A": A, "mean_length": round(float(lengths.float().mean()), 2)}
    models = {"stock": make_model(NARM, dev, T, 0), "native": make_model(NARM, dev, T, 1)}
    step_rows(models, fd, a, row)
    assert models["native"]._gru_native_ok == {T: True} and models["native"]._pool_native_ok == {T: True}

    m = models["native"]
    gen = torch.Generator(device=dev).manual_seed(3)
    live = (fd["history_items"] > 0)[:, :, None]
    rows = torch.arange(B, device=dev)

    # the pooling alone: hs as gru_seq leaves it (zero past the length)
    pool_in = [(torch.tanh(torch.randn(B, T, H, device=dev, generator=gen)) * live).requires_grad_(True),
               torch.tanh(torch.randn(B, H, device=dev, generator=gen)).requires_grad_(True)]
    pool_w = [m.A1.weight, m.A2.weight, m.attention_out.weight]
    g_c = torch.randn(B, H, device=dev, generator=gen)

    def clear(ts):
        for t in ts:
            t.grad = None

    def pool_stock():
        clear(pool_in + pool_w)
        hs, hg = pool_in
        e = m.attention_out(torch.sigmoid(m.A1(hg)[:, None, :] + m.A2(hs))).squeeze(-1)
        e = e * (torch.arange(T, device=dev)[None, :] < lengths[:, None]).to(e.dtype)
        (e[:, :, None] * hs).sum(dim=1).backward(g_c)

    def pool_native():
        clear(pool_in + pool_w)
        hip_ops.narm_pool(pool_in[0], pool_in[1], lengths, *pool_w).backward(g_c)

    for tag, res in alternated({"stock": pool_stock, "native": pool_native}, a.reps, a.rounds, warmup=20).items():
        row[tag + "_pool_fwd_bwd"] = res
    clear(pool_in + pool_w)

    # both recurrences: a gradient on the global encoder's last state and on every state of the local one
    pg = [getattr(m.encoder_g, n + "_l0") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    pl = [getattr(m.encoder_l, n + "_l0") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    x = (torch.randn(B, T, E, device=dev, generator=gen) * 0.3 * live).requires_grad_(True)
    g_last = torch.randn(B, H, device=dev, generator=gen)
    g_hs = torch.randn(B, T, H, device=dev, generator=gen) * live

    def gru_stock():
        clear([x] + pg + pl)
        h_g = m.encoder_g(x)[0][rows, lengths - 1, :]
        hs_l = m.encoder_l(x)[0]
        torch.autograd.backward([h_g, hs_l], [g_last, g_hs])

    def gru_native():
        clear([x] + pg + pl)
        torch.autograd.backward([hip_ops.gru_last(x, lengths, *pg), hip_ops.gru_seq(x, lengths, *pl)], [g_last, g_hs])

    for tag, res in alternated({"stock": gru_stock, "native": gru_native}, a.reps, a.rounds).items():
        row[tag + "_two_gru_fwd_bwd"] = res
    clear([x] + pg + pl)
    row["pool_workspace_mb"] = round(hip_ops.narm_pool_workspace_bytes(B, T, H, A) / 2**20, 2)
    row["gru_workspace_mb"] = round(hip_ops.gru_workspace_bytes(B, T, E, H) / 2**20, 2)
    for key in ("step", "pool_fwd_bwd", "two_gru_fwd_bwd"):
        row[key + "_ratio_native_to_stock"] = round(row["native_" + key]["ms"][0] / row["stock_" + key]["ms"][0], 3)
    row["step_peak_ratio_native_to_stock"] = round(row["native_step_peak_mb"] / row["stock_step_peak_mb"], 4)
    print(json.dumps(row), file=sys.stderr, flush=True)
    del models
    torch.cuda.empty_cache()
    return row


def bench_gru4rec_two_layers(a, dev, T=20, B=2048):
    from bench_gru4rec import feed
    from whisprrec_amd.gru4rec import GRU4Rec
    fd = feed(dev, T, B)
    row = {"model": "GRU4Rec", "num_layers": 2, "T": T, "B": B, "E": E, "H": H}
    models = {"stock": make_model(GRU4Rec, dev, T, 0, num_layers=2), "native": make_model(GRU4Rec, dev, T, 1, num_layers=2)}
    step_rows(models, fd, a, row)
    assert models["native"]._gru_native_ok == {T: True}
    row["step_ratio_native_to_stock"] = round(row["native_step"]["ms"][0] / row["stock_step"]["ms"][0], 3)
    row["step_peak_ratio_native_to_stock"] = round(row["native_step_peak_mb"] / row["stock_step_peak_mb"], 4)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent_lib", default="")
    ap.add_argument("--ab_runs", type=int, default=3)
    ap.add_argument("--ab_child", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "narm_bench_n1.json"))
    a = ap.parse_args()
    if a.ab_child:
        return ab_child(a)
    ab = gru_last_ab(a) if a.parent_lib else None      # before this process opens the device
    dev = torch.device("cuda:0")
    res = {"bench": "narm", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds,
           "ms": "[median, min, max] over rounds x reps; round_medians = [min, max] of the rounds' medians",
           "note": "step = zero_grad + predict + backward + torch.optim.Adam.step (BPR loss); stock = --gru_native 0 --pool_native 0 "
                   "(nn.GRU over the padded batch, torch pooling ops with the length mask); native = both flags 1 (hip_ops.gru_last "
                   "+ gru_seq + narm_pool); pool_fwd_bwd = from hs [B, T, H] and h_g to their gradients and those of A1, A2, v; "
                   "two_gru_fwd_bwd = both encoders from x [B, T, E] to gx and the eight parameter gradients; lengths uniform in "
                   "[1, T]; the arms alternate inside every repetition; peak_mb = peak allocation of one step beyond the model and "
                   "optimizer state; the native arm's kernel workspaces are allocated once, at the first step, and are not in it",
           "shapes": [bench_shape(a, dev, T, B) for T, B in SHAPES],
           "gru4rec_num_layers_2": bench_gru4rec_two_layers(a, dev)}
    if ab is not None:
        res["gru_last_ab"] = ab
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
