#!/usr/bin/env python3
"""A/B of two builds of the library on the fused InfoNCE (K12) and supervised contrastive (K15) losses: same bits, same speed.

    python scripts/ab_loss_libs.py --lib PATH --out run.json        one run of one library, in a fresh process
    python scripts/ab_loss_libs.py --merge OUT.json --parent p1.json p2.json p3.json --new n1.json n2.json n3.json

A run covers every infonce_ref.SHAPES case with and without duplicates, every contrarec_ref.LOSS_SHAPES case and the bench
shapes (InfoNCE n in {6040, 100000} at B = 2048, D = 64, tau = 0.2; SupCon B in {256, 2048, 4096} at D = 64), each with gradients
and loss-only, from seeded host data.  Per case it records the SHA-256 of every output's bytes and the time of one call: device
events around a window of back-to-back calls at least 50 ms long, after warm-up, median of five windows.

The merge fails (exit 1) when a hash of the new library differs from the parent's, or when a case's best new median exceeds
the parent's worst median by more than the parent's own spread (worst minus best median of its runs): what the machine cannot
tell apart from the parent itself.

Recorded (profiles/loss_pass_ab_n1.json, the shared pair pass of wr_pair_pass.h against the two separate pass kernels before it):
every hash equal, all 48 cases within the speed rule."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW_MS, WINDOWS = 50.0, 5
INFONCE_WEIGHT = 0.05


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def time_call(fn, torch):
    """-> (median us per call over WINDOWS windows, calls per window, shortest window in ms)"""
    def window(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = 4
    while True:                                                         # grow the window until it is long enough
        ms = window(reps)
        if ms >= 1.2 * WINDOW_MS:
            break
        reps = max(reps * 2, int(reps * 1.5 * WINDOW_MS / max(ms, 1e-3)) + 1)
    ws = [window(reps) for _ in range(WINDOWS)]
    assert min(ws) >= WINDOW_MS, ws
    return sorted(ws)[WINDOWS // 2] / reps * 1e3, reps, min(ws)


def run(a):
    from whisprrec_amd import abi
    abi.LIB_PATH = os.path.abspath(a.lib)                               # before the first abi.lib()
    assert os.path.exists(abi.LIB_PATH), abi.LIB_PATH
    import numpy as np
    import torch
    from whisprrec_amd import hip_ops
    import contrarec_ref as C
    import infonce_ref as R

    dev = torch.device("cuda:0")
    to = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    cases = {}

    def record(name, fn, fn_timed, outs):
        res = fn()
        us, reps, wmin = time_call(fn_timed, torch)
        cases[name] = {"sha256": {k: sha(t) for k, t in zip(outs, res) if t is not None}, "us": round(us, 3), "calls": reps,
                       "window_ms": round(wmin, 1)}
        print(name, cases[name]["us"], file=sys.stderr, flush=True)

    def infonce(name, n, B, D, tau, seed, dup):
        A, Bm, idx = (to(x) for x in R.make_case(n, B, D, seed, dup))
        for grads in (True, False):
            record("infonce %s %s" % (name, "grad" if grads else "loss"),
                   lambda: hip_ops.infonce_loss_grad(A, Bm, idx, tau, INFONCE_WEIGHT, grads=grads),
                   lambda: hip_ops.infonce_loss_grad(A, Bm, idx, tau, INFONCE_WEIGHT, grads=grads, validate=False),   # no read-back
                   ("loss", "gA", "gB"))
        hip_ops.infonce_release_workspaces()

    def supcon(name, F, labels, tau):
        F, labels = to(F), to(labels)
        for grads in (True, False):
            fn = lambda: hip_ops.supcon_loss_grad(F, labels, tau, grads=grads)  # noqa: E731
            record("supcon %s %s" % (name, "grad" if grads else "loss"), fn, fn, ("loss", "gF"))
        hip_ops.supcon_release_workspaces()

    for i, (n, B, D, tau) in enumerate(R.SHAPES):
        for dup in (False, True):
            infonce("n=%d B=%d D=%d tau=%g dup=%d" % (n, B, D, tau, dup), n, B, D, tau, 100 + i, dup)
    for n in (6040, 100000):
        infonce("bench n=%d B=2048 D=64 tau=0.2" % n, n, 2048, 64, 0.2, 21 + n, False)
    for i, shape in enumerate(C.LOSS_SHAPES):
        supcon("B=%d D=%d tau=%g labels=%d" % shape, *C.make_loss_case(i))
    for B in (256, 2048, 4096):
        rng = np.random.RandomState(B)
        supcon("bench B=%d D=64 tau=0.2" % B, rng.standard_normal((2 * B, 64)).astype(np.float32),
               rng.randint(1, 3706, size=B).astype(np.int64), 0.2)
    torch.cuda.synchronize()
    with open(a.out, "w") as f:
        json.dump({"lib": a.lib, "device": torch.cuda.get_device_name(0), "cases": cases}, f, indent=1)
        f.write("\n")


def merge(a):
    parent, new = ([json.load(open(p)) for p in ps] for ps in (a.parent, a.new))
    out = {"bench": "loss_pass_ab", "device": parent[0]["device"], "order": "parent, new, alternating, one fresh process per run",
           "us": "median per call of %d windows of back-to-back calls, each at least %g ms" % (WINDOWS, WINDOW_MS), "cases": {}}
    bad = []
    for name, ref in parent[0]["cases"].items():
        p_us = [r["cases"][name]["us"] for r in parent]
        n_us = [r["cases"][name]["us"] for r in new]
        same = all(r["cases"][name]["sha256"] == ref["sha256"] for r in parent + new)
        spread = max(p_us) - min(p_us)
        ok = min(n_us) <= max(p_us) + spread
        out["cases"][name] = {"sha256": ref["sha256"], "same_bits": same, "parent_us": p_us, "new_us": n_us,
                              "parent_spread_us": round(spread, 3), "same_speed": ok}
        if not same or not ok:
            bad.append(name)
    out["failed"] = bad
    with open(a.merge, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"cases": len(out["cases"]), "failed": bad}))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--merge")
    ap.add_argument("--parent", nargs="+")
    ap.add_argument("--new", nargs="+")
    a = ap.parse_args()
    if a.merge:
        return merge(a)
    run(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
