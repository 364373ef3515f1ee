#!/usr/bin/env python
"""Generate tests/golden/g15_tisasrec.npz by RUNNING THE REFERENCE's TimeIntervalTransformerLayer (src/utils/layers.py:149-170) on
the CPU.

    WR_REFERENCE=<reference checkout> python tests/golden/make_golden_tisasrec.py

Needs the reference tree; the tests need only the file it writes.  One case: B = 12, T = 20, D = 64, 4 heads, time_max = 32,
dropout 0.  The layer's inputs are gathered from small tables exactly as a model gathers them, so that the file stays below the
size of g14_if4rec.npz: x = item_tab[hist], pos_k = pos_k_tab[position], pos_v = pos_v_tab[position], inter_k =
time_k_tab[interval], inter_v = time_v_tab[interval], and the gradients of x, pos_k, pos_v, inter_k, inter_v are stored as the
gradients of those tables (autograd's scatter-add).  Every input (state dict, tables, upstream gradient) holds values that fp16
represents exactly and is stored as fp16; the layer ran on their fp32 casts.  Arrays and name lists only:
  names                     the state-dict names in order
  sd__<name>                the layer's state dict (fp16-exact; xavier weights, biases and layer-norm parameters moved off 0 / 1)
  item_tab, pos_k_tab, pos_v_tab, time_k_tab, time_v_tab       the tables (fp16-exact)
  hist, lengths, position   [B, T] item ids (left-aligned, zero-padded; lengths 1..20, both ends present), [B], [B, T]
  times, min_interval       [B, T] int64 timestamps (0 at padding), [B] int64 scales.  Rows 0-1: all timestamps equal; rows 2-3:
                            every gap above time_max * scale; the rest spread over both sides of the clamp
  interval                  [B, T, T] int16: min(|t_i - t_j| // scale, time_max), what the layer's inter_k / inter_v were gathered by
  gout                      [B, T, D] upstream gradient (fp16-exact); the loss is sum(out * gout)
  out                       [B, T, D] fp32, the layer's output
  g__<name>                 fp32 gradient of every parameter
  g__item_tab, g__pos_k_tab, g__pos_v_tab, g__time_k_tab, g__time_v_tab      fp32 gradients of the tables
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("WR_REFERENCE")
if not REF:
    raise SystemExit("set WR_REFERENCE to a checkout of the reference (the directory that holds src/utils)")
sys.path.insert(0, os.path.join(REF, "src"))
HERE = os.path.dirname(os.path.abspath(__file__))

from utils.layers import TimeIntervalTransformerLayer  # noqa: E402

B, T, D, HEADS, TIME_MAX, N_ITEMS = 12, 20, 64, 4, 32, 30


def h16(a):
    """the nearest values fp16 holds exactly, as fp32"""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def main():
    torch.manual_seed(3407)
    rng = np.random.RandomState(15)
    layer = TimeIntervalTransformerLayer(d_model=D, d_ff=D, n_heads=HEADS, dropout=0.0, kq_same=False)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            if p.dim() == 2:
                torch.nn.init.xavier_normal_(p)
            elif "layer_norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            elif "layer_norm" in name:
                p.copy_(0.1 * torch.randn_like(p))
            else:
                p.copy_(0.05 * torch.randn_like(p))
            p.copy_(torch.from_numpy(h16(p.numpy())))
    layer.train()

    def table(rows):       # the scale of xavier-initialised tables of a few thousand rows
        return h16(rng.standard_normal((rows, D)) * np.sqrt(2.0 / (3706 + D)) * 4.0)

    tabs = {"item_tab": table(N_ITEMS), "pos_k_tab": table(T + 1), "pos_v_tab": table(T + 1),
            "time_k_tab": table(TIME_MAX + 1), "time_v_tab": table(TIME_MAX + 1)}
    lengths = np.asarray([20, 1, 20, 7, 13, 2, 19, 5, 20, 11, 3, 16], np.int64)
    hist = np.zeros((B, T), np.int64)
    times = np.zeros((B, T), np.int64)
    min_interval = np.asarray([1, 7, 3, 60, 1, 5, 86400, 2, 30, 65535, 4, 9], np.int64)
    for b in range(B):
        n = int(lengths[b])
        hist[b, :n] = rng.randint(1, N_ITEMS, n)
        if b < 2:
            gaps = np.zeros(n, np.int64)                                  # equal timestamps: every pair on row 0
        elif b < 4:
            gaps = (TIME_MAX + 1 + rng.randint(0, 5, n)) * min_interval[b]    # every off-diagonal pair on the last row
        else:
            gaps = rng.randint(0, 6 * min_interval[b] + 1, n)             # both sides of the clamp, quotients with remainders
        times[b, :n] = 1_000_000_000 + np.cumsum(gaps)
    valid = hist > 0
    position = (lengths[:, None] - np.arange(T)[None, :]) * valid
    interval = np.minimum(np.abs(times[:, :, None] - times[:, None, :]) // min_interval[:, None, None], TIME_MAX)
    gout = h16(rng.standard_normal((B, T, D)))

    leaves = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in tabs.items()}
    x = leaves["item_tab"][torch.from_numpy(hist)]
    pos_k, pos_v = leaves["pos_k_tab"][torch.from_numpy(position)], leaves["pos_v_tab"][torch.from_numpy(position)]
    it = torch.from_numpy(interval)
    inter_k, inter_v = leaves["time_k_tab"][it], leaves["time_v_tab"][it]
    mask = torch.tril(torch.ones(1, 1, T, T, dtype=torch.int32))
    out = layer(x, pos_k, pos_v, inter_k, inter_v, mask)
    (out * torch.from_numpy(gout)).sum().backward()

    names = list(layer.state_dict().keys())
    blob = {"names": np.asarray(names), "hist": hist.astype(np.int16), "lengths": lengths.astype(np.int16),
            "position": position.astype(np.int16), "times": times, "min_interval": min_interval,
            "interval": interval.astype(np.int16), "gout": gout.astype(np.float16), "out": out.detach().numpy().astype(np.float32),
            "heads": np.asarray(HEADS), "time_max": np.asarray(TIME_MAX)}
    for k, v in layer.state_dict().items():
        assert np.array_equal(h16(v.numpy()), v.numpy())
        blob["sd__" + k] = v.numpy().astype(np.float16)
    for k, p in layer.named_parameters():
        blob["g__" + k] = p.grad.numpy().astype(np.float32)
    for k, v in tabs.items():
        blob[k] = v.astype(np.float16)
        blob["g__" + k] = leaves[k].grad.numpy().astype(np.float32)
    path = os.path.join(HERE, "g15_tisasrec.npz")
    np.savez_compressed(path, **blob)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
