#!/usr/bin/env python
"""Generate tests/golden/g14_if4rec.npz by RUNNING THE REFERENCE's IF4Rec.forward (src/models/sequential/IF4Rec.py) on the CPU.

    WR_REFERENCE=<reference checkout> python tests/golden/make_golden_if4rec.py

Needs the reference tree; the tests need only the file it writes.  The reference's constructor names an initialiser that no
base class has, so the object is made with ``IF4Rec.__new__`` + ``nn.Module.__init__``, given the attributes of IF4Rec.py:49-57,
its own ``_define_params()`` and ``len_range`` under ``torch.manual_seed(3407)``, then ``xavier_normal_`` on every embedding and
linear weight and 0 in every linear bias (src/models/init.py:13-29).  Every number below comes from the reference's ``forward``
on a hand-made feed dict (``item_id`` = [pos, neg] in train phase, every item in test phase).  Arrays and name lists only:
  names                 the state-dict names in order
  sd__<name>            the initial state dict (300 items, D = 64, A = 8, K = 2, T = 20, 8 heads, dropout 0)
  history, lengths      one batch, B = 96: lengths 1..20 (both ends present), row 5 has an interior zero; items from a pool of 60
  item_id               [B, 2]: positive, negative
  pred, loss, g__<name> train phase: predictions [B, 2], BPRLoss (loss.py:38) of column 0 against column 1, every gradient
  fp_rows, fp_scores    test phase for 4 rows over all items
  k4__*                 a second case, K = 4 and 4 heads: the same state dict but ``W2`` (k4__sd__W2.weight / .bias), the same
                        batch; k4__pred, k4__loss, k4__fp_scores and k4__g__<name> for every parameter of at most 2048 elements
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("WR_REFERENCE")
if not REF:
    raise SystemExit("set WR_REFERENCE to a checkout of the reference (the directory that holds src/models)")
sys.path.insert(0, os.path.join(REF, "src"))
HERE = os.path.dirname(os.path.abspath(__file__))

from models.sequential.IF4Rec import IF4Rec  # noqa: E402
from utils.loss import BPRLoss  # noqa: E402

N_ITEMS, D, A, T, B = 300, 64, 8, 20, 96


def build(K, n_head):
    torch.manual_seed(3407)
    m = IF4Rec.__new__(IF4Rec)
    nn.Module.__init__(m)
    m.emb_size, m.attn_size, m.K, m.add_pos, m.max_his = D, A, K, 1, T
    m.encoder_layer, m.n_head, m.encoder_dropout, m.add_multi = 1, n_head, 0.0, 1
    m.item_num = N_ITEMS
    m._define_params()
    m.len_range = torch.from_numpy(np.arange(m.max_his))
    for mod in m.modules():
        if isinstance(mod, nn.Embedding):
            nn.init.xavier_normal_(mod.weight.data)
        elif isinstance(mod, nn.Linear):
            nn.init.xavier_normal_(mod.weight.data)
            nn.init.constant_(mod.bias.data, 0)
    m.train()
    return m


def batch():
    rng = np.random.RandomState(14)
    pool = 1 + rng.permutation(N_ITEMS - 1)[:60]
    lengths = np.concatenate([[1, T], rng.randint(1, T + 1, size=B - 2)]).astype(np.int64)
    history = np.zeros((B, T), np.int64)
    for r in range(B):
        history[r, :lengths[r]] = pool[rng.randint(0, 60, size=lengths[r])]
    lengths[5] = max(lengths[5], 6)
    history[5, :lengths[5]] = pool[rng.randint(0, 60, size=lengths[5])]
    history[5, 2] = 0                                    # an interior zero: masked by history > 0, not by the length
    item_id = np.stack([pool[rng.randint(0, 60, size=B)], pool[rng.randint(0, 60, size=B)]], axis=1).astype(np.int64)
    return history, lengths, item_id


def run(model, history, lengths, item_id, prefix, out, small_only):
    fd = {"item_id": torch.from_numpy(item_id), "history_items": torch.from_numpy(history), "lengths": torch.from_numpy(lengths),
          "phase": "train", "batch_size": B}
    model.zero_grad()
    pred = model.forward(fd)["prediction"]
    loss = BPRLoss()(pred[:, :1], pred[:, 1:])
    loss.backward()
    out[prefix + "pred"] = pred.detach().numpy().copy()
    out[prefix + "loss"] = loss.detach().numpy().reshape(1).astype(np.float32)
    for k, p in model.named_parameters():
        if not small_only or p.numel() <= 2048:
            out[prefix + "g__" + k] = p.grad.numpy().copy()
    fp_rows = np.array([0, 1, 5, B - 1], dtype=np.int64)
    fd = {"item_id": torch.arange(N_ITEMS)[None, :].repeat(4, 1), "history_items": torch.from_numpy(history[fp_rows]),
          "lengths": torch.from_numpy(lengths[fp_rows]), "phase": "test", "batch_size": 4}
    model.eval()
    with torch.no_grad():
        out["fp_rows"] = fp_rows
        out[prefix + "fp_scores"] = model.forward(fd)["prediction"].numpy().copy()
    model.train()


def main():
    out = {}
    history, lengths, item_id = batch()
    out.update(history=history, lengths=lengths, item_id=item_id)
    model = build(2, 8)
    out["names"] = np.array(list(model.state_dict().keys()))
    for k, v in model.state_dict().items():
        out["sd__" + k] = v.detach().numpy().copy()
    run(model, history, lengths, item_id, "", out, small_only=False)

    model4 = build(4, 4)
    sd = {k: v for k, v in model.state_dict().items() if not k.startswith("W2.")}
    model4.load_state_dict(sd, strict=False)
    for k, v in model4.state_dict().items():
        if k.startswith("W2."):
            out["k4__sd__" + k] = v.detach().numpy().copy()
    run(model4, history, lengths, item_id, "k4__", out, small_only=True)

    path = os.path.join(HERE, "g14_if4rec.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
