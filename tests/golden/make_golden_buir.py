#!/usr/bin/env python
"""Generate tests/golden/g13_buir.npz by RUNNING THE REFERENCE's BUIR methods (src/models/general/BUIR.py) on the CPU.

    WR_REFERENCE=<reference checkout> python tests/golden/make_golden_buir.py

Needs the reference tree; the tests need only the file it writes.  The reference's constructor no longer fits its own base
class, so the object is made with ``BUIR.__new__`` + ``nn.Module.__init__``, given the attributes of BUIR.py:48-57 under
``torch.manual_seed(3407)``, initialised by the reference's ``_init_weights`` and the target copies of :61-66; every number
below then comes from the reference's ``predict`` / ``full_predict`` / ``_update_target``.  Arrays and name lists only:
  names                   the state-dict names in order
  sd__<name>              the initial state dict (50 users, 70 items, D = 64)
  users, items            one batch, B = 96: users drawn from 8 ids, items from 12 (42 user rows are never touched)
  loss, g__<name>         predict() on it and the gradient of every trainable parameter
  fp_users, fp_scores     full_predict for 4 users
  a_* / b_*               two runs of 5 Adam steps with _update_target after each step, (a) momentum 0.995 lr 1e-3, (b)
                          momentum 0.9 lr 1e-2: <run>_losses (predict before each step) and <run>_sd__<table> for the four tables
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("WR_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "src"))
HERE = os.path.dirname(os.path.abspath(__file__))

from models.general.BUIR import BUIR  # noqa: E402

N_USERS, N_ITEMS, D, B = 50, 70, 64, 96
TABLES = ["user_online.weight", "user_target.weight", "item_online.weight", "item_target.weight"]


def build(momentum):
    torch.manual_seed(3407)
    m = BUIR.__new__(BUIR)
    nn.Module.__init__(m)
    m.embedding_size, m.momentum, m.user_num, m.item_num = D, momentum, N_USERS, N_ITEMS
    m.user_online = nn.Embedding(m.user_num, m.embedding_size)
    m.user_target = nn.Embedding(m.user_num, m.embedding_size)
    m.item_online = nn.Embedding(m.item_num, m.embedding_size)
    m.item_target = nn.Embedding(m.item_num, m.embedding_size)
    m.predictor = nn.Linear(m.embedding_size, m.embedding_size)
    m._init_weights()
    for online, target in ((m.user_online, m.user_target), (m.item_online, m.item_target)):
        for param_o, param_t in zip(online.parameters(), target.parameters()):
            param_t.data.copy_(param_o.data)
            param_t.requires_grad = False
    m.train()
    return m


def main():
    out = {}
    model = build(0.995)
    out["names"] = np.array(list(model.state_dict().keys()))
    for k, v in model.state_dict().items():
        out["sd__" + k] = v.detach().numpy().copy()

    rng = np.random.RandomState(13)
    user_pool = rng.permutation(N_USERS)[:8]
    item_pool = 1 + rng.permutation(N_ITEMS - 1)[:12]
    users = user_pool[rng.randint(0, 8, size=B)].astype(np.int64)
    items = item_pool[rng.randint(0, 12, size=B)].astype(np.int64)
    out.update(users=users, items=items)
    fd = {"user_id": torch.from_numpy(users), "pos_item": torch.from_numpy(items), "batch_size": B, "phase": "train"}

    model.zero_grad()
    loss = model.predict(fd)
    loss.backward()
    out["loss"] = loss.detach().numpy().reshape(1).astype(np.float32)
    for k, p in model.named_parameters():
        if p.requires_grad:
            out["g__" + k] = p.grad.numpy().copy()

    fp_users = np.array([user_pool[0], user_pool[3], 0, N_USERS - 1], dtype=np.int64)
    with torch.no_grad():
        out["fp_users"] = fp_users
        out["fp_scores"] = model.full_predict({"user_id": torch.from_numpy(fp_users)}).numpy().copy()

    for tag, momentum, lr in (("a", 0.995, 1e-3), ("b", 0.9, 1e-2)):
        m = build(momentum)
        opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=lr)
        curve = []
        for _ in range(5):
            opt.zero_grad()
            step_loss = m.predict(fd)
            step_loss.backward()
            opt.step()
            m._update_target()
            curve.append(float(step_loss.detach()))
        out[tag + "_losses"] = np.asarray(curve, dtype=np.float32)
        sd = m.state_dict()
        for t in TABLES:
            out[tag + "_sd__" + t] = sd[t].detach().numpy().copy()

    path = os.path.join(HERE, "g13_buir.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
