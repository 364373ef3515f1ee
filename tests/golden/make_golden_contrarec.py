#!/usr/bin/env python
"""Generate tests/golden/g12_contrarec.npz by RUNNING THE REFERENCE's ContraRec (src/models/sequential/ContraRec.py) on the CPU.

    WR_REFERENCE=<reference checkout> python tests/golden/make_golden_contrarec.py

Needs the reference tree; the tests need only the file it writes.  Arrays and name lists only:
  sd__<name>            the initial state dict (300 items + the mask-token row, emb_size 64, history_max 20)
  hist, hist_a, hist_b  one batch, B = 96, T = 20, right-padded with 0; lengths cover 1, T and values between
  lengths, pos, neg     pos drawn from 24 items, so most rows have same-label partners
  ctc, ccc, loss        the two loss terms and predict()'s sum (gamma = 0.5, ccc_temp = 0.2), fp32
  g__<name>             every parameter's gradient of `loss`
  adam_losses           predict() before each of 5 Adam steps (lr 1e-3) on that batch
  aug_in, aug_len, aug_out   200 sequences and what Dataset.augment returns for them, in order, after np.random.seed(2023)
  names                 the state-dict names in order
"""
import argparse
import os
import sys

import numpy as np
import torch

REF = os.environ.get("WR_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "src"))
HERE = os.path.dirname(os.path.abspath(__file__))

from models.sequential.ContraRec import ContraRec  # noqa: E402
from utils.loss import BPRLoss  # noqa: E402

N_ITEMS, D, B, T = 300, 64, 96, 20
GAMMA, TEMP = 0.5, 0.2


class _Corpus:
    n_users, n_items = 40, N_ITEMS
    train_clicked_set, residual_clicked_set = {}, {}


class _Aug:
    """the three augmentation methods of ContraRec.Dataset bound to a model, without a corpus behind them"""
    reorder_op, mask_op, augment = ContraRec.Dataset.reorder_op, ContraRec.Dataset.mask_op, ContraRec.Dataset.augment

    def __init__(self, model):
        self.model = model


def pad(seqs, width):
    out = np.zeros((len(seqs), width), dtype=np.int64)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out


def main():
    torch.manual_seed(3407)
    args = argparse.Namespace(device=torch.device("cpu"), model_path="/tmp/wr_golden_contrarec.pt", buffer=1, num_neg=1, test_all=1,
                              history_max=T, emb_size=D, gamma=GAMMA, beta_a=3, beta_b=3, ccc_temp=TEMP)
    model = ContraRec(args, _Corpus())
    model.train()
    out = {}
    names = list(model.state_dict().keys())
    out["names"] = np.array(names)
    for k, v in model.state_dict().items():
        out["sd__" + k] = v.detach().numpy().copy()

    rng = np.random.RandomState(12)
    lengths = rng.randint(1, T + 1, size=B).astype(np.int64)
    lengths[:4] = [1, T, 2, T - 1]
    seqs = [rng.randint(1, N_ITEMS, size=n).astype(np.int64) for n in lengths]
    aug = _Aug(model)
    np.random.seed(12)
    seqs_a = [aug.augment(s) for s in seqs]
    seqs_b = [aug.augment(s) for s in seqs]
    pos = rng.randint(1, 25, size=B).astype(np.int64)
    neg = rng.randint(1, N_ITEMS, size=B).astype(np.int64)
    out.update(hist=pad(seqs, T), hist_a=pad(seqs_a, T), hist_b=pad(seqs_b, T), lengths=lengths, pos=pos, neg=neg)
    fd = {"history_items": torch.from_numpy(out["hist"]), "history_items_a": torch.from_numpy(out["hist_a"]),
          "history_items_b": torch.from_numpy(out["hist_b"]), "lengths": torch.from_numpy(lengths), "pos_item": torch.from_numpy(pos),
          "neg_items": torch.from_numpy(neg), "phase": "train", "batch_size": B}

    # the two terms by the reference's own pieces, then predict()'s sum and its gradients
    with torch.no_grad():
        user = model.forward(fd)
        ctc = BPRLoss()((user * model.item_embeddings(fd["pos_item"])).sum(1), (user * model.item_embeddings(fd["neg_items"])).sum(1))
        va = model.encoder(model.item_embeddings(fd["history_items_a"]), fd["lengths"])
        vb = model.encoder(model.item_embeddings(fd["history_items_b"]), fd["lengths"])
        feats = torch.nn.functional.normalize(torch.stack([va, vb], dim=1), dim=-1)
        ccc = model.ccc_loss(features=feats, labels=fd["pos_item"])
    model.zero_grad()
    loss = model.predict(fd)
    loss.backward()
    out["ctc"] = ctc.numpy().reshape(1).astype(np.float32)
    out["ccc"] = ccc.numpy().reshape(1).astype(np.float32)
    out["loss"] = loss.detach().numpy().reshape(1).astype(np.float32)
    assert abs(float(ctc) + GAMMA * float(ccc) - float(loss.detach())) < 1e-5 * abs(float(loss.detach()))
    for k, p in model.named_parameters():
        out["g__" + k] = p.grad.numpy().copy()

    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    curve = []
    for _ in range(5):
        opt.zero_grad()
        step_loss = model.predict(fd)
        step_loss.backward()
        opt.step()
        curve.append(float(step_loss.detach()))
    out["adam_losses"] = np.asarray(curve, dtype=np.float32)

    r2 = np.random.RandomState(13)
    aug_len = r2.randint(1, T + 1, size=200).astype(np.int64)
    aug_len[:3] = [1, 2, T]
    aug_in = [r2.randint(1, N_ITEMS, size=n).astype(np.int64) for n in aug_len]
    np.random.seed(2023)
    aug_out = [aug.augment(s) for s in aug_in]
    out.update(aug_in=pad(aug_in, T), aug_len=aug_len, aug_out=pad(aug_out, T))

    path = os.path.join(HERE, "g12_contrarec.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
