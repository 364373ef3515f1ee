"""``--train_loss softmax`` for SASRec, TiSASRec and GRU4Rec: softmax cross-entropy of the last-position query against the whole item
catalogue, instead of the reference's BPRLoss against one sampled negative (SASRec.py / TiSASRec.py ``loss``).

The stock path (``--softmax_native 0``) is what defines the feature:

    logits = user_e @ item_embedding.weight.t();  logits[:, 0] = -inf;  F.cross_entropy(logits, pos_item)

It keeps the [B, n_items] logits and their softmax alive for autograd.  ``--softmax_native 1`` is one call of
``hip_ops.softmax_ce_loss`` (wr_softmax.hip, K26): the same loss and the gradients of the queries and of the item table without
that matrix.  An embedding size the kernel does not take is logged once and keeps the stock path.  Item 0 is padding and no class.
A positive that is no class (item 0, or an id past the table) raises ``IndexError`` — at once, or, inside ``HipRunner.fit``
(which range-checks the epoch's columns once), from a device word read when the model next leaves training mode, so that a step
has no host round trip.  ``neg_items`` is ignored under ``softmax``.  ``--emb_lazy 1`` is refused: every item row gets a gradient every step, so there is
nothing for the row-lazy table to skip.
"""
import logging

import torch
import torch.nn.functional as F

from . import hip_ops


class SoftmaxLossMixin:
    """the two flags, the construction-time check and the loss of ``predict`` under ``--train_loss softmax``"""

    @staticmethod
    def add_softmax_loss_args(parser):
        parser.add_argument("--train_loss", type=str, default="bpr", choices=["bpr", "softmax"],
                            help="bpr: BPRLoss against the sampled negative (the reference).  softmax: cross-entropy of the "
                                 "query against the whole item catalogue; neg_items is ignored.")
        parser.add_argument("--softmax_native", type=int, default=0, choices=[0, 1],
                            help="--train_loss softmax only.  1: loss and gradients by the fused HIP kernel, no [B, n_items] "
                                 "logits; 0: torch matmul + cross_entropy under autograd.")

    def _install_softmax_loss(self, args):
        self.train_loss = str(getattr(args, "train_loss", "bpr"))
        if self.train_loss not in ("bpr", "softmax"):
            raise ValueError("--train_loss must be bpr or softmax, got %r" % (self.train_loss,))
        self.softmax_native = bool(int(getattr(args, "softmax_native", 0)))
        self._softmax_native_ok = None      # decided at the first training batch: the library says what it takes
        self._softmax_err = None            # device error word of the loss kernel (a positive that is no class), read by train(False)
        if self.train_loss == "softmax" and int(getattr(args, "emb_lazy", 0)):
            raise ValueError("--train_loss softmax cannot run with --emb_lazy 1: under the full-catalogue softmax every item row gets "
                             "a gradient every step, so there is nothing for the row-lazy table to skip")

    def _use_softmax_native(self):
        if not self.softmax_native:
            return False
        if self._softmax_native_ok is None:
            self._softmax_native_ok = hip_ops.softmax_ce_supports(self.emb_size)
            if not self._softmax_native_ok:
                logging.warning("--softmax_native 1: the loss kernel does not take emb_size=%d; keeping the torch path",
                                self.emb_size)
        return self._softmax_native_ok

    def softmax_loss(self, user_e, pos_item):
        """mean over the batch of the cross-entropy of user_e [B, D] against every item but the padding row"""
        weight = self.item_embedding.weight
        target = pos_item.reshape(-1)
        if self._use_softmax_native():
            if not getattr(self, "_trusted_indices", False):
                return hip_ops.softmax_ce_loss(user_e, weight, target, 1)
            if self._softmax_err is None or self._softmax_err.device != weight.device:
                self._softmax_err = torch.zeros(1, dtype=torch.int32, device=weight.device)
            return hip_ops.softmax_ce_loss(user_e, weight, target, 1, err_word=self._softmax_err)
        logits = user_e @ weight.t()
        logits[:, 0] = -float("inf")
        return F.cross_entropy(logits, target)

    def check_softmax_targets(self):
        """raise if a native loss call since the last check met a positive that is no class (one read of the device word)"""
        if self._softmax_err is not None and int(self._softmax_err.item()) != 0:
            self._softmax_err.zero_()
            raise IndexError("--train_loss softmax: a positive item outside [1, %d) reached the loss kernel (clamped to the "
                             "nearest class); item 0 is padding and no class" % self.item_embedding.weight.shape[0])

    def train(self, mode=True):
        try:
            if not mode and getattr(self, "_softmax_err", None) is not None:
                self.check_softmax_targets()      # model.eval() precedes every evaluation
        finally:
            out = super().train(mode)             # the mode changes even when the check raises
        return out
