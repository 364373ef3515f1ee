"""ContraRec (reference src/models/sequential/ContraRec.py): a BERT4Rec-style encoder over the item history, trained with BPR
(the paper's context-target contrast at tau_1 = 1, K = 1) plus ``gamma`` times a supervised contrastive loss between two
augmented views of every history (context-context contrast), the views' labels being the target items.

Parameter names are the reference's, so checkpoints interchange: ``item_embeddings`` (``item_num + 1`` rows: the last one is the
mask token of the augmentation; no padding index), ``encoder.p_embeddings``, ``encoder.transformer_block.{0,1}`` (two
``sasrec._Block`` layers, 2 heads, d_ff = emb_size, dropout 0).  Initialisation: ``xavier_uniform_initialization`` of
src/models/init.py:32-48 — xavier_uniform_ on every embedding and linear weight, linear biases 0, LayerNorm untouched.

The encoder (``BERT4RecEncoder.forward``, :216-233) masks KEYS by length: every query position, padded ones included, attends
to the keys j < length.  Two native paths, both off by default:
  --block_native 1   the six block calls of a training step (three views x two layers) go through
                     ``hip_ops.sasrec_block(key_lengths=...)`` (wr_sasblock_fwd_keys / _bwd_keys, K13).  Each view is its own
                     call, so each keeps the reference's per-call score maximum.
  --ccc_native 1     the contrastive term goes through ``hip_ops.supcon_loss`` (wr_supcon_loss_grad, K15): no [2B, 2B] array.
A shape the kernels do not take is logged once and keeps the torch path.

The two augmented views of a training row come from ``Dataset._get_feed_dict``, sample by sample from NumPy's global stream, so
``HipRunner.fit`` leaves this model to the reference's DataLoader loop (``per_sample_feed``).  Off by default:
  --aug_native 1     the views of a batch are drawn on the device (``hip_ops.seq_augment``, wr_seq_augment, K21) from the runner's
                     history table, keyed by (--random_seed, epoch, dataset row, view): the reference's distribution, not NumPy's
                     stream.  The model then trains through ``HipRunner.fit``'s batch loop like SASRec (``train_batch_extras``).
                     A (history_max, beta_a, beta_b) the kernel does not take is logged once and keeps the host path.
"""
import logging

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip_ops, host
from .sasrec import EmbLazyMixin, HipEmbedding, _Block


def _xavier_uniform_all(module):
    """reference src/models/init.py:32-48 applied through nn.Module.apply"""
    if isinstance(module, (nn.Embedding, HipEmbedding)):
        nn.init.xavier_uniform_(module.weight.data)
    elif isinstance(module, nn.Linear):
        nn.init.xavier_uniform_(module.weight.data)
        if module.bias is not None:
            nn.init.constant_(module.bias.data, 0)


def contra_loss(features, labels, temperature):
    """ContraLoss.forward (ContraRec.py:148-204) as written, on stock torch ops.  features [B, 2, D] (normalised), labels [B]."""
    bsz, views = features.shape[0], features.shape[1]
    labels = labels.contiguous().view(-1, 1)
    mask = torch.eq(labels, labels.transpose(0, 1)).float()
    contrast = torch.cat(torch.unbind(features, dim=1), dim=0)
    adc = torch.matmul(contrast, contrast.transpose(0, 1)) / temperature
    logits_max, _ = torch.max(adc, dim=1, keepdim=True)
    adc = adc - logits_max                       # the reference's in-place sub_ (:181) ...
    logits = adc - logits_max.detach()           # ... and the second shift (:182)
    mask = mask.repeat(views, views)
    logits_mask = torch.scatter(torch.ones_like(mask), 1, torch.arange(bsz * views, device=mask.device).view(-1, 1), 0)
    mask = mask * logits_mask
    exp_logits = torch.exp(logits) * logits_mask
    log_prob = logits - torch.log(exp_logits.sum(1, keepdim=True) + 1e-10)
    mean_log_prob_pos = (mask * log_prob).sum(1) / (mask.sum(1) + 1e-10)
    return (-temperature * mean_log_prob_pos).mean()


class BERT4RecEncoder(nn.Module):
    """ContraRec.py:207-233.  `block_fn(block, x, lengths)` replaces the torch call of a block when given."""

    def __init__(self, emb_size, max_his, num_layers=2, num_heads=2):
        super().__init__()
        self.p_embeddings = nn.Embedding(max_his + 1, emb_size)
        self.transformer_block = nn.ModuleList([_Block(emb_size, emb_size, num_heads, 0.0) for _ in range(num_layers)])

    def forward(self, seq, lengths, block_fn=None):
        bsz, T = seq.size(0), seq.size(1)
        len_range = torch.arange(T, device=seq.device)
        valid = len_range[None, :] < lengths[:, None]
        seq = seq + self.p_embeddings(len_range[None, :] * valid.long())
        attn_mask = valid.view(bsz, 1, 1, T)
        for blk in self.transformer_block:
            seq = blk(seq, attn_mask) if block_fn is None else block_fn(blk, seq, lengths)
        seq = seq * valid[:, :, None].float()
        return seq[torch.arange(bsz, device=seq.device), lengths - 1]


def make_contrarec(sequential_model_cls):
    class ContraRec(EmbLazyMixin, sequential_model_cls):
        reader = "SeqReader"
        runner = "BaseRunner"
        extra_log_args = ["gamma", "num_neg", "batch_size", "ccc_temp"]
        NUM_LAYERS, NUM_HEADS = 2, 2
        per_sample_feed = True       # HipRunner.fit: the augmented views come from Dataset._get_feed_dict, row by row
                                     # (an instance under --aug_native 1 with a supported shape sets it to False)

        @staticmethod
        def parse_model_args(parser):
            parser.add_argument("--emb_size", type=int, default=64, help="Size of embedding vectors.")
            parser.add_argument("--gamma", type=float, default=1, help="Coefficient of the contrastive loss.")
            parser.add_argument("--beta_a", type=int, default=3, help="Parameter of the beta distribution for sampling.")
            parser.add_argument("--beta_b", type=int, default=3, help="Parameter of the beta distribution for sampling.")
            parser.add_argument("--ccc_temp", type=float, default=0.2, help="Temperature in context-context contrastive loss.")
            parser.add_argument("--block_native", type=int, default=0, choices=[0, 1],
                                help="1: each encoder block by the fused HIP kernels with a key-length mask; 0: torch ops + autograd.")
            parser.add_argument("--ccc_native", type=int, default=0, choices=[0, 1],
                                help="1: the contrastive loss and its gradient by the fused HIP kernel; 0: torch ops + autograd.")
            parser.add_argument("--aug_native", type=int, default=0, choices=[0, 1],
                                help="1: the two augmented views of every batch are drawn on the device and the model trains "
                                     "through HipRunner's batch loop; the views follow the reference's distribution and are keyed "
                                     "by --random_seed, but are not NumPy's stream.  0: the reference's per-sample DataLoader loop.")
            EmbLazyMixin.add_emb_lazy_arg(parser)
            return sequential_model_cls.parse_model_args(parser)

        def __init__(self, args, corpus):
            super().__init__(args, corpus)
            self.emb_size, self.max_his = args.emb_size, args.history_max
            self.gamma, self.beta_a, self.beta_b, self.ccc_temp = args.gamma, args.beta_a, args.beta_b, args.ccc_temp
            self.mask_token = corpus.n_items
            self.item_embeddings = HipEmbedding(self.item_num + 1, self.emb_size)
            self.encoder = BERT4RecEncoder(self.emb_size, self.max_his, self.NUM_LAYERS, self.NUM_HEADS)
            self.apply(_xavier_uniform_all)
            self.block_native = bool(int(getattr(args, "block_native", 0)))
            self.ccc_native = bool(int(getattr(args, "ccc_native", 0)))
            self._block_native_ok = {}   # per history length, decided at its first batch: the library says what it takes
            self._ccc_native_ok = {}     # per batch size
            self._block_err = None       # device error word of the key lengths, read by check_key_lengths()
            self.aug_native = bool(int(getattr(args, "aug_native", 0)))
            self.aug_seed = int(getattr(args, "random_seed", 3407))
            self._aug_table = None       # (histories [n, T], lengths [n]) of the training rows, unshuffled: set_history_table()
            self._aug_err = None         # device error word of the view builder, read by check_train_extras()
            if self.aug_native:
                if hip_ops.seq_augment_supports(self.max_his, self.beta_a, self.beta_b):
                    self.per_sample_feed = False     # HipRunner.fit: slices of the epoch's device columns + train_batch_extras
                else:
                    logging.warning("--aug_native 1: the view builder does not take history_max=%s beta_a=%s beta_b=%s; keeping "
                                    "the host path", self.max_his, self.beta_a, self.beta_b)
            self._install_emb_lazy(args, self.item_embeddings)

        # ------------------------------------------------------------------------------------ native paths
        def _use_block_native(self, T):
            if not self.block_native:
                return False
            if T not in self._block_native_ok:
                ok = hip_ops.sasblock_supports(self.emb_size, self.emb_size, self.NUM_HEADS, T)
                if not ok and not any(v is False for v in self._block_native_ok.values()):
                    logging.warning("--block_native 1: the block kernels do not take emb_size=%d num_heads=%d history=%d; keeping "
                                    "the torch path", self.emb_size, self.NUM_HEADS, T)
                self._block_native_ok[T] = ok
            return self._block_native_ok[T]

        def _use_ccc_native(self, bsz):
            if not self.ccc_native:
                return False
            if bsz not in self._ccc_native_ok:
                ok = hip_ops.supcon_supports(self.emb_size) and 1 <= bsz and 2 * bsz <= hip_ops.SUPCON_MAX_ROWS
                if not ok and not any(v is False for v in self._ccc_native_ok.values()):
                    logging.warning("--ccc_native 1: the loss kernel does not take emb_size=%d batch=%d; keeping the torch path",
                                    self.emb_size, bsz)
                self._ccc_native_ok[bsz] = ok
            return self._ccc_native_ok[bsz]

        def _native_block(self, blk, x, lengths):
            if self._block_err is None:
                self._block_err = torch.zeros(1, dtype=torch.int32, device=x.device)
            return hip_ops.sasrec_block(x, blk, self.NUM_HEADS, 0.0, 0, False, key_lengths=lengths, err_word=self._block_err)

        def check_key_lengths(self):
            """raise if a block call since the last check was handed a length outside [1, T] (one read of the device word)"""
            if self._block_err is not None and int(self._block_err.item()) != 0:
                self._block_err.zero_()
                raise IndexError("ContraRec: a history length outside [1, history_max] reached the block kernels")

        # ------------------------------------------------------------------------------------ the views on the device
        def set_history_table(self, hist, lengths):
            """HipRunner.fit, once per epoch: the histories [n, T] and lengths [n] of the training rows in dataset order"""
            self._aug_table = (hist, lengths)

        def train_batch_extras(self, batch, rows, epoch):
            """HipRunner.fit, per batch: adds the two views of the dataset rows `rows` (device int64 [B]) in epoch `epoch`"""
            hist, lengths = self._aug_table
            if self._aug_err is None:
                self._aug_err = torch.zeros(1, dtype=torch.int32, device=hist.device)
            batch["history_items_a"], batch["history_items_b"] = hip_ops.seq_augment(
                hist, lengths, rows, self.mask_token, self.beta_a, self.beta_b, self.aug_seed, epoch, err_word=self._aug_err)
            return batch

        def check_train_extras(self):
            """raise if a view builder call since the last check met a length outside [1, T] or a row id outside the table (one
            read of the device word; HipRunner.fit asks once per epoch)"""
            if self._aug_err is not None:
                word = int(self._aug_err.item())
                if word != 0:
                    self._aug_err.zero_()
                    raise IndexError("ContraRec: the view builder met %s" % " and ".join(
                        t for bit, t in ((1, "a history length outside [1, history_max]"), (2, "a row id outside the history table"))
                        if word & bit))

        # ------------------------------------------------------------------------------------ the reference's methods
        def _encode(self, history, lengths):
            block_fn = self._native_block if self._use_block_native(history.shape[1]) else None
            return self.encoder(self.item_embeddings(history), lengths, block_fn)

        def forward(self, feed_dict):
            return self._encode(feed_dict["history_items"], feed_dict["lengths"])

        def predict(self, feed_dict):
            pos_item, lengths = feed_dict["pos_item"], feed_dict["lengths"]
            pos_e = self.item_embeddings(pos_item)
            neg_e = self.item_embeddings(feed_dict["neg_items"].reshape(-1))
            user_e = self.forward(feed_dict)
            pos = (user_e * pos_e).sum(dim=1)
            neg = (user_e * neg_e).sum(dim=1)
            ctc_loss = -torch.log(1e-10 + torch.sigmoid(pos - neg)).mean()               # BPRLoss, loss.py:38
            his_a = self._encode(feed_dict["history_items_a"], lengths)
            his_b = self._encode(feed_dict["history_items_b"], lengths)
            if self._use_ccc_native(his_a.shape[0]):
                ccc_loss = hip_ops.supcon_loss(torch.cat([his_a, his_b], dim=0), pos_item, self.ccc_temp)
            else:
                features = F.normalize(torch.stack([his_a, his_b], dim=1), dim=-1)
                ccc_loss = contra_loss(features, pos_item, self.ccc_temp)
            self.last_losses = (ctc_loss.detach(), ccc_loss.detach())
            return ctc_loss + self.gamma * ccc_loss

        def full_predict(self, feed_dict):
            # all item_num + 1 rows: the reference ranks the mask-token column too (ContraRec.py:98-104)
            self._sync_tables()
            return torch.matmul(self.forward(feed_dict), self.item_embeddings.weight.t())

        # The query protocol of HipRunner's device evaluation (--seq_eval_native 1) and recommend_rows, as SASRec's.
        def eval_queries(self, history_items, lengths):
            """[n, D] query vectors of rows with these histories ([n, T] left-aligned, zero-padded) and lengths: `forward` in
            eval mode without autograd, on the block path `forward` itself picks.  The training flag is restored."""
            was_training = self.training
            self.eval()
            try:
                with torch.no_grad():
                    return self.forward({"history_items": history_items, "lengths": lengths})
            finally:
                self.train(was_training)

        def eval_items(self):
            """[item_num + 1, D] item side of the scores: full_predict's second operand, the mask-token row included"""
            self._sync_tables()
            return self.item_embeddings.weight

        class Dataset(sequential_model_cls.Dataset):
            """ContraRec.py:106-138.  The NumPy draws are the reference's, in its order: the global stream is consumed alike."""

            def reorder_op(self, seq):
                ratio = np.random.beta(a=self.model.beta_a, b=self.model.beta_b)
                select_len = int(len(seq) * ratio)
                start = np.random.randint(0, len(seq) - select_len + 1)
                idx_range = np.arange(len(seq))
                np.random.shuffle(idx_range[start: start + select_len])
                return seq[idx_range]

            def mask_op(self, seq):
                ratio = np.random.beta(a=self.model.beta_a, b=self.model.beta_b)
                selected_len = int(len(seq) * ratio)
                mask = np.full(len(seq), False)
                mask[:selected_len] = True
                np.random.shuffle(mask)
                seq[mask] = self.model.mask_token
                return seq

            def augment(self, seq):
                aug_seq = np.array(seq).copy()
                if np.random.rand() > 0.5:
                    return self.mask_op(aug_seq)
                return self.reorder_op(aug_seq)

            def _get_feed_dict(self, index):
                feed_dict = super()._get_feed_dict(index)
                if self.phase == "train":
                    feed_dict["history_items_a"] = self.augment(feed_dict["history_items"])
                    feed_dict["history_items_b"] = self.augment(feed_dict["history_items"])
                return feed_dict

    ContraRec.__qualname__ = "ContraRec"
    return ContraRec


ContraRec = make_contrarec(host.SequentialModel)


def bind(reference_sequential_model_cls):
    return make_contrarec(reference_sequential_model_cls)
