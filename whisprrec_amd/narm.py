"""NARM (Li et al., CIKM 2017): a global and a local GRU encoder over the history's item embeddings; every state of the local one
is pooled by an additive attention against the global encoder's last state.

The reference ships no such file (ReChorus, which it descends from, does); this module is the definition, in SASRec's protocol:

  x        = item_embedding(history_items)          [B, T, E], histories left-aligned and zero-padded
  h_g      = the last state of encoder_g(x)         [B, H]: the state after step lengths[b] - 1
  hs_l     = every state of encoder_l(x)            [B, T, H]
  e_t      = attention_out(sigmoid(A1 h_g + A2 hs_l[t]))      for t < lengths[b]; no softmax (NARM's own form)
  c_l      = sum_t e_t hs_l[t]                      [B, H]
  user_e   = out(cat(c_l, h_g))                     out: Linear(2 hidden, emb, bias=False)
  BPR loss (loss.py:38) against one sampled negative as SASRec, or ``--train_loss softmax`` through SoftmaxLossMixin.

Parameters: ``item_embedding`` (a ``HipEmbedding``, padding row 0), ``encoder_g`` and ``encoder_l`` (``nn.GRU(emb_size,
hidden_size, batch_first=True)``, nn.GRU's own initialisation), ``A1`` and ``A2`` (``Linear(hidden, attention, bias=False)``),
``attention_out`` (``Linear(attention, 1, bias=False)``) and ``out``.

Two flags, both off by default:
  --gru_native 1     encoder_g through ``hip_ops.gru_last`` and encoder_l through ``hip_ops.gru_seq`` (wr_gru.hip, K27): rows stop
                     at their own length, hs_l is zero past it, the padded steps are never read.
  --pool_native 1    the pooling through ``hip_ops.narm_pool`` (wr_narm.hip, K28): one launch forward, two backward, no
                     [B, T, A] array; the states past a row's length are never read.
Flag-off: ``nn.GRU`` over the padded batch, the row at lengths - 1, and the mask ``arange(T) < lengths`` on the attention values —
a GRU is causal and the rows are left-aligned, so this equals ReChorus's sort / pack_padded_sequence / unsort form with its mask
``history > 0`` (tests/test_narm_contract.py pins the equality).  A shape the kernels do not take is logged once and keeps the
stock path.  A length of 0 gives a zero query under both flags (the stock path would index out of range).  ``--emb_lazy`` as SASRec.
"""
import logging

import torch
import torch.nn as nn

from . import hip_ops, host
from .sasrec import EmbLazyMixin, HipEmbedding, _xavier_normal_all
from .softmax_loss import SoftmaxLossMixin


def _gru_params(rnn, layer=0):
    return tuple(getattr(rnn, "%s_l%d" % (n, layer)) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


def make_narm(sequential_model_cls):
    class NARM(EmbLazyMixin, SoftmaxLossMixin, sequential_model_cls):
        reader = "SeqReader"
        runner = "BaseRunner"
        extra_log_args = ["emb_size", "hidden_size", "attention_size", "train_loss", "softmax_native"]

        @staticmethod
        def parse_model_args(parser):
            parser.add_argument("--emb_size", type=int, default=64, help="Size of embedding vectors.")
            parser.add_argument("--hidden_size", type=int, default=64, help="Size of hidden vectors in the GRUs.")
            parser.add_argument("--attention_size", type=int, default=16, help="Size of the attention hidden space.")
            parser.add_argument("--gru_native", type=int, default=0, choices=[0, 1],
                                help="1: both GRU recurrences by the fused HIP kernels (forward and backward), rows stop at their "
                                     "own length; 0: nn.GRU over the padded batch + autograd.")
            parser.add_argument("--pool_native", type=int, default=0, choices=[0, 1],
                                help="1: the attention pooling by the fused HIP kernels (forward and backward); 0: torch ops over "
                                     "the padded batch + autograd.")
            EmbLazyMixin.add_emb_lazy_arg(parser)
            SoftmaxLossMixin.add_softmax_loss_args(parser)
            return sequential_model_cls.parse_model_args(parser)

        def __init__(self, args, corpus):
            super().__init__(args, corpus)
            self.emb_size, self.hidden_size, self.max_his = int(args.emb_size), int(args.hidden_size), args.history_max
            self.attention_size = int(args.attention_size)
            self.item_embedding = HipEmbedding(self.item_num, self.emb_size, padding_idx=0)
            self.encoder_g = nn.GRU(input_size=self.emb_size, hidden_size=self.hidden_size, batch_first=True)
            self.encoder_l = nn.GRU(input_size=self.emb_size, hidden_size=self.hidden_size, batch_first=True)
            self.A1 = nn.Linear(self.hidden_size, self.attention_size, bias=False)
            self.A2 = nn.Linear(self.hidden_size, self.attention_size, bias=False)
            self.attention_out = nn.Linear(self.attention_size, 1, bias=False)
            self.out = nn.Linear(2 * self.hidden_size, self.emb_size, bias=False)
            self.apply(_xavier_normal_all)      # embeddings and linears; the GRUs keep nn.GRU's own initialisation
            self.gru_native = bool(int(getattr(args, "gru_native", 0)))
            self.pool_native = bool(int(getattr(args, "pool_native", 0)))
            self._gru_native_ok, self._pool_native_ok = {}, {}     # per history length, decided at its first batch
            self._install_softmax_loss(args)
            self._install_emb_lazy(args, self.item_embedding)

        def _use_native(self, flag, seen, T, ask, what):
            if not flag:
                return False
            if T not in seen:
                ok = ask(T)
                if not ok and not any(v is False for v in seen.values()):
                    logging.warning("%s; keeping the torch path", what % T)
                seen[T] = ok
            return seen[T]

        def _use_gru_native(self, T):
            return self._use_native(self.gru_native, self._gru_native_ok, T,
                                    lambda t: hip_ops.gru_supports(self.emb_size, self.hidden_size, t),
                                    "--gru_native 1: the GRU kernels do not take emb_size=%d hidden_size=%d history=%%d"
                                    % (self.emb_size, self.hidden_size))

        def _use_pool_native(self, T):
            return self._use_native(self.pool_native, self._pool_native_ok, T,
                                    lambda t: hip_ops.narm_pool_supports(self.hidden_size, self.attention_size, t),
                                    "--pool_native 1: the pooling kernels do not take hidden_size=%d attention_size=%d history=%%d"
                                    % (self.hidden_size, self.attention_size))

        def forward(self, feed_dict):
            history, lengths = feed_dict["history_items"], feed_dict["lengths"]
            bsz, T = history.shape
            x = self.item_embedding(history)
            if self._use_gru_native(T):
                h_g = hip_ops.gru_last(x, lengths, *_gru_params(self.encoder_g))
                hs_l = hip_ops.gru_seq(x, lengths, *_gru_params(self.encoder_l))
            else:
                output_g, _ = self.encoder_g(x)
                h_g = output_g[torch.arange(bsz, device=history.device), lengths - 1, :]
                hs_l, _ = self.encoder_l(x)
            if self._use_pool_native(T):
                c_l = hip_ops.narm_pool(hs_l, h_g, lengths, self.A1.weight, self.A2.weight, self.attention_out.weight)
            else:
                u = self.A1(h_g)[:, None, :] + self.A2(hs_l)
                e = self.attention_out(torch.sigmoid(u)).squeeze(-1)
                e = e * (torch.arange(T, device=history.device)[None, :] < lengths[:, None]).to(e.dtype)
                c_l = (e[:, :, None] * hs_l).sum(dim=1)
            return self.out(torch.cat((c_l, h_g), dim=1))

        def predict(self, feed_dict):
            user_e = self.forward(feed_dict)
            if self.train_loss == "softmax":
                return self.softmax_loss(user_e, feed_dict["pos_item"])      # neg_items is ignored
            pos_e = self.item_embedding(feed_dict["pos_item"])
            neg_e = self.item_embedding(feed_dict["neg_items"].reshape(-1))
            pos = (user_e * pos_e).sum(dim=1)
            neg = (user_e * neg_e).sum(dim=1)
            return -torch.log(1e-10 + torch.sigmoid(pos - neg)).mean()                   # BPRLoss, loss.py:38

        def full_predict(self, feed_dict):
            self._sync_tables()
            return torch.matmul(self.forward(feed_dict), self.item_embedding.weight.t())

        # The query protocol of HipRunner's device evaluation (--seq_eval_native 1) and recommend_rows, as SASRec.
        def eval_queries(self, history_items, lengths):
            """[n, emb_size] query vectors of rows with these histories ([n, T] left-aligned, zero-padded) and lengths: `forward`
            in eval mode without autograd, on the paths `forward` itself picks.  The training flag is restored."""
            was_training = self.training
            self.eval()
            try:
                with torch.no_grad():
                    return self.forward({"history_items": history_items, "lengths": lengths})
            finally:
                self.train(was_training)

        def eval_items(self):
            """[n_items, emb_size] item side of the scores: full_predict's second operand"""
            self._sync_tables()
            return self.item_embedding.weight

    NARM.__qualname__ = "NARM"
    return NARM


NARM = make_narm(host.SequentialModel)


def bind(reference_sequential_model_cls):
    return make_narm(reference_sequential_model_cls)
