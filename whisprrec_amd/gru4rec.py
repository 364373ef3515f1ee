"""GRU4Rec (Hidasi et al., ICLR 2016): the recurrent sequential baseline — a one-layer GRU over the history's item embeddings.

The reference ships no such file (ReChorus, which it descends from, does); this module is the definition, in SASRec's protocol:

  x        = item_embedding(history_items)        [B, T, E], histories left-aligned and zero-padded
  h_t      = GRU(x_t, h_{t-1}), h_0 = 0           torch's cell and gate order (r, z, n), over row b's first lengths[b] steps
  user_e   = out(h_last)                          h_last[b] = the state after step lengths[b] - 1;  out: Linear(hidden, emb)
  BPR loss (loss.py:38) against one sampled negative as SASRec, or ``--train_loss softmax`` through SoftmaxLossMixin (the query
  width is emb_size, what ``out`` produces).

Parameters: ``item_embedding`` (a ``HipEmbedding``, padding row 0), ``rnn`` (``nn.GRU(emb_size, hidden_size, batch_first=True)``:
``weight_ih_l0`` [3H, E], ``weight_hh_l0`` [3H, H], ``bias_ih_l0``, ``bias_hh_l0`` [3H]; nn.GRU's own initialisation) and ``out``.

Two paths:
  --gru_native 0 (default)  ``rnn(x)`` over the padded batch, then the row at lengths - 1.  A GRU is causal and the rows are
                            left-aligned, so this equals ReChorus's sort / pack_padded_sequence / unsort form without its host
                            read of the lengths (tests/test_gru4rec_contract.py pins the equality).
  --gru_native 1            ``hip_ops.gru_last`` (wr_gru.hip, K27): one launch forward, two backward; rows stop at their own
                            length, the padded steps are never read, and autograd keeps one [B, T, H] array instead of the
                            per-step gate activations.  A length of 0 gives a zero state and no gradient; a length above T acts
                            as T (the stock path would index out of range for either).
A shape the kernels do not take is logged once and keeps the stock path.  ``--emb_lazy`` as SASRec.

``--num_layers L`` (default 1) stacks L GRUs (``nn.GRU(..., num_layers=L)``, no dropout between them); with L = 1 the module, its
state_dict keys and every result are those of the one-layer model.  Under --gru_native 1 the layers 0 .. L - 2 run through
``hip_ops.gru_seq`` (every state, zero past the length) and the last through ``hip_ops.gru_last``.
"""
import logging

import torch
import torch.nn as nn

from . import hip_ops, host
from .sasrec import EmbLazyMixin, HipEmbedding, _xavier_normal_all
from .softmax_loss import SoftmaxLossMixin


_GRU_PARAMS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def make_gru4rec(sequential_model_cls):
    class GRU4Rec(EmbLazyMixin, SoftmaxLossMixin, sequential_model_cls):
        reader = "SeqReader"
        runner = "BaseRunner"
        extra_log_args = ["emb_size", "hidden_size", "train_loss", "softmax_native"]

        @staticmethod
        def parse_model_args(parser):
            parser.add_argument("--emb_size", type=int, default=64, help="Size of embedding vectors.")
            parser.add_argument("--hidden_size", type=int, default=64, help="Size of hidden vectors in GRU.")
            parser.add_argument("--num_layers", type=int, default=1, help="Number of stacked GRU layers.")
            parser.add_argument("--gru_native", type=int, default=0, choices=[0, 1],
                                help="1: the GRU recurrence by the fused HIP kernels (forward and backward), rows stop at their "
                                     "own length; 0: nn.GRU over the padded batch + autograd.")
            EmbLazyMixin.add_emb_lazy_arg(parser)
            SoftmaxLossMixin.add_softmax_loss_args(parser)
            return sequential_model_cls.parse_model_args(parser)

        def __init__(self, args, corpus):
            super().__init__(args, corpus)
            self.emb_size, self.hidden_size, self.max_his = int(args.emb_size), int(args.hidden_size), args.history_max
            self.item_embedding = HipEmbedding(self.item_num, self.emb_size, padding_idx=0)
            self.num_layers = int(getattr(args, "num_layers", 1))
            if self.num_layers < 1:
                raise ValueError("--num_layers must be at least 1 (got %d)" % self.num_layers)
            self.rnn = nn.GRU(input_size=self.emb_size, hidden_size=self.hidden_size, num_layers=self.num_layers, batch_first=True)
            self.out = nn.Linear(self.hidden_size, self.emb_size)
            self.apply(_xavier_normal_all)      # embeddings and linears; the GRU keeps nn.GRU's own initialisation
            self.gru_native = bool(int(getattr(args, "gru_native", 0)))
            self._gru_native_ok = {}     # per history length, decided at its first batch: the library says what it takes
            self._install_softmax_loss(args)
            self._install_emb_lazy(args, self.item_embedding)

        def _use_gru_native(self, T):
            if not self.gru_native:
                return False
            if T not in self._gru_native_ok:
                ok = hip_ops.gru_supports(self.emb_size, self.hidden_size, T) and (
                    self.num_layers == 1 or hip_ops.gru_supports(self.hidden_size, self.hidden_size, T))
                if not ok and not any(v is False for v in self._gru_native_ok.values()):
                    logging.warning("--gru_native 1: the GRU kernels do not take emb_size=%d hidden_size=%d history=%d; keeping "
                                    "the torch path", self.emb_size, self.hidden_size, T)
                self._gru_native_ok[T] = ok
            return self._gru_native_ok[T]

        def forward(self, feed_dict):
            history, lengths = feed_dict["history_items"], feed_dict["lengths"]
            bsz, T = history.shape
            x = self.item_embedding(history)
            if self._use_gru_native(T):
                for layer in range(self.num_layers - 1):      # the lower layers hand every state up
                    x = hip_ops.gru_seq(x, lengths, *(getattr(self.rnn, "%s_l%d" % (n, layer)) for n in _GRU_PARAMS))
                h_last = hip_ops.gru_last(x, lengths, *(getattr(self.rnn, "%s_l%d" % (n, self.num_layers - 1)) for n in _GRU_PARAMS))
            else:
                output, _ = self.rnn(x)
                h_last = output[torch.arange(bsz, device=history.device), lengths - 1, :]
            return self.out(h_last)

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
            in eval mode without autograd, on the GRU path `forward` itself picks.  The training flag is restored."""
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

    GRU4Rec.__qualname__ = "GRU4Rec"
    return GRU4Rec


GRU4Rec = make_gru4rec(host.SequentialModel)


def bind(reference_sequential_model_cls):
    return make_gru4rec(reference_sequential_model_cls)
