"""TiSASRec (Li et al., WSDM 2020): SASRec whose attention also sees the time gap between every pair of history items.

The reference ships the layer — ``TimeIntervalMultiHeadAttention`` / ``TimeIntervalTransformerLayer`` (src/utils/layers.py:89-170)
— and puts ``history_times`` into every sequential feed dict, but has no model file that uses either; this module defines the
model around that layer:

  min_interval[u] = min(smallest positive difference between any two of u's timestamps, 65535), 65535 without one; computed once
                    from ``corpus.user_his`` and kept as an int64 buffer indexed by user id, so a batch needs only ``user_id``
  valid    = history > 0                      position = (lengths[:, None] - arange(T)[None, :]) * valid
  x        = item_embedding(history)          pos_k, pos_v = the two position tables at `position`
  interval[b, i, j] = min(|t_i - t_j| // min_interval[user_b], time_max)      integer floor division in int64
  causal mask, ``num_layers`` blocks, output * valid, the row at lengths - 1; BPR loss (loss.py:38) as SASRec.

Parameter names are the layer's (``transformer_block.N.masked_attn_head.{v,k,q}_linear``, ``layer_norm1``, ``linear1``,
``linear2``, ``layer_norm2``; ``kq_same=False``), the tables are ``item_embedding`` (a ``HipEmbedding``, padding row 0),
``position_{k,v}_embedding`` [history_max + 1, D] and ``time_{k,v}_embedding`` [time_max + 1, D].

Two paths:
  --ti_native 0 (default)  exactly the ops of layers.py:89-170 under autograd, the shift by the call's global score maximum
                           included: two gathered [B, T, T, D] arrays per block.
  --ti_native 1            the projections and the position terms stay torch ops; the attention is one call of
                           ``hip_ops.ti_attention`` (wr_tiattn.hip, K25): the intervals are formed in the kernel from
                           ``history_times`` and the table rows are looked up while the scores are — no [B, T, T, D] and no
                           [B, T, T] array.  Dropout, residuals, layer norms and the feed-forward stay torch ops (torch's
                           generator).  The kernel shifts by each row's own maximum.
A shape the kernels do not take is logged once and keeps the torch path.  ``--emb_lazy`` as SASRec.
"""
import logging

import numpy as np
import torch
import torch.nn as nn

from . import hip_ops, host
from .sasrec import EmbLazyMixin, HipEmbedding, _xavier_normal_all
from .softmax_loss import SoftmaxLossMixin

MIN_INTERVAL_CAP = 65535


def user_min_intervals(user_his, n_users):
    """int64 [n_users]: per user the smallest positive difference between any two of its timestamps, capped at 65535; 65535 for
    a user without one (a single interaction, repeated timestamps only, or no history)."""
    out = np.full(int(n_users), MIN_INTERVAL_CAP, np.int64)
    for u, his in user_his.items():
        if len(his) < 2:
            continue
        t = np.unique(np.asarray([x[1] for x in his], dtype=np.int64))      # sorted: the smallest gap is between neighbours
        if t.size >= 2:
            out[int(u)] = min(int(np.diff(t).min()), MIN_INTERVAL_CAP)
    return out


def interval_matrix(times, min_interval, time_max):
    """[B, T, T] int64: min(|t_i - t_j| // m_b, time_max) by integer floor division (a float division can land on the other side
    of an integer)"""
    gap = (times[:, :, None] - times[:, None, :]).abs()
    return torch.clamp(torch.div(gap, min_interval.clamp(min=1)[:, None, None], rounding_mode="floor"), max=int(time_max))


def ti_attention_torch(q, k, v, inter_k, inter_v, mask, n_heads):
    """layers.py:116-146 as written, after the projections: q, k, v [B, T, D] (position terms already in k and v), inter_k /
    inter_v [B, T, T, D] gathered interval rows, mask [1, 1, T, T] -> [B, T, D].  The scores are shifted by the GLOBAL maximum
    before the softmax (:143); this layer has no NaN fill."""
    bs, seq_len, d_model = k.size(0), k.size(1), k.size(2)
    d_k = d_model // n_heads
    k = k.view(bs, seq_len, n_heads, d_k).transpose(1, 2)
    q = q.view(bs, seq_len, n_heads, d_k).transpose(1, 2)
    v = v.view(bs, seq_len, n_heads, d_k).transpose(1, 2)
    inter_k = inter_k.view(bs, seq_len, seq_len, n_heads, d_k).transpose(2, 3).transpose(1, 2)
    inter_v = inter_v.view(bs, seq_len, seq_len, n_heads, d_k).transpose(2, 3).transpose(1, 2)   # bs, head, T, T, d_k
    scores = torch.matmul(q, k.transpose(-2, -1))
    scores += (q[:, :, :, None, :] * inter_k).sum(-1)
    scores = scores / d_k ** 0.5
    scores.masked_fill_(mask == 0, -np.inf)
    scores = (scores - scores.max()).softmax(dim=-1)
    output = torch.matmul(scores, v)
    output += (scores[:, :, :, :, None] * inter_v).sum(-2)
    return output.transpose(1, 2).reshape(bs, -1, d_model)


class _TiAttention(nn.Module):
    """layers.py:89-146 as written (kq_same=False): k and v get the position terms after their projections, the scores the
    products of q with the gathered interval rows, the shift by the GLOBAL maximum before the softmax; no NaN fill."""

    def __init__(self, d_model, n_heads):
        super().__init__()
        self.d_model, self.h, self.d_k = d_model, n_heads, d_model // n_heads
        self.v_linear = nn.Linear(d_model, d_model)
        self.k_linear = nn.Linear(d_model, d_model)
        self.q_linear = nn.Linear(d_model, d_model)

    def forward(self, q, k, v, pos_k, pos_v, inter_k, inter_v, mask):
        return ti_attention_torch(self.q_linear(q), self.k_linear(k) + pos_k, self.v_linear(v) + pos_v, inter_k, inter_v, mask,
                                  self.h)

    def forward_native(self, x, pos_k, pos_v, times, min_interval, time_k, time_v, time_max, err_word):
        k = self.k_linear(x) + pos_k
        v = self.v_linear(x) + pos_v
        return hip_ops.ti_attention(self.q_linear(x), k, v, times, min_interval, time_k, time_v, self.h, time_max, err_word)


class _TiBlock(nn.Module):
    """layers.py:149-170: post-norm residual time-interval attention + 2-layer ReLU feed-forward."""

    def __init__(self, d_model, d_ff, n_heads, dropout):
        super().__init__()
        self.masked_attn_head = _TiAttention(d_model, n_heads)
        self.layer_norm1 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)
        self.linear1 = nn.Linear(d_model, d_ff)
        self.linear2 = nn.Linear(d_ff, d_model)
        self.layer_norm2 = nn.LayerNorm(d_model)
        self.dropout2 = nn.Dropout(dropout)

    def _rest(self, context, seq):
        context = self.layer_norm1(self.dropout1(context) + seq)
        output = self.linear2(self.linear1(context).relu())
        return self.layer_norm2(self.dropout2(output) + context)

    def forward(self, seq, pos_k, pos_v, inter_k, inter_v, mask):
        return self._rest(self.masked_attn_head(seq, seq, seq, pos_k, pos_v, inter_k, inter_v, mask), seq)

    def forward_native(self, seq, pos_k, pos_v, times, min_interval, time_k, time_v, time_max, err_word=None):
        return self._rest(self.masked_attn_head.forward_native(seq, pos_k, pos_v, times, min_interval, time_k, time_v, time_max,
                                                               err_word), seq)


def make_tisasrec(sequential_model_cls):
    class TiSASRec(EmbLazyMixin, SoftmaxLossMixin, sequential_model_cls):
        reader = "SeqReader"
        runner = "BaseRunner"
        extra_log_args = ["emb_size", "num_layers", "num_heads", "time_max", "train_loss", "softmax_native"]
        needs_history_times = True       # HipRunner's native loops carry history_times and user_id to this model

        @staticmethod
        def parse_model_args(parser):
            parser.add_argument("--emb_size", type=int, default=64, help="Size of embedding vectors.")
            parser.add_argument("--num_layers", type=int, default=1, help="Number of self-attention layers.")
            parser.add_argument("--num_heads", type=int, default=4, help="Number of attention heads.")
            parser.add_argument("--dropout", type=float, default=0.1, help="Dropout probability.")
            parser.add_argument("--time_max", type=int, default=512, help="Max time intervals.")
            parser.add_argument("--ti_native", type=int, default=0, choices=[0, 1],
                                help="1: the time-interval attention by the fused HIP kernels (forward and backward), no "
                                     "[B, T, T, D] gather; 0: torch ops + autograd.")
            EmbLazyMixin.add_emb_lazy_arg(parser)
            SoftmaxLossMixin.add_softmax_loss_args(parser)
            return sequential_model_cls.parse_model_args(parser)

        def __init__(self, args, corpus):
            super().__init__(args, corpus)
            self.emb_size, self.max_his, self.time_max = int(args.emb_size), args.history_max, int(args.time_max)
            self.num_heads, self.dropout = int(args.num_heads), float(args.dropout)
            self.item_embedding = HipEmbedding(self.item_num, self.emb_size, padding_idx=0)
            self.position_k_embedding = nn.Embedding(self.max_his + 1, self.emb_size)
            self.position_v_embedding = nn.Embedding(self.max_his + 1, self.emb_size)
            self.time_k_embedding = nn.Embedding(self.time_max + 1, self.emb_size)
            self.time_v_embedding = nn.Embedding(self.time_max + 1, self.emb_size)
            self.transformer_block = nn.ModuleList([_TiBlock(self.emb_size, self.emb_size, self.num_heads, self.dropout)
                                                    for _ in range(args.num_layers)])
            self.apply(_xavier_normal_all)
            self.register_buffer("min_interval", torch.from_numpy(user_min_intervals(corpus.user_his, self.user_num)))
            self.ti_native = bool(int(getattr(args, "ti_native", 0)))
            self._ti_native_ok = {}      # per history length, decided at its first batch: the library says what it takes
            self._ti_err = None          # device error word of the kernels (a scale below 1), read by check_train_extras()
            self._install_softmax_loss(args)
            self._install_emb_lazy(args, self.item_embedding)

        def _use_ti_native(self, T):
            if not self.ti_native:
                return False
            if T not in self._ti_native_ok:
                ok = hip_ops.ti_attention_supports(self.emb_size, self.num_heads, T, self.time_max)
                if not ok and not any(v is False for v in self._ti_native_ok.values()):
                    logging.warning("--ti_native 1: the attention kernels do not take emb_size=%d num_heads=%d history=%d "
                                    "time_max=%d; keeping the torch path", self.emb_size, self.num_heads, T, self.time_max)
                self._ti_native_ok[T] = ok
            return self._ti_native_ok[T]

        def check_train_extras(self):
            """HipRunner.fit calls this once per epoch: raise if an attention call since the last check met a scale below 1 (one read of the device word)"""
            if self._ti_err is not None and int(self._ti_err.item()) != 0:
                self._ti_err.zero_()
                raise ValueError("TiSASRec: a min_interval below 1 reached the attention kernels (clamped to 1)")

        def forward(self, feed_dict):
            history, lengths = feed_dict["history_items"], feed_dict["lengths"]
            times, users = feed_dict["history_times"], feed_dict["user_id"]
            bsz, T = history.shape
            dev = history.device
            valid = (history > 0).long()
            position = (lengths[:, None] - torch.arange(T, device=dev)[None, :]) * valid
            x = self.item_embedding(history)
            pos_k, pos_v = self.position_k_embedding(position), self.position_v_embedding(position)
            scale = self.min_interval[users]
            if self._use_ti_native(T):
                if self._ti_err is None or self._ti_err.device != dev:
                    self._ti_err = torch.zeros(1, dtype=torch.int32, device=dev)
                times = times.to(torch.int64).contiguous()
                for blk in self.transformer_block:
                    x = blk.forward_native(x, pos_k, pos_v, times, scale, self.time_k_embedding.weight,
                                           self.time_v_embedding.weight, self.time_max, self._ti_err)
            else:
                interval = interval_matrix(times.to(torch.int64), scale, self.time_max)
                inter_k, inter_v = self.time_k_embedding(interval), self.time_v_embedding(interval)
                mask = torch.tril(torch.ones(1, 1, T, T, dtype=torch.int32, device=dev))
                for blk in self.transformer_block:
                    x = blk(x, pos_k, pos_v, inter_k, inter_v, mask)
            x = x * valid[:, :, None].float()
            return x[torch.arange(bsz, device=dev), lengths - 1, :]

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

        # The query protocol of HipRunner's device evaluation (--seq_eval_native 1) and recommend_rows, with the two extra
        # columns a model that declares needs_history_times is handed.
        def eval_queries(self, history_items, lengths, history_times=None, user_id=None):
            """[n, D] query vectors of rows with these histories ([n, T] left-aligned, zero-padded), their timestamps and users:
            `forward` in eval mode without autograd, on the attention path `forward` itself picks."""
            if history_times is None or user_id is None:
                raise ValueError("TiSASRec.eval_queries needs history_times and user_id: the attention sees the time gaps, "
                                 "scaled per user")
            was_training = self.training
            self.eval()
            try:
                with torch.no_grad():
                    return self.forward({"history_items": history_items, "lengths": lengths, "history_times": history_times,
                                         "user_id": user_id})
            finally:
                self.train(was_training)

        def eval_items(self):
            """[n_items, D] item side of the scores: full_predict's second operand"""
            self._sync_tables()
            return self.item_embedding.weight

    TiSASRec.__qualname__ = "TiSASRec"
    return TiSASRec


TiSASRec = make_tisasrec(host.SequentialModel)


def bind(reference_sequential_model_cls):
    return make_tisasrec(reference_sequential_model_cls)
