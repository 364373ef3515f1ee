"""IF4Rec (reference src/models/sequential/IF4Rec.py): K interest vectors per history — an attention pooling of item + position
rows with K score heads — refined by transformer blocks over the K interest tokens; a row's score against an item is the
MAXIMUM over its interests.

The reference file no longer fits its own launcher: ``self.apply(self.init_weights)`` names a method no base class has,
``forward`` reads ``feed_dict['item_id']`` which no Dataset produces, and there is no ``predict`` / ``full_predict``.  The
formulas are sound and are kept exactly as written (:87-118):
  mask = history > 0 (not ``lengths``), position t for a valid entry and 0 otherwise, scores W2(leaky_relu(W1(his + pos))) with
  masked entries at -inf, softmax over T after the shift by the call's global maximum, NaN -> 0, interests = weighted sums of
  his + pos, then ``encoder_layer`` blocks (d_ff = emb_size, ``n_head`` heads, no mask) when ``add_multi``.
  train (:110-115): the interest with the largest score against the positive scores every candidate; BPRLoss (loss.py:38).
  test  (:117-118): max over the interests, here as ``matmul(interests, items^T).max(1)`` — no [B, n, K, D] product.
One deviation, in the backward only: a row with no valid entry (a history that holds only item 0, which `history > 0` masks) passes
no gradient, where the reference's softmax backward would put NaN into every parameter (`interest_pool_torch`; the kernels alike).
Initialisation: the reference names a missing method; this uses ``xavier_normal_initialization`` (src/models/init.py:13-29,
``sasrec._xavier_normal_all``), as the reference's SASRec does.

Parameter names are the reference's, so checkpoints interchange: ``i_embeddings.weight`` (a ``HipEmbedding`` without padding
index), ``p_embeddings.weight``, ``W1``, ``W2``, ``transformer_block.N.*`` with ``sasrec._Block``'s names.

Two native paths, both off by default:
  --interest_native 1   gather, scores, masked softmax and the K weighted sums in one launch, their gradients in two
                        (``hip_ops.interest_pool``, wr_if4rec.hip, K18): no [B, T, D] or [B, K, T, D] array.
  --block_native 1      each block over the K interest tokens by ``hip_ops.sasrec_block(key_lengths = K for every row)`` — the
                        unmasked case of the key-length kernels (K13) — when ``sasblock_supports(D, D, n_head, K)`` (n_head in
                        {1, 2, 4}; the default 8 heads keep torch); dropout by the kernel's counter-based generator, seeded per
                        step and layer as SASRec's.
A shape the kernels do not take is logged once and keeps the torch path.

There is no ``eval_queries``: this model has no single query per row.  ``eval_interests`` / ``eval_items`` are the protocol of
``HipRunner``'s multi-interest ranking (wr_rank_eval_multi, K19) and, with ``--interest_topk_native 1``, of its top-K over the
interests (wr_topk_recommend_multi, K23): ``recommend_rows`` / ``recommend_next`` / ``--save_rec``.
"""
import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip_ops, host
from .sasrec import EmbLazyMixin, HipEmbedding, _Block, _xavier_normal_all


def interest_pool_torch(his_pos, valid, W1, W2):
    """IF4Rec.py:97-103 as written, on stock torch ops: his_pos [B, T, D], valid [B, T] (0 / 1) -> interests [B, K, D].
    One thing is added: a row with no valid entry (softmax of all -inf = NaN, set to 0 by :101) has its shifted scores replaced
    by 0 BEFORE the softmax and its weights set to 0 after it.  The forward is the reference's bit for bit; the backward passes
    such a row no gradient where the reference's passes NaN into every parameter (softmax's backward multiplies by the NaN
    output) — one history that holds only item 0 would end the training.  The pooling kernels do the same."""
    attn = W2(F.leaky_relu(W1(his_pos)))
    attn = attn.masked_fill(valid.unsqueeze(-1) == 0, -float("inf"))
    attn = attn.transpose(-1, -2)
    dead = (valid.sum(dim=1) == 0)[:, None, None]
    attn = (attn - attn.max()).masked_fill(dead, 0).softmax(dim=-1)
    attn = attn.masked_fill(dead, 0)
    attn = attn.masked_fill(torch.isnan(attn), 0)
    return (his_pos[:, None, :, :] * attn[:, :, :, None]).sum(-2)


def make_if4rec(sequential_model_cls):
    class IF4Rec(EmbLazyMixin, sequential_model_cls):
        reader = "SeqReader"
        runner = "BaseRunner"
        extra_log_args = ["emb_size", "attn_size", "K", "encoder_layer", "n_head", "encoder_dropout", "add_pos", "add_multi"]

        @staticmethod
        def parse_model_args(parser):
            parser.add_argument("--emb_size", type=int, default=64, help="Size of embedding vectors.")
            parser.add_argument("--attn_size", type=int, default=8, help="Size of attention vectors.")
            parser.add_argument("--K", type=int, default=2, help="Number of hidden intent.")
            parser.add_argument("--add_pos", type=int, default=1, help="Whether add position embedding.")
            parser.add_argument("--encoder_layer", type=int, default=1, help="Number of encoder layer.")
            parser.add_argument("--n_head", type=int, default=8, help="Number of multi-attention head")
            parser.add_argument("--encoder_dropout", type=float, default=0.1, help="encoder dropout")
            parser.add_argument("--add_multi", type=int, default=1, help="Whether add multi-head.")
            parser.add_argument("--interest_native", type=int, default=0, choices=[0, 1],
                                help="1: interest pooling (gather, scores, softmax, weighted sums) and its gradients by the fused "
                                     "HIP kernels; 0: torch ops + autograd.")
            parser.add_argument("--block_native", type=int, default=0, choices=[0, 1],
                                help="1: each block over the interest tokens by the fused HIP kernels (n_head in {1, 2, 4}); "
                                     "0: torch ops + autograd.")
            EmbLazyMixin.add_emb_lazy_arg(parser)
            return sequential_model_cls.parse_model_args(parser)

        def __init__(self, args, corpus):
            super().__init__(args, corpus)
            self.emb_size, self.attn_size, self.K = int(args.emb_size), int(args.attn_size), int(args.K)
            self.add_pos, self.add_multi = int(args.add_pos), int(args.add_multi)
            self.max_his = args.history_max
            self.encoder_layer, self.n_head = int(args.encoder_layer), int(args.n_head)
            self.encoder_dropout = float(args.encoder_dropout)
            self.i_embeddings = HipEmbedding(self.item_num, self.emb_size)
            if self.add_pos:
                self.p_embeddings = nn.Embedding(self.max_his + 1, self.emb_size)
            self.W1 = nn.Linear(self.emb_size, self.attn_size)
            self.W2 = nn.Linear(self.attn_size, self.K)
            self.transformer_block = nn.ModuleList([_Block(self.emb_size, self.emb_size, self.n_head, self.encoder_dropout)
                                                    for _ in range(self.encoder_layer)])
            self.apply(_xavier_normal_all)
            self.interest_native = bool(int(getattr(args, "interest_native", 0)))
            self.block_native = bool(int(getattr(args, "block_native", 0)))
            self._interest_native_ok = {}    # per history length, decided at its first batch: the library says what it takes
            self._block_native_ok = None
            self._block_seed = int(getattr(args, "random_seed", 0)) * 0x9E3779B97F4A7C15
            self._block_calls = 0            # one dropout stream per training step and layer
            self._id_err = None              # device error word of the history ids, read by check_history_ids()
            self._key_len = None             # [B] tensor of K: every interest token is a key
            # the pooling kernels read the table's rows themselves (wr_if4rec.hip): they would see rows that lag
            self._install_emb_lazy(args, self.i_embeddings, blocked="--interest_native 1 reads the item table inside the pooling "
                                   "kernels" if self.interest_native else None)

        n_interests = property(lambda self: self.K)

        # ------------------------------------------------------------------------------------ native paths
        def _use_interest_native(self, T):
            if not self.interest_native:
                return False
            if T not in self._interest_native_ok:
                ok = hip_ops.interest_pool_supports(self.emb_size, self.attn_size, self.K, T)
                if not ok and not any(v is False for v in self._interest_native_ok.values()):
                    logging.warning("--interest_native 1: the pooling kernels do not take emb_size=%d attn_size=%d K=%d history=%d; "
                                    "keeping the torch path", self.emb_size, self.attn_size, self.K, T)
                self._interest_native_ok[T] = ok
            return self._interest_native_ok[T]

        def _use_block_native(self):
            if not self.block_native:
                return False
            if self._block_native_ok is None:
                self._block_native_ok = hip_ops.sasblock_supports(self.emb_size, self.emb_size, self.n_head, self.K)
                if not self._block_native_ok:
                    logging.warning("--block_native 1: the block kernels do not take emb_size=%d n_head=%d over %d interest "
                                    "tokens; keeping the torch path", self.emb_size, self.n_head, self.K)
            return self._block_native_ok

        def check_history_ids(self):
            """raise if a pooling call since the last check was handed an item id outside the table (one read of the device word)"""
            if self._id_err is not None and int(self._id_err.item()) != 0:
                self._id_err.zero_()
                raise IndexError("IF4Rec: a history item id outside [0, item_num) reached the pooling kernels")

        def _blocks(self, x):
            bsz = x.shape[0]
            if self._use_block_native():
                if self._key_len is None or self._key_len.numel() < bsz or self._key_len.device != x.device:
                    self._key_len = torch.full((bsz,), self.K, dtype=torch.int64, device=x.device)
                for blk in self.transformer_block:
                    x = hip_ops.sasrec_block(x, blk, self.n_head, self.encoder_dropout, self._block_seed + self._block_calls,
                                             self.training, key_lengths=self._key_len[:bsz])
                    self._block_calls += int(self.training)
                return x
            mask = torch.ones(1, 1, self.K, self.K, dtype=torch.int32, device=x.device)     # no mask (TransformerLayer(seq))
            for blk in self.transformer_block:
                x = blk(x, mask)
            return x

        # ------------------------------------------------------------------------------------ the reference's methods
        def forward(self, feed_dict):
            """interest vectors [B, K, D] of the rows' histories (IF4Rec.py:87-107)"""
            history = feed_dict["history_items"]
            T = history.shape[1]
            if self._use_interest_native(T):
                if self._id_err is None:
                    self._id_err = torch.zeros(1, dtype=torch.int32, device=history.device)
                interests = hip_ops.interest_pool(self.i_embeddings.weight, self.p_embeddings.weight if self.add_pos else None,
                                                  history, self.W1.weight, self.W1.bias, self.W2.weight, self.W2.bias,
                                                  err_word=self._id_err)
            else:
                valid = (history > 0).long()
                his_pos = self.i_embeddings(history)
                if self.add_pos:
                    position = torch.arange(T, device=history.device)[None, :] * valid          # :91
                    his_pos = his_pos + self.p_embeddings(position)
                interests = interest_pool_torch(his_pos, valid, self.W1, self.W2)
            if self.add_multi:
                interests = self._blocks(interests)
            return interests

        def predict(self, feed_dict):
            interests = self.forward(feed_dict)
            bsz = interests.shape[0]
            i_ids = torch.cat([feed_dict["pos_item"].reshape(-1, 1), feed_dict["neg_items"].reshape(bsz, -1)], dim=1)
            i_vectors = self.i_embeddings(i_ids.reshape(-1)).view(bsz, i_ids.shape[1], -1)
            target_pred = (interests * i_vectors[:, 0][:, None, :]).sum(-1)                      # :111-112
            idx_select = target_pred.max(-1)[1]
            user_vector = interests[torch.arange(bsz, device=interests.device), idx_select, :]
            prediction = (user_vector[:, None, :] * i_vectors).sum(-1)                           # :115
            self.last_prediction = prediction.detach()
            # BPRLoss (loss.py:38) of column 0 against the rest
            return -torch.log(1e-10 + torch.sigmoid(prediction[:, :1] - prediction[:, 1:])).mean()

        def full_predict(self, feed_dict):
            self._sync_tables()
            return torch.matmul(self.forward(feed_dict), self.i_embeddings.weight.t()).max(1)[0]

        # The interest protocol of HipRunner's device evaluation (--seq_eval_native 1): a model whose score of row e against
        # item j is max_k <eval_interests(...)[e, k], eval_items()[j]>.
        def eval_interests(self, history_items, lengths):
            """[n, K, D] interest vectors of rows with these histories ([n, T] left-aligned, zero-padded): `forward` in eval
            mode without autograd, on the paths `forward` itself picks.  The training flag is restored."""
            was_training = self.training
            self.eval()
            try:
                with torch.no_grad():
                    return self.forward({"history_items": history_items, "lengths": lengths})
            finally:
                self.train(was_training)

        def eval_items(self):
            """[item_num, D] item side of the scores: full_predict's second operand"""
            self._sync_tables()
            return self.i_embeddings.weight

    IF4Rec.__qualname__ = "IF4Rec"
    return IF4Rec


IF4Rec = make_if4rec(host.SequentialModel)


def bind(reference_sequential_model_cls):
    return make_if4rec(reference_sequential_model_cls)
