"""SASRec with its item-embedding gather / scatter on the HIP kernels (reference src/models/sequential/SASRec.py).

In scope for this path: ``item_embedding(padding_idx=0)`` looked up for the history, the positive
and the negative items (SASRec.py:84,105-106) and the scatter-add of its backward with the padding row's gradient
dropped.  ``HipEmbedding`` does exactly that through ``wr_gather_rows`` / ``wr_scatter_add_rows`` (sorted, deterministic).
The transformer block (src/utils/layers.py:8-86) is restated here with the reference's parameter names so checkpoints
interchange, and has two paths.  ``--block_native 0`` (default): stock PyTorch-ROCm ops under autograd.  ``--block_native 1``:
each block is one call of ``hip_ops.sasrec_block`` (wr_sasblock.hip, K13) — two launches forward, two backward, in training
and evaluation alike; its dropout mask is the kernel's own counter-based generator, seeded per step and per layer from
``--random_seed``.  A shape the kernels do not take is logged once and keeps the stock path.
``--emb_lazy 1`` (SASRec, ContraRec, IF4Rec; Adam and SGD): the item table gets no dense gradient.  ``HipEmbedding`` reads rows
through ``hip_ops.RowLazyTable.gather`` (wr_rowopt.hip, K22: the optimizer steps a row has missed are replayed on the way, nothing
is written), its backward hands (idx, grad_out) to ``RowLazyOptimizer``, which advances the table row by row exactly as the dense
optimizer would and leaves every other parameter to ``torch.optim``; ``EmbLazyMixin`` flushes before anything else reads the table.
``--train_loss softmax`` (SASRec, TiSASRec): ``predict`` returns the cross-entropy against the whole catalogue instead of BPRLoss
(softmax_loss.py; ``--softmax_native 1``: wr_softmax.hip, K26).
"""
import logging

import numpy as np
import torch
import torch.nn as nn

from . import hip_ops, host
from .softmax_loss import SoftmaxLossMixin


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, idx, padding_idx):
        ctx.save_for_backward(idx)
        ctx.shape, ctx.padding_idx = weight.shape, padding_idx
        return hip_ops.gather_rows(weight.detach(), idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        grad = torch.zeros(ctx.shape, dtype=torch.float32, device=grad_out.device)
        hip_ops.scatter_add_rows(grad, idx, grad_out.contiguous(), padding_idx=ctx.padding_idx)
        return grad, None, None


class HipEmbedding(nn.Module):
    """nn.Embedding replacement: same ``weight`` parameter name/shape; ``padding_idx`` rows receive no gradient (their
    stored values are returned as they are — xavier init overwrites the zero row in the reference too)."""

    def __init__(self, num_embeddings, embedding_dim, padding_idx=None):
        super().__init__()
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        self.padding_idx = -1 if padding_idx is None else int(padding_idx)
        self.weight = nn.Parameter(torch.empty(num_embeddings, embedding_dim))
        nn.init.normal_(self.weight)
        if padding_idx is not None:
            with torch.no_grad():
                self.weight[padding_idx].fill_(0)
        self._lazy = None           # a RowLazyOptimizer: the weight's optimizer state is advanced row by row (--emb_lazy 1)
        self._pending = []           # (lookup number, idx, grad_out) of the step's lookups whose backward has run
        self._lookups = 0            # training lookups since zero_grad
        self._marker = None

    def bind_lazy(self, optimizer):
        """lazy mode: forward reads rows as of the optimizer's current step (RowLazyTable.gather), backward hands (idx,
        grad_out) to the optimizer's sparse step instead of building a [num_embeddings, D] gradient; weight.grad stays None"""
        self._lazy = optimizer

    def forward(self, idx):
        if self._lazy is None:
            return _GatherRows.apply(self.weight, idx, self.padding_idx)
        if not (self.training and torch.is_grad_enabled()):
            return self._lazy.table().gather(idx, check=False)     # nothing is recorded
        if self._marker is None or self._marker.device != self.weight.device:
            # autograd calls a backward only below an input that requires grad; the weight must not be that input (it would
            # be handed a dense gradient), so a scalar stands in for it (bprmf._DeferredBprLoss's trick)
            self._marker = torch.zeros((), device=self.weight.device, requires_grad=True)
        self._lookups += 1
        return _LazyGatherRows.apply(self._marker, idx, self, self._lookups)


class _LazyGatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, marker, idx, module, number):
        ctx.save_for_backward(idx)
        ctx.module, ctx.number = module, number
        return module._lazy.table().gather(idx, check=False)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        ctx.module._pending.append((ctx.number, idx, grad_out.contiguous()))
        return None, None, None, None


class RowLazyOptimizer:
    """Duck-types what the runners need from ``model.optimizer`` (``zero_grad`` / ``step``, as bprmf.FusedOptimizer does) for a
    model whose item table is a lazy ``HipEmbedding``: every other parameter is stepped by ``torch.optim.<name>(lr,
    weight_decay=l2)``, the table by ``hip_ops.RowLazyTable`` — row by row, exactly as dense Adam / SGD would advance it, from
    the (idx, grad_out) pairs the lookups' backward recorded, in the order of the forward lookups."""

    @staticmethod
    def supports(name):
        return name in ("SGD", "Adam")

    def __init__(self, model, emb, name, lr, l2, max_lag=None):
        if not self.supports(name):
            raise ValueError("RowLazyOptimizer supports SGD and Adam, got %r" % (name,))
        self.emb, self.name, self.lr, self.l2, self.max_lag = emb, name, float(lr), float(l2), max_lag
        others = [p for p in model.parameters() if p is not emb.weight]
        self.inner = getattr(torch.optim, name)(others, lr=self.lr, weight_decay=self.l2)
        self._table = None
        emb.bind_lazy(self)

    param_groups = property(lambda self: self.inner.param_groups)

    def table(self):
        """the RowLazyTable of the weight's present storage (models are built on the host and moved afterwards)"""
        w = self.emb.weight.data
        if self._table is None or self._table.w.data_ptr() != w.data_ptr():
            if self._table is not None and self._table.t > 0:
                raise RuntimeError("the embedding table was re-allocated after optimizer steps had been taken")
            self._table = hip_ops.RowLazyTable(w, self.name, self.lr, self.l2, max_lag=self.max_lag,
                                               padding_idx=self.emb.padding_idx)
        return self._table

    def zero_grad(self, set_to_none=True):
        self.inner.zero_grad(set_to_none=set_to_none)
        self.emb._pending.clear()
        self.emb._lookups = 0

    @torch.no_grad()
    def step(self):
        pending = sorted(self.emb._pending, key=lambda e: e[0])
        if not pending:
            raise RuntimeError("optimizer.step() without a preceding training predict() / backward(): no lookup of the lazy "
                               "table recorded a gradient")
        self.table().step([e[1] for e in pending], [e[2] for e in pending], check=False)
        self.inner.step()
        self.emb._pending.clear()
        self.emb._lookups = 0

    def flush(self):
        """every row of the table up to the current step; called by the model before anything but a training step reads it"""
        if self._table is not None:
            self._table.flush()


class EmbLazyMixin:
    """``--emb_lazy`` for a model whose item table is a ``HipEmbedding``: the flag, the pre-installed optimizer (the runners
    build one only while ``model.optimizer`` is None, as for BPRMF) and the flushes before anything but a training step reads
    the table (the pattern of bprmf.BPRMF._sync_tables).  With the flag off every method here falls through."""

    @staticmethod
    def add_emb_lazy_arg(parser):
        parser.add_argument("--emb_lazy", type=int, default=0, choices=[0, 1],
                            help="1: the item table gets no dense gradient; its Adam / SGD state is advanced row by row, exactly "
                                 "as the dense optimizer would (other parameters keep torch.optim).  0: dense gradient + torch.optim.")

    def _install_emb_lazy(self, args, emb, blocked=None):
        """blocked: why this configuration cannot take the lazy table (logged once), or None"""
        self.emb_lazy = False
        if not int(getattr(args, "emb_lazy", 0)):
            return
        name = getattr(args, "optimizer", None)
        if blocked is None and not (RowLazyOptimizer.supports(name) and hasattr(args, "lr")):
            blocked = "--optimizer %s is not SGD or Adam" % (name,)
        if blocked is not None:
            logging.warning("--emb_lazy 1: %s; keeping the dense gradient and torch.optim", blocked)
            return
        self.optimizer = RowLazyOptimizer(self, emb, name, args.lr, getattr(args, "l2", 0.0))
        self.emb_lazy = True

    def _sync_tables(self):
        """lazy rows -> current (a no-op otherwise); every reader of the item table outside a training step calls it"""
        opt = getattr(self, "optimizer", None)
        if isinstance(opt, RowLazyOptimizer):
            opt.flush()

    def train(self, mode=True):
        if not mode:
            self._sync_tables()           # model.eval() precedes every evaluation
        return super().train(mode)

    def state_dict(self, *a, **kw):
        self._sync_tables()
        return super().state_dict(*a, **kw)

    def load_state_dict(self, *a, **kw):
        self._sync_tables()               # pending replays belong to the old weights
        return super().load_state_dict(*a, **kw)


class _Attention(nn.Module):
    """Multi-head self-attention of layers.py:8-57: separate q/k/v projections, no output projection, scores shifted by
    their GLOBAL maximum before the softmax (:54), NaN rows zeroed (:55)."""

    def __init__(self, d_model, n_heads):
        super().__init__()
        self.h, self.d_k = n_heads, d_model // n_heads
        self.q_linear = nn.Linear(d_model, d_model)
        self.k_linear = nn.Linear(d_model, d_model)
        self.v_linear = nn.Linear(d_model, d_model)

    def _split(self, x):
        return x.view(*x.shape[:-1], self.h, self.d_k).transpose(-2, -3)

    def forward(self, x, mask):
        q, k, v = self._split(self.q_linear(x)), self._split(self.k_linear(x)), self._split(self.v_linear(x))
        s = torch.matmul(q, k.transpose(-2, -1)) / self.d_k ** 0.5
        s = s.masked_fill(mask == 0, -np.inf)
        s = (s - s.max()).softmax(dim=-1)
        s = s.masked_fill(torch.isnan(s), 0)
        return torch.matmul(s, v).transpose(-2, -3).reshape(x.shape)


class _Block(nn.Module):
    """layers.py:60-86: post-norm residual attention + 2-layer ReLU feed-forward."""

    def __init__(self, d_model, d_ff, n_heads, dropout):
        super().__init__()
        self.masked_attn_head = _Attention(d_model, n_heads)
        self.layer_norm1 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)
        self.linear1 = nn.Linear(d_model, d_ff)
        self.linear2 = nn.Linear(d_ff, d_model)
        self.layer_norm2 = nn.LayerNorm(d_model)
        self.dropout2 = nn.Dropout(dropout)

    def forward(self, seq, mask):
        ctx = self.layer_norm1(self.dropout1(self.masked_attn_head(seq, mask)) + seq)
        out = self.linear2(self.linear1(ctx).relu())
        return self.layer_norm2(self.dropout2(out) + ctx)


def _xavier_normal_all(module):
    """reference src/models/init.py:13-29 applied through nn.Module.apply"""
    if isinstance(module, (nn.Embedding, HipEmbedding)):
        nn.init.xavier_normal_(module.weight.data)
    elif isinstance(module, nn.Linear):
        nn.init.xavier_normal_(module.weight.data)
        if module.bias is not None:
            nn.init.constant_(module.bias.data, 0)


def make_sasrec(sequential_model_cls):
    class SASRec(EmbLazyMixin, SoftmaxLossMixin, sequential_model_cls):
        reader = "SeqReader"
        runner = "BaseRunner"
        extra_log_args = ["emb_size", "num_layers", "num_heads", "train_loss", "softmax_native"]

        @staticmethod
        def parse_model_args(parser):
            parser.add_argument("--emb_size", type=int, default=64, help="Size of embedding vectors.")
            parser.add_argument("--num_layers", type=int, default=1, help="Number of self-attention layers.")
            parser.add_argument("--num_heads", type=int, default=4, help="Number of attention heads.")
            parser.add_argument("--dropout", type=float, default=0.1, help="Dropout probability.")
            parser.add_argument("--block_native", type=int, default=0, choices=[0, 1],
                                help="1: each transformer block by the fused HIP kernels (forward and backward); 0: torch ops + autograd.")
            EmbLazyMixin.add_emb_lazy_arg(parser)
            SoftmaxLossMixin.add_softmax_loss_args(parser)
            return sequential_model_cls.parse_model_args(parser)

        def __init__(self, args, corpus):
            super().__init__(args, corpus)
            self.emb_size, self.max_his = args.emb_size, args.history_max
            self.item_embedding = HipEmbedding(self.item_num, self.emb_size, padding_idx=0)
            self.position_embedding = nn.Embedding(self.max_his + 1, self.emb_size)
            self.transformer_block = nn.ModuleList([_Block(self.emb_size, self.emb_size, args.num_heads, args.dropout)
                                                    for _ in range(args.num_layers)])
            self.apply(_xavier_normal_all)
            self.num_heads, self.dropout = int(args.num_heads), float(args.dropout)
            self.block_native = bool(int(getattr(args, "block_native", 0)))
            self._block_native_ok = {}   # per history length, decided at its first batch: the library says what it takes
            self._block_seed = int(getattr(args, "random_seed", 0)) * 0x9E3779B97F4A7C15
            self._block_calls = 0        # one dropout stream per training step and layer
            self._install_softmax_loss(args)
            self._install_emb_lazy(args, self.item_embedding)

        def _use_block_native(self, T):
            if not self.block_native:
                return False
            if T not in self._block_native_ok:
                ok = hip_ops.sasblock_supports(self.emb_size, self.emb_size, self.num_heads, T)
                if not ok and not any(v is False for v in self._block_native_ok.values()):
                    logging.warning("--block_native 1: the block kernels do not take emb_size=%d num_heads=%d history=%d; keeping "
                                    "the torch path", self.emb_size, self.num_heads, T)
                self._block_native_ok[T] = ok
            return self._block_native_ok[T]

        def forward(self, feed_dict):
            history, lengths = feed_dict["history_items"], feed_dict["lengths"]
            bsz, T = history.shape
            valid = (history > 0).float()
            pos_ids = torch.arange(T, device=history.device).unsqueeze(0).expand_as(history)
            x = self.item_embedding(history) + self.position_embedding(pos_ids)        # SASRec.py:79-85
            mask = torch.tril(torch.ones(1, 1, T, T, dtype=torch.int32, device=history.device))
            if self._use_block_native(T):
                for blk in self.transformer_block:
                    x = hip_ops.sasrec_block(x, blk, self.num_heads, self.dropout, self._block_seed + self._block_calls, self.training)
                    self._block_calls += int(self.training)
            else:
                for blk in self.transformer_block:
                    x = blk(x, mask)
            x = x * valid[:, :, None]
            return x[torch.arange(bsz, device=history.device), lengths - 1, :]          # last valid position (:95)

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

        # The query protocol of HipRunner's device evaluation (--seq_eval_native 1) and recommend_rows: a model whose score
        # of row e against item j is <eval_queries(...)[e], eval_items()[j]>.
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
            """[n_items, D] item side of the scores: full_predict's second operand"""
            self._sync_tables()
            return self.item_embedding.weight

    SASRec.__qualname__ = "SASRec"
    return SASRec


SASRec = make_sasrec(host.SequentialModel)


def bind(reference_sequential_model_cls):
    return make_sasrec(reference_sequential_model_cls)
