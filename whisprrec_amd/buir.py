"""BUIR (reference src/models/general/BUIR.py): bootstrapping user and item representations from positive pairs alone.  Two
online tables and a shared linear predictor are trained to predict the OTHER side's target row; the target tables follow the
online ones by a momentum update after every optimizer step.

The reference's own glue is stale (its ``__init__(corpus, configs)`` and ``BUIRRunner`` no longer fit its launcher), so this is
the model behind the ``(args, corpus)`` / ``BaseRunner`` surface every other model here uses; the formulas are BUIR.py:69-110.

Parameter names are the reference's, so checkpoints interchange: ``user_online.weight``, ``user_target.weight``,
``item_online.weight``, ``item_target.weight``, ``predictor.weight``, ``predictor.bias``.  Initialisation: ``_init_weights``
(:35-42) in ``self.modules()`` order — xavier_normal_ on every embedding and on the linear weight, normal_ (std 1) on the linear
bias — then the targets are copied from the online tables and frozen (:61-66); the same torch seed gives the same bits.

The target update needs no runner of its own: ``optimizer`` is a property, and assigning an optimizer registers a step post hook
that calls ``_update_target()``.  BUIR therefore trains under ``BaseRunner.fit``, ``HipRunner.fit`` and the reference's
``BaseRunner`` alike.

``--buir_native 1`` (off by default): ``predict`` goes through ``hip_ops.buir_loss`` (wr_buir_loss_grad, K16: the loss and every
gradient in one call) and ``_update_target`` through ``hip_ops.ema_update_`` (wr_ema_update, K17: one pass per table).  An
embedding size the kernel does not take is logged once and keeps the torch path.  With the flag off the model is stock torch
ops and runs on the CPU too.

``--emb_lazy 1`` (with ``--buir_native 1``, Adam or SGD; off by default): the four tables get no dense gradient and no table
pass.  ``predict`` gathers the batch's online and target rows as of the current step (``hip_ops.RowLazyEmaTable.gather``), hands
those four ``[B, D]`` arrays to the same loss kernel with ``arange(B)`` as the ids, and records the per-sample gradient rows;
``BuirLazyOptimizer.step`` advances each (online, target) pair row by row — optimizer step, then the momentum update — exactly as
the dense optimizer followed by ``_update_target`` would (K24), and leaves the predictor to ``torch.optim``.  ``_sync_tables``
flushes before anything but a training step reads a table.  Any other configuration logs one line and keeps the dense path.

Evaluation: ``full_predict``'s score u.P(i) + P(u).i is the inner product of [u, P(u)] and [P(i), i], so ``eval_factors()``
hands ``HipRunner.evaluate`` / ``recommend`` / ``--save_rec`` two matrices of width 2 D.  At D = 128 that width (256) is past
what the ranking kernels take: ``evaluate`` falls back to the host loop there and ``recommend`` raises NotImplementedError.
"""
import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip_ops, host
from .sasrec import EmbLazyMixin


class _BuirLazyLoss(torch.autograd.Function):
    """the bootstrap loss on the gathered rows of the lazy tables: wr_buir_loss_grad reads four [B, D] arrays at arange(B) (the
    bits it produces from the flushed tables at the real ids); the backward records the per-sample gradient rows for
    BuirLazyOptimizer.step and hands the predictor its gradients.  `marker`: a scalar that requires grad stands in for the
    tables, which must not be handed a dense gradient (sasrec.HipEmbedding's trick)."""

    @staticmethod
    def forward(ctx, marker, W, b, model, users, items):
        opt = model.optimizer
        ut, it = opt.tables()
        uo, utg = ut.gather(users, check=False)
        io, itg = it.gather(items, check=False)
        pos = model._batch_positions(users.numel(), W.device)
        loss, gU, gI, gW, gb = hip_ops.buir_loss_grad(uo, io, utg, itg, W.detach(), b.detach(), pos, pos)
        ctx.save_for_backward(gU, gI, gW, gb, users, items)
        ctx.model = model
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        gU, gI, gW, gb, users, items = ctx.saved_tensors
        ctx.model._pending = (users, gU * grad_out, items, gI * grad_out)
        return None, gW * grad_out, gb * grad_out, None, None, None


class BuirLazyOptimizer:
    """Duck-types what the runners need from ``model.optimizer`` (``zero_grad`` / ``step`` / ``param_groups``, as
    sasrec.RowLazyOptimizer does) for BUIR under ``--emb_lazy 1``: the two (online, target) pairs are stepped by
    ``hip_ops.RowLazyEmaTable`` from the rows the loss recorded — the target update is part of that step —, the predictor by
    ``torch.optim.<name>(lr, weight_decay=l2)``."""

    supports = staticmethod(lambda name: name in ("SGD", "Adam"))

    def __init__(self, model, name, lr, l2, max_lag=None):
        if not self.supports(name):
            raise ValueError("BuirLazyOptimizer supports SGD and Adam, got %r" % (name,))
        self.model, self.name, self.lr, self.l2, self.max_lag = model, name, float(lr), float(l2), max_lag
        self.inner = getattr(torch.optim, name)(list(model.predictor.parameters()), lr=self.lr, weight_decay=self.l2)
        self._tables = None

    param_groups = property(lambda self: self.inner.param_groups)

    def tables(self):
        """(user pair, item pair) as RowLazyEmaTables of the weights' present storage (models are built on the host and moved)"""
        m = self.model
        pairs = ((m.user_online.weight.data, m.user_target.weight.data), (m.item_online.weight.data, m.item_target.weight.data))
        if self._tables is None or any(t.w.data_ptr() != w.data_ptr() or t.tgt.data_ptr() != g.data_ptr()
                                       for t, (w, g) in zip(self._tables, pairs)):
            if self._tables is not None and any(t.t > 0 for t in self._tables):
                raise RuntimeError("a BUIR table was re-allocated after optimizer steps had been taken")
            self._tables = tuple(hip_ops.RowLazyEmaTable(w, g, self.name, self.lr, self.l2, m.momentum, max_lag=self.max_lag)
                                 for w, g in pairs)
        return self._tables

    def zero_grad(self, set_to_none=True):
        self.inner.zero_grad(set_to_none=set_to_none)
        self.model._pending = None

    @torch.no_grad()
    def step(self):
        pending = self.model._pending
        if pending is None:
            raise RuntimeError("optimizer.step() without a preceding training predict() / backward(): the loss recorded no "
                               "gradient rows for the lazy tables")
        users, gU, items, gI = pending
        ut, it = self.tables()
        ut.step([users], [gU], check=False)
        it.step([items], [gI], check=False)
        self.inner.step()
        self.model._pending = None

    def flush(self):
        """every row of the four tables up to the current step (and the findings of the unchecked training steps)"""
        if self._tables is not None:
            for t in self._tables:
                t.flush()


def make_buir(general_model_cls):
    class BUIR(EmbLazyMixin, general_model_cls):
        reader = "BaseReader"
        runner = "BaseRunner"
        extra_log_args = ["embedding_size", "momentum"]

        @staticmethod
        def parse_model_args(parser):
            parser.add_argument("--embedding_size", type=int, default=64, help="Size of embedding vectors.")
            parser.add_argument("--momentum", type=float, default=0.995, help="Momentum update.")
            parser.add_argument("--buir_native", type=int, default=0, choices=[0, 1],
                                help="1: the loss, its gradients and the target update by the fused HIP kernels; 0: torch ops.")
            EmbLazyMixin.add_emb_lazy_arg(parser)
            return general_model_cls.parse_model_args(parser)

        def __init__(self, args, corpus):
            super().__init__(args, corpus)
            self.embedding_size = args.embedding_size
            self.momentum = args.momentum
            self.user_num, self.item_num = int(corpus.n_users), int(corpus.n_items)
            self.user_online = nn.Embedding(self.user_num, self.embedding_size)
            self.user_target = nn.Embedding(self.user_num, self.embedding_size)
            self.item_online = nn.Embedding(self.item_num, self.embedding_size)
            self.item_target = nn.Embedding(self.item_num, self.embedding_size)
            self.predictor = nn.Linear(self.embedding_size, self.embedding_size)
            self._init_weights()
            for online, target in ((self.user_online, self.user_target), (self.item_online, self.item_target)):
                for param_o, param_t in zip(online.parameters(), target.parameters()):
                    param_t.data.copy_(param_o.data)
                    param_t.requires_grad = False
            self.buir_native = bool(int(getattr(args, "buir_native", 0)))
            self._buir_native_ok = None      # decided at the first batch: the library says what it takes
            self._id_err = None              # device error word of the ids, read by check_ids()
            self._pending = None             # (users, gU, items, gI) of the step, recorded by the lazy loss's backward
            self._positions = None           # cached arange(B): the ids of the gathered rows
            self._marker = None              # the scalar that requires grad in the tables' place
            self._install_buir_lazy(args)

        def _init_weights(self):
            for m in self.modules():
                if isinstance(m, nn.Linear):
                    nn.init.xavier_normal_(m.weight.data)
                    nn.init.normal_(m.bias.data)
                if isinstance(m, nn.Embedding):
                    nn.init.xavier_normal_(m.weight.data)

        # ------------------------------------------------------------------------------------ the optimizer hook
        @property
        def optimizer(self):
            return self.__dict__.get("_optimizer")

        @optimizer.setter
        def optimizer(self, opt):
            handle = self.__dict__.pop("_optimizer_hook", None)
            if handle is not None:
                handle.remove()
            self.__dict__["_optimizer"] = opt
            # a BuirLazyOptimizer updates the targets inside its table step and has no hooks
            if opt is not None and hasattr(opt, "register_step_post_hook"):
                self.__dict__["_optimizer_hook"] = opt.register_step_post_hook(lambda *_: self._update_target())

        # ------------------------------------------------------------------------------------ --emb_lazy
        def _install_buir_lazy(self, args):
            self.emb_lazy = False
            if not int(getattr(args, "emb_lazy", 0)):
                return
            name = getattr(args, "optimizer", None)
            blocked = None
            if not self.buir_native:
                blocked = "it needs --buir_native 1"
            elif not (BuirLazyOptimizer.supports(name) and hasattr(args, "lr")):
                blocked = "--optimizer %s is not SGD or Adam" % (name,)
            elif not hip_ops.buir_supports(self.embedding_size):
                blocked = "the loss kernel does not take embedding_size=%d" % self.embedding_size
                self._buir_native_ok = False          # said here: _use_native does not log it a second time
            if blocked is not None:
                logging.warning("--emb_lazy 1: %s; keeping the dense gradient and torch.optim", blocked)
                return
            self.optimizer = BuirLazyOptimizer(self, name, args.lr, getattr(args, "l2", 0.0))
            self.emb_lazy = True

        def _sync_tables(self):
            """lazy rows -> current (a no-op otherwise); every reader of a table outside a training step calls it"""
            opt = self.optimizer
            if isinstance(opt, BuirLazyOptimizer):
                opt.flush()

        def _batch_positions(self, B, dev):
            if self._positions is None or self._positions.numel() < B or self._positions.device != dev:
                self._positions = torch.arange(B, dtype=torch.int64, device=dev)
            return self._positions[:B]

        # ------------------------------------------------------------------------------------ native path
        def _use_native(self):
            if not self.buir_native:
                return False
            if self._buir_native_ok is None:
                self._buir_native_ok = hip_ops.buir_supports(self.embedding_size)
                if not self._buir_native_ok:
                    logging.warning("--buir_native 1: the kernels do not take embedding_size=%d; keeping the torch path",
                                    self.embedding_size)
            return self._buir_native_ok

        def check_ids(self):
            """raise if a fused loss call since the last check was handed an id outside its table (one read of the device word)"""
            if self._id_err is not None and int(self._id_err.item()) != 0:
                self._id_err.zero_()
                raise IndexError("BUIR: a user or item id outside its table reached the loss kernel")

        def train(self, mode=True):
            if not mode:
                self.check_ids()             # model.eval() precedes every evaluation: once per epoch
            return super().train(mode)       # EmbLazyMixin.train flushes the lazy tables (ids outside a table raise there)

        # ------------------------------------------------------------------------------------ the reference's methods
        @torch.no_grad()
        def _update_target(self):
            native = self._use_native()
            for online, target in ((self.user_online, self.user_target), (self.item_online, self.item_target)):
                for param_o, param_t in zip(online.parameters(), target.parameters()):
                    if native:
                        hip_ops.ema_update_(param_t.data, param_o.data, self.momentum)
                    else:
                        param_t.data = param_t.data * self.momentum + param_o.data * (1. - self.momentum)

        def forward(self, feed_dict):
            user, item = feed_dict["user_id"], feed_dict["pos_item"]
            u_online = self.predictor(self.user_online(user))
            u_target = self.user_target(user)
            i_online = self.predictor(self.item_online(item))
            i_target = self.item_target(item)
            return u_online, u_target, i_online, i_target

        def predict(self, feed_dict):
            """the bootstrap loss of the batch; ``neg_items`` is not read (the dataset still samples it, as the reference's
            does, so NumPy's stream stays the reference's)"""
            if self.emb_lazy:
                dev = self.predictor.weight.device
                users, items = feed_dict["user_id"].to(dev).reshape(-1), feed_dict["pos_item"].to(dev).reshape(-1)
                if self.training and torch.is_grad_enabled():
                    if self._marker is None or self._marker.device != dev:
                        self._marker = torch.zeros((), device=dev, requires_grad=True)
                    return _BuirLazyLoss.apply(self._marker, self.predictor.weight, self.predictor.bias, self, users, items)
                self._sync_tables()          # no step follows: the flushed tables through the ordinary call
            if self._use_native():
                dev = self.predictor.weight.device
                if self._id_err is None:
                    self._id_err = torch.zeros(1, dtype=torch.int32, device=dev)
                return hip_ops.buir_loss(self.user_online.weight, self.item_online.weight, self.user_target.weight,
                                         self.item_target.weight, self.predictor.weight, self.predictor.bias,
                                         feed_dict["user_id"].to(dev).reshape(-1), feed_dict["pos_item"].to(dev).reshape(-1),
                                         err_word=self._id_err)
            u_online, u_target, i_online, i_target = self.forward(feed_dict)
            u_online = F.normalize(u_online, dim=-1)
            u_target = F.normalize(u_target, dim=-1)
            i_online = F.normalize(i_online, dim=-1)
            i_target = F.normalize(i_target, dim=-1)
            loss_ui = 2 - 2 * (u_online * i_target.detach()).sum(dim=-1)
            loss_iu = 2 - 2 * (i_online * u_target.detach()).sum(dim=-1)
            return (loss_ui + loss_iu).mean()

        def full_predict(self, feed_dict):
            self._sync_tables()
            user_e = self.user_online(feed_dict["user_id"])
            all_item_e = self.item_online.weight
            user_predictor = self.predictor(user_e)
            item_weights = self.predictor(self.item_online.weight).transpose(0, 1)
            return torch.matmul(user_e, item_weights) + torch.matmul(user_predictor, all_item_e.transpose(0, 1))

        @torch.no_grad()
        def eval_factors(self):
            """(user matrix, item matrix), both of width 2 D, whose inner products are full_predict's scores:
            u.P(i) + P(u).i = [u, P(u)] . [P(i), i]"""
            self._sync_tables()
            U, I = self.user_online.weight, self.item_online.weight
            return (torch.cat([U, self.predictor(U)], dim=1).contiguous(), torch.cat([self.predictor(I), I], dim=1).contiguous())

    BUIR.__qualname__ = "BUIR"
    return BUIR


BUIR = make_buir(host.GeneralModel)


def bind(reference_general_model_cls):
    """``BUIRHip = bind(GeneralModel)`` inside the reference tree."""
    return make_buir(reference_general_model_cls)
