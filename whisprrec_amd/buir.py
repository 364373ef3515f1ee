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

Evaluation: ``full_predict``'s score u.P(i) + P(u).i is the inner product of [u, P(u)] and [P(i), i], so ``eval_factors()``
hands ``HipRunner.evaluate`` / ``recommend`` / ``--save_rec`` two matrices of width 2 D.  At D = 128 that width (256) is past
what the ranking kernels take: ``evaluate`` falls back to the host loop there and ``recommend`` raises NotImplementedError.
"""
import logging

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import hip_ops, host


def make_buir(general_model_cls):
    class BUIR(general_model_cls):
        reader = "BaseReader"
        runner = "BaseRunner"
        extra_log_args = ["embedding_size", "momentum"]

        @staticmethod
        def parse_model_args(parser):
            parser.add_argument("--embedding_size", type=int, default=64, help="Size of embedding vectors.")
            parser.add_argument("--momentum", type=float, default=0.995, help="Momentum update.")
            parser.add_argument("--buir_native", type=int, default=0, choices=[0, 1],
                                help="1: the loss, its gradients and the target update by the fused HIP kernels; 0: torch ops.")
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
            if opt is not None:
                self.__dict__["_optimizer_hook"] = opt.register_step_post_hook(lambda *_: self._update_target())

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
            return super().train(mode)

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
            user_e = self.user_online(feed_dict["user_id"])
            all_item_e = self.item_online.weight
            user_predictor = self.predictor(user_e)
            item_weights = self.predictor(self.item_online.weight).transpose(0, 1)
            return torch.matmul(user_e, item_weights) + torch.matmul(user_predictor, all_item_e.transpose(0, 1))

        @torch.no_grad()
        def eval_factors(self):
            """(user matrix, item matrix), both of width 2 D, whose inner products are full_predict's scores:
            u.P(i) + P(u).i = [u, P(u)] . [P(i), i]"""
            U, I = self.user_online.weight, self.item_online.weight
            return (torch.cat([U, self.predictor(U)], dim=1).contiguous(), torch.cat([self.predictor(I), I], dim=1).contiguous())

    BUIR.__qualname__ = "BUIR"
    return BUIR


BUIR = make_buir(host.GeneralModel)


def bind(reference_general_model_cls):
    """``BUIRHip = bind(GeneralModel)`` inside the reference tree."""
    return make_buir(reference_general_model_cls)
