"""``ModelModuleRegression``: the regression twin of :class:`starcop_amd.model_module.ModelModule`.

Mirrors starcop/models/model_module_regression.py member for member:
  ModelModuleRegression(settings) :16-55, training_step :57-73, forward :75-86, val_step :95-103, the empty epoch ends :115-123,
  configure_optimizers :125-138, batch_with_preds :144-161, configure_architecture :165-192, load_weights :194-202,
  differences :204-205.  ``inhibit_normalisation`` is True as there: forward and losses see the raw ``x`` / ``y``.

Underneath, ``cnn_v2`` / ``cnn_v3`` are :mod:`starcop_amd.pointwise_net` (HIP forward, moment-sweep backward), ``unet_semseg`` is
the HIP U-Net called without normaliser constants, the losses are ``sc_reg_loss`` and the optimiser is the fused Adam.
``fused_train_step`` is the whole step without an autograd graph: for the pointwise networks one sweep over ``x`` and ``y``, a
one-work-group finalize and Adam.  Gradient exchange across ranks and hipGraph capture of this step are out of scope: the step is
rank-local and allocates nothing after its first call, but neither has been wired up or tested.
"""
from typing import Dict

import torch
import torch.nn

from . import _lib
from ._lib import check, ptr, stream
from .model_module import HAVE_LIGHTNING, _Base, _multi_rank, load_weights  # noqa: F401  (load_weights is part of this module's surface)
from .network import HyperStarcopUNet
from .normalizer import DataNormalizer
from .optim import FusedAdam
from .pointwise_net import SimpleCNN_v2, SimpleCNN_v3, _PointwiseNet

_KIND = {"l1": _lib.REG_L1, "mse": _lib.REG_MSE}


def reg_loss_sum(pred, target, kind, dpred=None):
    """``sc_reg_loss``: float64 device scalar sum |pred - y| (``l1``) or sum (pred - y)^2 (``mse``); ``dpred`` (optional, same shape)
    receives the gradient of the MEAN.  Both tensors must be dense fp32 device tensors of one shape."""
    _lib.require_device(pred)
    _lib.require_device(target)
    if pred.shape != target.shape:
        raise ValueError(f"prediction {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    lib = _lib.load()
    acc = torch.empty(1, dtype=torch.float64, device=pred.device)
    work = torch.empty(_lib.REG_LOSS_PARTS, dtype=torch.float64, device=pred.device)
    check(lib.sc_reg_loss(ptr(pred), ptr(target), pred.numel(), _KIND[kind], ptr(acc), ptr(dpred), ptr(work), stream()))
    return acc


class _RegLossFunction(torch.autograd.Function):
    """mean |pred - y| or mean (pred - y)^2 and its gradient w.r.t. pred in one HIP pass."""

    @staticmethod
    def forward(ctx, pred, target, kind):
        p = pred.contiguous().float()
        t = target.contiguous().float()
        d = torch.empty_like(p)
        acc = reg_loss_sum(p, t, kind, d)
        ctx.save_for_backward(d)
        return (acc / p.numel()).float().reshape(())

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return d * g, None, None


def l1(input, target):
    """``F.l1_loss(input, target)`` (models/utils/losses.py:3-4)."""
    return _RegLossFunction.apply(input, target, "l1")


def mse(input, target):
    """``F.mse_loss(input, target)`` (models/utils/losses.py:6-7)."""
    return _RegLossFunction.apply(input, target, "mse")


def differences(y_pred: torch.Tensor, y_gt: torch.Tensor) -> torch.Tensor:
    return y_pred - y_gt


def configure_architecture(architecture, num_channels, num_classes, extra_settings_model):
    if architecture == "unet_semseg":
        backbone = extra_settings_model.semseg_backbone
        if backbone != "mobilenet_v2":
            raise Exception(f"No HIP model implemented for semseg_backbone: {backbone}")
        return HyperStarcopUNet(in_channels=num_channels, classes=num_classes)
    if architecture == "cnn_v1":
        raise NotImplementedError("model_type 'cnn_v1' (SimpleCNN: 3x3 double convolutions, 64 and 128 channels wide) has no HIP "
                                  "implementation; the regression path serves cnn_v2, cnn_v3 and unet_semseg")
    if architecture == "cnn_v2":
        return SimpleCNN_v2(num_channels, num_classes)
    if architecture == "cnn_v3":
        return SimpleCNN_v3(num_channels, num_classes)
    raise Exception(f"No model implemented for model_type: {architecture}")


class ModelModuleRegression(_Base):

    def __init__(self, settings):
        super().__init__()
        if HAVE_LIGHTNING:
            self.save_hyperparameters()
        self.settings_model = settings.model
        self.settings_wandb = settings.wandb if "wandb" in settings else None
        self.normalizer = DataNormalizer(settings)
        self.num_classes = self.settings_model.num_classes
        self.num_channels = len(settings.dataset.input_products)
        architecture = self.settings_model.model_type
        self.network = configure_architecture(architecture, self.num_channels, self.num_classes, self.settings_model)
        self.lr = self.settings_model.lr
        self.lr_decay = self.settings_model.lr_decay
        self.lr_patience = self.settings_model.lr_patience
        self.loss_name = self.settings_model.loss
        if self.settings_model.loss == "l1":
            self.loss_function = l1
            self.loss_name = "l1_loss"
        elif self.settings_model.loss == "mse":
            self.loss_function = mse
            self.loss_name = "mse_loss"
        assert self.settings_model.model_mode == "regression_output", "this model module should be only used with regression!"
        self.inhibit_normalisation = True
        self._logged = {}
        self._optimizer = None
        self._loss_acc = None

    # -- Lightning shims when Lightning is absent (as ModelModule) --------------------------------
    if not HAVE_LIGHTNING:
        @property
        def device(self):
            return next(self.parameters()).device

        @classmethod
        def load_from_checkpoint(cls, checkpoint_path, settings=None, map_location="cpu", strict=True, **kw):
            ckpt = torch.load(checkpoint_path, map_location=map_location, weights_only=False)
            model = cls(settings)
            model.load_state_dict(ckpt["state_dict"] if "state_dict" in ckpt else ckpt, strict=strict)
            return model

    def log(self, name, value=None, *args, **kwargs):
        try:
            if HAVE_LIGHTNING:
                super().log(name, value, *args, **kwargs)
            else:
                self._logged[name] = value
        except Exception as e:
            print(f"Bug logging {e}")

    # ---------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(B, num_channels, H, W) -> (B, num_classes, H, W) prediction of the network, on the raw input."""
        if not self.inhibit_normalisation:
            return self.network(self.normalizer.normalize_x(x))
        return self.network(x)

    def _target(self, y):
        return y if self.inhibit_normalisation else self.normalizer.normalize_y(y)

    def training_step(self, batch: Dict, batch_idx) -> torch.Tensor:
        x, y = batch["input"], batch["output"]
        predictions = self.forward(x)
        loss = self.loss_function(predictions, self._target(y))
        if (batch_idx % 100) == 0:
            self.log(f"train_{self.loss_name}", loss)
        return loss

    def val_step(self, batch, batch_idx: int, prefix: str = "val"):
        x, y = batch["input"], batch["output"]
        predictions = self.forward(x)
        loss = self.loss_function(predictions, self._target(y))
        self.log(f"{prefix}_loss", loss, on_epoch=True)

    def validation_step(self, batch, batch_idx: int):
        return self.val_step(batch, batch_idx, prefix="val")

    def test_step(self, batch, batch_idx: int):
        return self.val_step(batch, batch_idx, prefix="test")

    def val_epoch_end(self, outputs, prefix):
        outs = {}
        return outs

    def validation_epoch_end(self, outputs) -> None:
        self.val_epoch_end(outputs, prefix="val")

    def test_epoch_end(self, outputs) -> None:
        self.val_epoch_end(outputs, prefix="test")

    def configure_optimizers(self):
        if self.settings_model.optimizer == "adam":
            optimizer = FusedAdam(self.network, lr=self.lr)
        else:
            raise Exception(f"No optimizer implemented for : {self.settings_model.optimizer}")
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=self.lr_decay,
                                                               patience=self.lr_patience)
        return {"optimizer": optimizer, "lr_scheduler": scheduler, "monitor": "val_loss"}

    def debug(self):
        print("Model debug:")
        print(self)

    def batch_with_preds(self, batch):
        pred = self(batch["input"])
        batch = batch.copy()
        batch["input_norm"] = self.normalizer.normalize_x(batch["input"])
        batch["output_norm"] = self.normalizer.normalize_y(batch["output"])
        batch["prediction"] = pred
        batch["logits"] = pred      # no logits here
        if not self.inhibit_normalisation:
            batch["differences"] = differences(batch["prediction"], batch["output_norm"].float())
        else:
            batch["differences"] = differences(batch["prediction"], batch["output"].float())
        return batch

    # ---------------------------------------------------------------------------------------------
    def fused_train_step(self, batch, optimizer=None):
        """forward + loss + backward + Adam without an autograd graph; the same arithmetic as training_step -> backward ->
        optimizer.step.  Returns a one-element float64 device tensor with the SUM of the per-element losses (divide by
        ``self.loss_n`` for the mean).  Rank-local: no gradient exchange; not validated under hipGraph capture."""
        if self.settings_model.loss not in _KIND:
            raise NotImplementedError(f"loss {self.settings_model.loss!r}: the regression path trains with 'l1' or 'mse'")
        if optimizer is None:
            if self._optimizer is None:
                self._optimizer = self.configure_optimizers()["optimizer"]
            optimizer = self._optimizer
        net = self.network
        if not net.training:
            raise RuntimeError("fused_train_step needs the module in train() mode")
        x = batch["input"]
        y = self._target(batch["output"])
        _lib.require_device(x)
        _lib.require_device(y)
        y = y.contiguous().float()
        if self._loss_acc is None or self._loss_acc.device != x.device:
            self._loss_acc = torch.empty(1, dtype=torch.float64, device=x.device)
        kind = _KIND[self.settings_model.loss]
        if isinstance(net, _PointwiseNet):
            self.loss_n = net.sweep_gradients(x, y, kind, self._loss_acc)
        else:
            lib = _lib.load()
            plan = net._forward_impl(x if self.inhibit_normalisation else self.normalizer.normalize_x(x), None, True, True)
            logits = plan.buf["logits"]
            if logits.shape != y.shape:
                raise ValueError(f"prediction {tuple(logits.shape)} and target {tuple(y.shape)} differ in shape")
            if not hasattr(plan, "reg_work"):
                plan.reg_work = torch.empty(_lib.REG_LOSS_PARTS, dtype=torch.float64, device=x.device)
            check(lib.sc_reg_loss(ptr(logits), ptr(y), logits.numel(), kind, ptr(self._loss_acc), ptr(plan.dlogits),
                                  ptr(plan.reg_work), stream()))
            net._backward_impl(plan, plan.dlogits)
            self.loss_n = logits.numel()
        optimizer.step_flat(sync_ranks=not _multi_rank())
        return self._loss_acc
