"""``ImageLogger`` (starcop/data/data_logger.py): at the end of every training / validation epoch, run one fixed batch of each
split through ``model.batch_with_preds`` and render its ``products_plot`` figure.

The reference moves the batch with its predictions to the host and builds a matplotlib figure there; here the figure is the
``plot.Panels`` of ``plot.render_batch``, drawn on the device.  ``on_split_epoch_end`` always returns ``{f"{split}_batch": Panels}``;
the hooks hand the figure's ``image`` array (as a ``wandb.Image`` where wandb is importable: a logger cannot serialise a ``Panels``)
to ``trainer.logger.experiment.log`` when the trainer has such a logger, and with ``folder`` the figure
is also written as ``<folder>/<split>_epoch<k>.png``.  A Lightning ``Callback`` when Lightning is importable, a plain class with
the same hooks otherwise.
"""
import importlib.util
import os
from typing import Dict, List, Optional

import torch

from . import plot as starcoplot
from .validation import to_device

try:
    from pytorch_lightning.callbacks import Callback
except ImportError:
    try:
        from lightning.pytorch.callbacks import Callback
    except ImportError:
        Callback = object


def _loggable(panels: starcoplot.Panels):
    """what an experiment logger can take: the (Hc, Wc, 3) uint8 image, as a wandb.Image where wandb is there"""
    if importlib.util.find_spec("wandb") is not None:
        import wandb
        return wandb.Image(panels.image)
    return panels.image


class ImageLogger(Callback):

    def __init__(self, batch_train: Dict[str, torch.Tensor], batch_test: Dict[str, torch.Tensor], input_products: List[str],
                 products_plot: List[str], folder: Optional[str] = None) -> None:
        super().__init__()
        self.batch_train = batch_train
        self.batch_test = batch_test
        self.input_products = input_products
        self.products_plot = products_plot
        self.folder = folder

    def _log(self, trainer, batch, model, data_split_name: str) -> Dict[str, starcoplot.Panels]:
        out = self.on_split_epoch_end(batch, model, data_split_name, epoch=getattr(trainer, "current_epoch", None))
        log = getattr(getattr(getattr(trainer, "logger", None), "experiment", None), "log", None)
        if log is not None:
            log({k: _loggable(p) for k, p in out.items()}, commit=False)
        return out

    def on_train_epoch_end(self, trainer, model, unused: Optional = None):
        return self._log(trainer, self.batch_train, model, "train")

    def on_validation_epoch_end(self, trainer, model):
        return self._log(trainer, self.batch_test, model, "val")

    def on_split_epoch_end(self, batch, model, data_split_name: str, epoch: Optional[int] = None) -> Dict[str, starcoplot.Panels]:
        with torch.no_grad():
            batch_device_with_preds = model.batch_with_preds(to_device(batch, model.device))
        panels = starcoplot.render_batch(batch_device_with_preds, self.input_products, self.products_plot)
        if self.folder is not None:
            os.makedirs(self.folder, exist_ok=True)
            panels.save(os.path.join(self.folder, f"{data_split_name}_epoch{0 if epoch is None else int(epoch)}.png"))
        return {f"{data_split_name}_batch": panels}
