"""``get_dataset(settings)`` as the reference's starcop/dataset_setup.py: the Permian 2019 data module over resident tiles."""
from .datamodule import Permian2019DataModule


def get_dataset(settings):
    return Permian2019DataModule(settings)
