"""losses/get_loss.py of the reference: the loss a config names."""
from .losses import BaseLoss, DefaultLoss


def get_loss(cfg, id):
    name = cfg.data.loss_name
    if name == "default":
        return DefaultLoss(cfg, id)
    if name == "base":
        return BaseLoss(cfg, id)
    raise NotImplementedError(name)
