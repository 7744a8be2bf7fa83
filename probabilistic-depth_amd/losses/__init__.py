"""Training losses with the interface of the reference's losses/ package: get_loss(cfg, id) -> BaseLoss | DefaultLoss.
The cross-entropy of every volume is one fused HIP call for the whole batch (ops.dpv_soft_ce, csrc/loss.hip)."""
from .get_loss import get_loss  # noqa: F401
