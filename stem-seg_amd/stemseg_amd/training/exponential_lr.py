"""``ExponentialLR(optimizer, decay_factor, decay_steps, start_at=0)``, the reference's scheduler of that name (training/exponential_lr.py).

The rate stays at its base value for the first ``start_at`` scheduler steps and is then multiplied by one constant per step, chosen so
that ``decay_steps`` steps later it has fallen by ``decay_factor``.  After k scheduler steps: ``base_lr * decay_factor ** (max(0, k -
start_at + 1) / decay_steps)``."""
from torch.optim.lr_scheduler import LRScheduler


class ExponentialLR(LRScheduler):
    def __init__(self, optimizer, decay_factor, decay_steps, start_at=0, last_epoch=-1):
        if not decay_steps > 0:
            raise ValueError("ExponentialLR: decay_steps %r must be positive" % (decay_steps,))
        if not 0.0 < decay_factor < 1.0:
            raise ValueError("ExponentialLR: decay_factor %r must lie in (0, 1)" % (decay_factor,))
        self.gamma = float(decay_factor) ** (1.0 / decay_steps)       # the per-step multiplier
        self.start_at = int(start_at)
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        current = [group["lr"] for group in self.optimizer.param_groups]
        return current if self.last_epoch < self.start_at else [lr * self.gamma for lr in current]
