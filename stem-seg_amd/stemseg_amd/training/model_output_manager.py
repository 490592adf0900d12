"""``ModelOutputManager(division_factor)``, the reference's class of that name (training/model_output_manager.py): with gradient
accumulation an optimiser step is fed by ``division_factor`` sub-iterations, so each one back-propagates its summed optimisation losses
divided by that factor, and the values that get logged are averaged over the sub-iterations in the same way."""
import torch

from ..utils.constants import ModelOutput


class ModelOutputManager(object):
    def __init__(self, division_factor, excluded_keys=()):
        self.division_factor = float(division_factor)
        self.excluded_keys = tuple(excluded_keys)
        self.tensor_vars, self.other_vars = {}, {}           # running means since the last reset: tensors (detached) / plain numbers

    def _add(self, values):
        for key, value in values.items():
            if key in self.excluded_keys:
                continue
            if torch.is_tensor(value):
                share, sums = value.detach() / self.division_factor, self.tensor_vars
            else:
                share, sums = value / self.division_factor, self.other_vars
            sums[key] = sums[key] + share if key in sums else share

    def __call__(self, model_output):
        """-> the loss to call ``backward()`` on; the output's losses and its 'others' entries join the running means."""
        losses = model_output[ModelOutput.OPTIMIZATION_LOSSES]
        self._add(losses)
        self._add(model_output[ModelOutput.OTHERS])
        return sum(losses.values()) / self.division_factor

    def reset(self):
        """-> (tensor means, other means) gathered since the last call, and start over."""
        gathered = self.tensor_vars, self.other_vars
        self.tensor_vars, self.other_vars = {}, {}
        return gathered
