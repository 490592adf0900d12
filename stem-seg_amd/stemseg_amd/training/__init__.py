"""Training on the device (the reference's ``stemseg/training``): the optimiser step and the gradient norm on csrc/optimizer.hip
(``optim``), the gradient bucket of data-parallel training (``optim.GradBucket``), the reference's helpers (``utils``, ``exponential_lr``, ``model_output_manager``) and its loop (``main.Trainer``)."""
from .exponential_lr import ExponentialLR
from .model_output_manager import ModelOutputManager
from .optim import DeviceAdam, DeviceSGD, GradBucket, grad_norm
from .utils import configure_trainable, create_lr_scheduler, create_optimizer, optimizer_step_interval, var_keys_to_str

__all__ = ["DeviceAdam", "DeviceSGD", "ExponentialLR", "GradBucket", "ModelOutputManager", "configure_trainable", "create_lr_scheduler", "create_optimizer",
           "grad_norm", "optimizer_step_interval", "var_keys_to_str"]
