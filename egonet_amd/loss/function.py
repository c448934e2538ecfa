"""Criteria of the angle-regression baselines with the reference's names and signatures
(``libs/loss/function.py:204-228``): ``MSELoss1D`` and ``SmoothL1Loss1D``, torch's ``nn.MSELoss`` / ``nn.SmoothL1Loss``
on the ``[N, 2]`` prediction and target; the target weight and the meta dictionary of the trainer's call are accepted
and unused, like there.

``trainer.make_step`` reads the class NAME of such an object and configures the native step
(``HRNetTrainStep(angle_type='mse' | 'sl1')``: loss and gradient seed in one HIP launch); the object itself is called
only where a torch tensor is wanted -- ``trainer.evaluate(loss_func=...)``'s validation loss, or the autograd bridge's
``loss = criterion(model(x), target)``.
"""
import torch.nn as nn


class MSELoss1D(nn.Module):
    def __init__(self, use_target_weight=False, reduction='mean'):
        super().__init__()
        self.use_target_weight = use_target_weight
        self.criterion = nn.MSELoss(reduction=reduction)

    def forward(self, output, target, target_weight=None, meta=None):
        return self.criterion(output, target)


class SmoothL1Loss1D(nn.Module):
    def __init__(self, use_target_weight=False):
        super().__init__()
        self.use_target_weight = use_target_weight
        self.criterion = nn.SmoothL1Loss(reduction='mean')

    def forward(self, output, target, target_weight=None, meta=None):
        return self.criterion(output, target)
