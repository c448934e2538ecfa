"""What the precision = 'f16s2' network-level checks add to tests/f16_mode_case.py (same model, batches and quantities):
the bounds file of the mode and its CPU emulation.  Shared by tests/golden/make_f16s2_bounds.py,
tests/test_f16s2_mode_cpu.py and tests/test_gpu_f16s2_mode.py (imported, not a conftest)."""
import os

import torch
import torch.nn as nn

from f16_mode_case import (HEADS, SIZE, BATCHES, config, model, crops, quantities, deviations, cpu_f32)  # noqa: F401
from egonet_amd import engine

BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'f16s2_mode_bounds.json')


def cpu_emulated(net, x):
    """(quantities, convolutions rounded, of which stride 2) of the 'f16s2' emulation."""
    with torch.no_grad(), engine.f16_emulation(net, precision='f16s2') as em:
        out = net(x)
    return quantities(out), len(em.hit), sum(1 for m in em.hit if m.stride == (2, 2))


def seen_conv_inputs(net, x):
    """{module name: input shape} of every nn.Conv2d in a torch forward of ``net`` on ``x``."""
    seen = {}
    hooks = [m.register_forward_pre_hook(lambda mod, args, name=name: seen.__setitem__(name, tuple(args[0].shape)))
             for name, m in net.named_modules() if isinstance(m, nn.Conv2d)]
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()
    return seen
