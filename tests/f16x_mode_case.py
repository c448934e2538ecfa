"""The model, inputs and measured quantities of the precision = 'f16x' network-level checks: shared by
tests/golden/make_f16x_bounds.py (which writes tests/golden/f16x_mode_bounds.json on the CPU), tests/test_f16x_mode_cpu.py
and tests/test_gpu_f16x_mode.py (imported, not a conftest).

Model: HRNet with the W32 widths (32 / 64 / 128 / 256) on the Pedestrian input, 192 x 256 (W x H; maps 64 x 48, 32 x 24,
16 x 12, 8 x 6 as H x W), one module per stage, one block per branch, 5 joints; seeded weights and BatchNorm statistics as
tests/f16_mode_case.py.  The true Pedestrian size is needed: the coordinate head's final (map_h / 16, map_w / 16) kernel
gives a 1 x 1 output only from a 64 x 48 map.  Quantities as in tests/f16_mode_case.py, pixels of the 192 x 256 input:
  heatmap         the heat-maps, absolute
  softargmax_px   the soft-arg-max of the heat-maps in INPUT pixels (map pixels x 4)
  coords_px       the coordinate head's output x (192, 256), pixels ('coordinates' only)
"""
import os

import torch
import torch.nn as nn

from egonet_amd import configs, engine, synth
from egonet_amd.model.heatmapModel import hrnet

HEADS = ('heatmap', 'coordinates')
WIDTH, HEIGHT = 192, 256
BATCHES = {'forward': (2, 0), 'infer_crops': (3, 1)}          # name -> (crops, seed of synth_crops)
BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'f16x_mode_bounds.json')


def config(head):
    return configs.hrnet_config(32, (WIDTH, HEIGHT), 5, head, modules=(1, 1, 1), num_blocks=1, lifter_neurons=128)


def model(head, seed=11):
    net = hrnet.get_pose_net(config(head), is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=seed))
    return net.eval()


def crops(which):
    n, seed = BATCHES[which]
    return synth.synth_crops(n, 3, HEIGHT, WIDTH, seed=seed)


def soft_arg_max_px(maps):
    """[N,K,H,W] -> [N,K,2] (x, y) in input pixels, float64."""
    n, k, h, w = maps.shape
    p = torch.softmax(maps.double().reshape(n, k, h * w), dim=2).reshape(n, k, h, w)
    xs = (p.sum(2) * torch.arange(w, dtype=torch.float64)).sum(2)
    ys = (p.sum(3) * torch.arange(h, dtype=torch.float64)).sum(2)
    return torch.stack([xs * (float(WIDTH) / w), ys * (float(HEIGHT) / h)], dim=2)


def quantities(out):
    """What a forward returned (maps, or (maps, coords)) -> {name: float64 CPU tensor}."""
    maps, coords = (out[0], out[1]) if isinstance(out, tuple) else (out, None)
    maps = maps.detach().cpu()
    q = {'heatmap': maps.double(), 'softargmax_px': soft_arg_max_px(maps)}
    if coords is not None:
        q['coords_px'] = coords.detach().cpu().double() * torch.tensor([WIDTH, HEIGHT], dtype=torch.float64)
    return q


def deviations(q, q_ref):
    return {k: float((q[k] - q_ref[k]).abs().max()) for k in q_ref}


def cpu_f32(net, x):
    with torch.no_grad():
        return quantities(net(x))


def cpu_emulated(net, x):
    """(quantities, convolutions rounded, of which ``f16x_eligible``) of the 'f16x' emulation."""
    with torch.no_grad(), engine.f16_emulation(net, precision='f16x') as em:
        out = net(x)
    return quantities(out), len(em.hit), sum(1 for m in em.hit if m.in_channels % 32 == 0)


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
