"""The model, inputs and measured quantities of the precision = 'f16' network-level checks: shared by
tests/golden/make_f16_bounds.py (which writes tests/golden/f16_mode_bounds.json on the CPU), tests/test_f16_mode_cpu.py
and tests/test_gpu_f16_mode.py (imported, not a conftest).

Model: HRNet with the W48 widths on a 64 x 64 input (maps 16 / 8 / 4 / 2), one module per stage, one block per branch, 5
joints; seeded weights and BatchNorm statistics as SURVEY.md section 8c-iii (egonet_amd.synth).  Quantities, each the
maximum absolute deviation from the plain fp32 CPU forward:
  heatmap         the heat-maps, absolute
  softargmax_px   the soft-arg-max of the heat-maps (softmax over the map, expectation of the pixel position, float64 on
                  the host for every forward alike), in INPUT pixels (map pixels x 4)
  coords_px       the coordinate head's output x the input size, pixels ('coordinates' only)
"""
import os

import torch

from egonet_amd import configs, engine, synth
from egonet_amd.model.heatmapModel import hrnet

HEADS = ('heatmap', 'coordinates')
SIZE = 64
BATCHES = {'forward': (3, 0), 'infer_crops': (4, 1)}          # name -> (crops, seed of synth_crops)
BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'f16_mode_bounds.json')


def config(head):
    return configs.hrnet_config(48, (SIZE, SIZE), 5, head, modules=(1, 1, 1), num_blocks=1, lifter_neurons=128)


def model(head, seed=11):
    net = hrnet.get_pose_net(config(head), is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=seed))
    return net.eval()


def crops(which):
    n, seed = BATCHES[which]
    return synth.synth_crops(n, 3, SIZE, SIZE, seed=seed)


def soft_arg_max_px(maps):
    """[N,K,H,W] -> [N,K,2] (x, y) in input pixels, float64."""
    n, k, h, w = maps.shape
    p = torch.softmax(maps.double().reshape(n, k, h * w), dim=2).reshape(n, k, h, w)
    xs = (p.sum(2) * torch.arange(w, dtype=torch.float64)).sum(2)
    ys = (p.sum(3) * torch.arange(h, dtype=torch.float64)).sum(2)
    return torch.stack([xs, ys], dim=2) * (float(SIZE) / w)


def quantities(out):
    """What a forward returned (maps, or (maps, coords)) -> {name: float64 CPU tensor}."""
    maps, coords = (out[0], out[1]) if isinstance(out, tuple) else (out, None)
    maps = maps.detach().cpu()
    q = {'heatmap': maps.double(), 'softargmax_px': soft_arg_max_px(maps)}
    if coords is not None:
        q['coords_px'] = coords.detach().cpu().double() * SIZE
    return q


def deviations(q, q_ref):
    return {k: float((q[k] - q_ref[k]).abs().max()) for k in q_ref}


def cpu_f32(net, x):
    with torch.no_grad():
        return quantities(net(x))


def cpu_emulated(net, x):
    with torch.no_grad(), engine.f16_emulation(net) as em:
        out = net(x)
    return quantities(out), len(em.hit)
