"""Training cost of the pixel-shuffle heat-map head (hrnet.py:373-383, 598-600) on HRNet-W48, 256 x 256 crops,
heatmap_size = input_size (upsampling factor 4), synthetic crops / targets / weights:

  native    HRNetTrainStep.step (forward, fused pixel-shuffle loss, backward, Adam: HIP launches only)
  base      the same step on the plain heat-map head (final_layer only): native minus base = the head's cost
  bridge    the reference's loop  optim.zero_grad(); loss = JointsMSELoss(model(x)); loss.backward(); optim.step()
            on the autograd bridge (one node on the native tape; torch owns loss and Adam)
  torch     that loop with EGONET_AMD_AUTOGRAD=0: the module graph in torch (MIOpen / rocBLAS)

    python tools/train_heads_bench.py [--batch 32] [--steps 5] [--warmup 2] [--modes native,base,bridge,torch]

Prints one JSON line per mode (ms per step: mean / min over the timed steps, each step synchronised).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egonet_amd import configs, synth                                   # noqa: E402
from egonet_amd.model.heatmapModel import hrnet                         # noqa: E402
from egonet_amd.train_hrnet import HRNetTrainStep                       # noqa: E402
from oracle.hrnet_train_oracle import joints_mse_loss                   # noqa: E402


def _model(pixel_shuffle):
    cfg = configs.w48_config('heatmap')
    if pixel_shuffle:
        cfg['heatmapModel']['pixel_shuffle'] = True
        cfg['heatmapModel']['heatmap_size'] = [256, 256]
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=1))
    return net.cuda().train(), cfg


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sum(ts) / len(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--modes', default='native,base,bridge,torch')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    n = a.batch
    g = torch.Generator().manual_seed(100)
    x = synth.synth_crops(n, 3, 256, 256, seed=50).cuda()
    for mode in a.modes.split(','):
        if mode == 'base':
            net, cfg = _model(False)
            tgt = torch.rand(n, 33, 64, 64, generator=g).cuda()
        else:
            net, cfg = _model(True)
            tgt = torch.rand(n, 33, 256, 256, generator=g).cuda()
        if mode in ('native', 'base'):
            tr = HRNetTrainStep(net, lr=1e-3, w_coor=0.0)

            def fn():
                tr.step(x, tgt, None)
        elif mode in ('bridge', 'torch'):
            os.environ['EGONET_AMD_AUTOGRAD'] = '1' if mode == 'bridge' else '0'
            optim = torch.optim.Adam(net.parameters(), lr=1e-3)

            def fn():
                optim.zero_grad()
                joints_mse_loss(net(x), tgt).backward()
                optim.step()
        else:
            raise SystemExit('unknown mode %r' % mode)
        mean, best = _time(fn, a.steps, a.warmup)
        print(json.dumps({'mode': mode, 'model': 'W48 heatmap' + (' + pixel shuffle f=4' if mode != 'base' else ''),
                          'batch': n, 'ms_per_step': round(mean, 2), 'ms_min': round(best, 2),
                          'crops_per_s': round(n * 1e3 / mean, 1), 'steps': a.steps, 'warmup': a.warmup}), flush=True)
        del net, fn
        torch.cuda.empty_cache()
    os.environ.pop('EGONET_AMD_AUTOGRAD', None)


if __name__ == '__main__':
    main()
