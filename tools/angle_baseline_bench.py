#!/usr/bin/env python
"""What an iteration of the angle-regression baselines ('baselinealpha' / 'baselinetheta') costs on the native step with
the metric on the device, against the autograd-bridge loop with the host metric -- the only way to train this head
before ``HRNetTrainStep(angle_type=...)`` -- on the same box.

    python tools/angle_baseline_bench.py [--passes 5] [--steps 5] [--batches 8,32] [--out profiles/angle_baseline_bench.json]

1. Per model (the tiny angle net and HRNet-W48 with the angle head, 256 x 256 crops) and batch size, milliseconds per
   iteration of
     native   ``HRNetTrainStep(angle_type='mse').step(x, t)`` + ``AngleErrorMeter.accumulate`` (one ``read()`` per window,
              like a report)
     bridge   ``optim.zero_grad(); loss = MSELoss1D()(model(x), t); loss.backward(); optim.step()`` (the native tape under
              torch.autograd, torch's Adam) + host ``get_angle_error`` on every batch
   over windows of ``--steps`` iterations.
2. ``TrainSampleBuilder`` per batch of 8 frames x 4 boxes (375 x 1242 frames, 256 x 256 crops, 64 x 64 maps) in angle mode
   against heat-map mode.
Medians of ``--passes`` after two warm-up rounds, the variants alternating inside every round; a host clock around work
that ends in a device synchronise."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egonet_amd import configs, synth                                            # noqa: E402
from egonet_amd.common import train_samples                                       # noqa: E402
from egonet_amd.loss.function import MSELoss1D                                    # noqa: E402
from egonet_amd.metric.criterions import AngleErrorMeter, get_angle_error         # noqa: E402
from egonet_amd.model.heatmapModel import hrnet                                   # noqa: E402
from egonet_amd.train_hrnet import HRNetTrainStep                                 # noqa: E402


def _net(cfg):
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=1))
    return net.cuda().train()


def bench_step(a, name, cfg, B):
    native_net, bridge_net = _net(cfg), _net(cfg)
    tr = HRNetTrainStep(native_net, lr=1e-3, angle_type='mse')
    optim, crit = torch.optim.Adam(bridge_net.parameters(), lr=1e-3), MSELoss1D()
    meter = AngleErrorMeter()
    rng = np.random.RandomState(3)
    gt = rng.uniform(-np.pi, np.pi, B)
    meta = {'angles_gt': gt}
    x = synth.synth_crops(B, 3, 256, 256, seed=50).cuda()
    t = torch.from_numpy(np.stack([np.cos(gt), np.sin(gt)], axis=1).astype(np.float32)).cuda()

    def window(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            if kind == 'native':
                tr.step(x, t)
                meter.accumulate(tr.last_angles, meta)
            else:
                optim.zero_grad()
                prediction = bridge_net(x)
                loss = crit(prediction, t)
                loss.backward()
                optim.step()
                get_angle_error(prediction.detach().cpu(), meta)
        if kind == 'native':
            meter.read()                                    # the report's read-back, once per window
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps

    kinds = ('native', 'bridge')
    times = {k: [] for k in kinds}
    for i in range(a.passes + 2):
        for k in kinds:
            s = window(k)
            if i >= 2:
                times[k].append(s)
    entry = {'model': name, 'batch': B, 'steps_per_window': a.steps}
    for k in kinds:
        entry[k + '_ms_per_iter'] = 1e3 * statistics.median(times[k])
        entry[k + '_all_ms'] = [1e3 * s for s in times[k]]
    print('%-5s B = %3d: native step + meter %.3f ms, bridge loop + host metric %.3f ms per iteration' % (
        name, B, entry['native_ms_per_iter'], entry['bridge_ms_per_iter']), flush=True)
    return entry


def bench_builder(a):
    cfg = configs.clone(configs.w48_config('angleregression'))
    cfg.update(train=True, dataset={'pth_transform': {}})
    cfg['heatmapModel'].update(jitter_bbox=True, jitter_params={'shift': [0.1, 0.1], 'scaling': [0.4, 0.4]},
                               target_type='gaussian', sigma=1)
    recs = synth.synth_frame_records(8, 4, 33, seed=2)
    rng = np.random.RandomState(4)
    for r in recs:
        r['rots'] = rng.uniform(-np.pi, np.pi, (4, 2))
    builders = {m: train_samples.TrainSampleBuilder(cfg, split='train', target=m) for m in ('heatmap', 'theta')}

    def window(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            builders[mode](recs, np.random.RandomState(1))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps

    times = {m: [] for m in builders}
    for i in range(a.passes + 2):
        for m in builders:
            s = window(m)
            if i >= 2:
                times[m].append(s)
    entry = {'frames': 8, 'instances': 32}
    for m in builders:
        entry[m + '_ms_per_batch'] = 1e3 * statistics.median(times[m])
        entry[m + '_all_ms'] = [1e3 * s for s in times[m]]
    print('builder, 8 frames x 4 boxes: heat-map mode %.3f ms, angle mode %.3f ms per batch' % (
        entry['heatmap_ms_per_batch'], entry['theta_ms_per_batch']), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5, help='iterations per timed window')
    ap.add_argument('--batches', default='8,32', help='batch sizes, comma separated')
    ap.add_argument('--models', default='tiny,w48')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('angle_baseline_bench: needs the GPU')
    cfgs = {'tiny': configs.tiny_config('angleregression', input_size=(256, 256)),
            'w48': configs.w48_config('angleregression')}
    result = {'what': 'ms per training iteration of the angle head (256 x 256 crops): native step + AngleErrorMeter against '
                      'the autograd-bridge loop (torch Adam) + host get_angle_error per batch; ms per TrainSampleBuilder '
                      'batch in angle and heat-map mode; medians of %d windows of %d after 2 warm-up rounds, variants '
                      'alternating' % (a.passes, a.steps),
              'step': [bench_step(a, m, cfgs[m], int(b)) for m in a.models.split(',') for b in a.batches.split(',')],
              'builder': bench_builder(a)}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(result, indent=1) + '\n')


if __name__ == '__main__':
    main()
