#!/usr/bin/env python
"""What the key-point model's source-image metric (get_distance_src / JointDistance2DSIP) costs with the whole metric
on the device (csrc/kpt_metrics.hip) against the host path of the same tree, on the same box.

    python tools/kpt_metrics_bench.py [--passes 7] [--steps 10] [--out profiles/kpt_metrics_bench.json]
    python tools/kpt_metrics_bench.py --kernel-only       # a few device passes, for rocprofv3 --kernel-trace --stats

1. A validation pass: ``trainer.evaluate`` with ``Evaluator(['JointDistance2DSIP'])`` over ``--batches`` batches of
   16 and of 140 instances (33 joints, 64 x 64 maps), ending with ``report()``, i.e. with the device path's one
   read-back.  The model is a stub that hands out heat-maps already in HBM, so a pass is the loader, the metric and
   nothing else; the host pass is the same evaluator with ``device_update`` off (decode on the device, coordinates and
   maxima copied to the host, the per-instance numpy loop).
2. The HC training step (HRNet-W48, 256 x 256, B = 32, coordinate head; bench.py's train_hc set-up) followed by the
   metric, as ``trainer.train`` calls it on every batch: plain ``get_distance_src``, ``DistanceSrcMeter.accumulate``
   (read back once per window, like a report), and no metric.  Milliseconds per step over windows of ``--steps``
   steps.
Medians of ``--passes`` after two warm-up rounds, the variants alternating inside every round; a host clock around
work that ends in a device synchronise."""
import argparse
import json
import logging
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egonet_amd import configs, synth, trainer                                    # noqa: E402
from egonet_amd.metric.criterions import DistanceSrcMeter, Evaluator, get_distance_src   # noqa: E402

K, HM = 33, 64


def labels(n, seed):
    """Seeded crop boxes and annotated joints of n instances (numpy, like TrainSampleBuilder's meta)."""
    rng = np.random.RandomState(seed)
    center = rng.rand(n, 2) * [1242.0, 375.0]
    scale = np.repeat(0.3 + rng.rand(n, 1) * 1.5, 2, axis=1)
    joints = np.concatenate([center[:, None] + (rng.rand(n, K, 2) - 0.5) * 200 * scale[:, None],
                             (rng.rand(n, K, 1) > 0.2).astype(np.float64)], axis=2)
    return {'center': center, 'scale': scale, 'original_joints': joints}


class _Batches(torch.utils.data.Dataset):
    def __init__(self, batches, per_batch):
        self.n, self.meta = batches * per_batch, labels(batches * per_batch, seed=7)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return torch.zeros(1), torch.zeros(1), torch.ones(1), i

    def collate(self, items):
        idx = [it[3] for it in items]
        z = torch.zeros(len(items), 1)
        return z, z, z, {k: v[idx] for k, v in self.meta.items()}


class _Stub(torch.nn.Module):
    def __init__(self, maps):
        super().__init__()
        self.maps = maps

    def forward(self, data):
        return self.maps[:data.shape[0]]


def eval_cfgs(per_batch):
    return {'use_gpu': True, 'heatmapModel': {'num_joints': K, 'input_size': [256, 256]},
            'testing_settings': {'arg_max': 'hard', 'batch_size': per_batch, 'num_threads': 0, 'shuffle': False,
                                 'unnormalize': False, 'apply_dropout': False}}


def one_pass(ds, model, cfgs, logger, device):
    ev = Evaluator(['JointDistance2DSIP'], cfgs)
    ev.metrics[0].device_update = device
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.evaluate(ds, model, None, cfgs, logger, ev, collate_fn=ds.collate)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, ev.metrics[0]


def bench_evaluate(a, logger):
    out = []
    for per_batch in (16, 140):
        ds = _Batches(a.batches, per_batch)
        maps = torch.randn(per_batch, K, HM, HM, generator=torch.Generator().manual_seed(5)).cuda()
        model, cfgs = _Stub(maps), eval_cfgs(per_batch)
        if a.kernel_only:
            for _ in range(3):
                one_pass(ds, model, cfgs, logger, True)
            continue
        times = {True: [], False: []}
        for i in range(a.passes + 2):
            for device in (True, False):                    # alternating: the same conditions for both
                t, m = one_pass(ds, model, cfgs, logger, device)
                if i >= 2:
                    times[device].append(t)
                if device:
                    dev_m = m
        entry = {'instances_per_batch': per_batch, 'batches': a.batches, 'device_s': statistics.median(times[True]),
                 'host_s': statistics.median(times[False]), 'device_all_s': times[True], 'host_all_s': times[False],
                 'rel_diff_mean': float(abs(dev_m.mean - m.mean) / m.mean),
                 'counts_equal': bool(dev_m.count == m.count and np.array_equal(dev_m.PCK_counts, m.PCK_counts))}
        out.append(entry)
        print('%3d instances x %d batches: device %.3f ms, host %.3f ms per pass' % (
            per_batch, a.batches, 1e3 * entry['device_s'], 1e3 * entry['host_s']), flush=True)
    return out


def bench_train_step(a):
    from egonet_amd.model.heatmapModel import hrnet
    from egonet_amd.train_hrnet import HRNetTrainStep
    B = 32
    cfg = configs.w48_config('coordinates')
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=1))
    net = net.cuda().train()
    tr = HRNetTrainStep(net, lr=1e-3)
    g = torch.Generator().manual_seed(100)
    x = synth.synth_crops(B, 3, 256, 256, seed=50).cuda()
    tgt = torch.rand(B, K, HM, HM, generator=g).cuda()
    jt = (torch.rand(B, K, 2, generator=g) * 256).cuda()
    meta = labels(B, seed=9)
    meter = DistanceSrcMeter(cfg)

    def window(kind):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.step(x, tgt, jt)
            prediction = (tr.last_maps, tr.last_coords)
            if kind == 'plain':
                get_distance_src(prediction, meta, cfg)
            elif kind == 'meter':
                meter.accumulate(prediction, meta, cfg)
        if kind == 'meter':
            meter.read()                                    # the report's read-back, once per window
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps

    kinds = ('none', 'plain', 'meter')
    times = {k: [] for k in kinds}
    for i in range(a.passes + 2):
        for k in kinds:
            t = window(k)
            if i >= 2:
                times[k].append(t)
    entry = {'batch': B, 'steps_per_window': a.steps}
    for k in kinds:
        entry[k + '_ms_per_step'] = 1e3 * statistics.median(times[k])
        entry[k + '_all_ms'] = [1e3 * t for t in times[k]]
    entry['plain_minus_none_ms'] = entry['plain_ms_per_step'] - entry['none_ms_per_step']
    entry['meter_minus_none_ms'] = entry['meter_ms_per_step'] - entry['none_ms_per_step']
    print('HC training step, B = %d: no metric %.3f ms, get_distance_src %.3f ms, meter %.3f ms per step' % (
        B, entry['none_ms_per_step'], entry['plain_ms_per_step'], entry['meter_ms_per_step']), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--batches', type=int, default=20, help='batches of a validation pass')
    ap.add_argument('--steps', type=int, default=10, help='training steps per timed window')
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--no-train-step', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('kpt_metrics_bench: needs the GPU')
    logger = logging.getLogger('kpt_metrics_bench')
    logger.addHandler(logging.NullHandler())
    logger.propagate = False
    result = {'what': 'seconds per trainer.evaluate pass with Evaluator([JointDistance2DSIP]) over a stub model '
                      '(33 joints, 64 x 64 maps, hard arg-max), and ms per HRNet-W48 training step (B = 32) followed '
                      'by the metric; medians of %d after 2 warm-up rounds, variants alternating' % a.passes,
              'evaluate': bench_evaluate(a, logger)}
    if a.kernel_only:
        return
    if not a.no_train_step:
        result['train_step'] = bench_train_step(a)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(result, indent=1) + '\n')


if __name__ == '__main__':
    main()
