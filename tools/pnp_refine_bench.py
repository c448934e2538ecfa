#!/usr/bin/env python
"""What the reprojection refinement of lifted cuboids (csrc/pnp_refine.hip) costs.

    python tools/pnp_refine_bench.py [--passes 5] [--steps 20] [--out profiles/pnp_refine_bench.json]

1. The launch alone at n = 16 / 64 / 140 / 1024 instances of 33 correspondences (noisy cuboids, an initial root off by
   up to (0.5, 0.2, 2.0) m, so 6-9 trial steps per instance): hipEvents around ``--reps`` back-to-back launches on
   inputs already in HBM, mean of ``--passes`` passes after a warm-up pass, beside the host twin (the same
   pnp_math.h as a plain loop, host clock).
2. The 64-crop ``EgoNet.infer_crops`` step of bench.py (HRNet-W48, coordinate head, seeded weights) with and without
   ``refine='pnp'`` in the same process: windows of ``--steps`` steps, the two variants alternating, medians of
   ``--passes`` windows; a host clock around work that ends in a device synchronise.  The refined step carries the
   launch and the few element-wise operations around it (relative shape, key point 0 in normalised coordinates).
   The weights are seeded, not trained: the lifted shapes are not cars, and the number of trial steps per fit (the
   file reports the statuses) need not be that of trained weights."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from egonet_amd import _lib, configs, synth                                      # noqa: E402
from egonet_amd.common.img_proc import modify_bbox                               # noqa: E402
from egonet_amd.model.egonet import EgoNet                                       # noqa: E402
import pnp_cases as pc                                                           # noqa: E402

KITTI_K = pc.KITTI_K


def kernel_rows(passes, reps):
    L = _lib.lib()
    rows = []
    for n in (16, 64, 140, 1024):
        case = pc.make(n, J=33, seed=n, noisy=True)
        up = lambda a: torch.as_tensor(a).cuda()          # noqa: E731
        shape, k, intr, r0 = up(case['shape']), up(case['k']), up(case['intr']), up(case['root0'])
        out = [torch.empty(n, 33, 3, dtype=torch.float64, device='cuda'),
               torch.empty(n, 12, dtype=torch.float64, device='cuda'),
               torch.empty(n, 2, dtype=torch.float64, device='cuda'),
               torch.empty(n, dtype=torch.int32, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda'),
               torch.empty(n, 3, dtype=torch.float64, device='cuda')]
        stream = _lib.current_stream()

        def launch():
            _lib.check(L.egn_pnp_refine_f64(_lib.ptr(shape), _lib.ptr(k), _lib.ptr(intr), None, _lib.ptr(r0), n, 33,
                                            5.0, *[_lib.ptr(o) for o in out], stream))
        dev_us = []
        for p in range(passes + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            if p:
                dev_us.append(e0.elapsed_time(e1) * 1e3 / reps)
        host_us = []
        for p in range(passes + 1):
            t0 = time.perf_counter()
            rc, host = pc.host_refine(L, case['shape'], case['k'], case['intr'], root0=case['root0'])
            if p:
                host_us.append((time.perf_counter() - t0) * 1e6)
        iters = out[3].cpu().numpy()
        rows.append({'instances': n, 'device_us': sum(dev_us) / len(dev_us), 'device_all_us': dev_us,
                     'host_us': sum(host_us) / len(host_us), 'host_all_us': host_us,
                     'refined': int((out[4].cpu().numpy() == 1).sum()), 'mean_iters': float(iters.mean()),
                     'max_iters': int(iters.max()),
                     'max_abs_diff_vs_host_m': float(np.abs(out[0].cpu().numpy() - host['refined']).max())})
    return rows


def step_rows(passes, steps, batch):
    cfg = configs.w48_config('coordinates')
    ego = EgoNet(cfg, pre_trained=False)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=1))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=2))
    ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    ego = ego.eval().cuda()
    crops = synth.synth_crops(batch, 3, 256, 256, seed=100).cuda()
    rets = [modify_bbox(b, 1.0) for b in synth.synth_boxes(batch, seed=5)]
    centers = torch.tensor(np.stack([r['c'] for r in rets]), dtype=torch.float64, device='cuda')
    scales = torch.tensor(np.stack([r['s'] for r in rets]), dtype=torch.float64, device='cuda')

    def window(refine):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            res = ego.infer_crops(crops, centers, scales, K=KITTI_K, decode='coords', to_host=False, refine=refine)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, res
    for refine in (None, 'pnp'):
        window(refine)
    plain, refined = [], []
    for _ in range(passes):
        plain.append(window(None)[0])
        ms, res = window('pnp')
        refined.append(ms)
    status = res['refine_status'].cpu().numpy()
    iters = float(ego.refine_pnp(res['kpts_3d'], res['kpts_2d'], torch.as_tensor(KITTI_K).cuda())['iters'].double().mean())
    p, r = statistics.median(plain), statistics.median(refined)
    return {'batch': batch, 'steps_per_window': steps, 'plain_ms_per_step': p, 'plain_all_ms': plain,
            'refined_ms_per_step': r, 'refined_all_ms': refined, 'refined_minus_plain_ms': r - p,
            'share_of_plain_step_percent': 100.0 * (r - p) / p,
            'statuses': {str(v): int((status == v).sum()) for v in (-1, 0, 1)}, 'mean_iters': iters}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--no-step', action='store_true', help='the launch alone, without the HRNet-W48 step')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pnp_refine_bench.json'))
    a = ap.parse_args(argv)
    if a.passes < 3:
        ap.error('--passes must be at least 3')
    os.environ.setdefault('EGONET_AMD_AUTOTUNE', '0')
    out = {'what': 'microseconds per egn_pnp_refine_f64 launch (hipEvents, mean of the passes, %d launches each) beside '
                   'the host twin, and ms per 64-crop infer_crops step with and without refine=pnp (medians, '
                   'alternating windows)' % a.reps,
           'kernel': kernel_rows(a.passes, a.reps)}
    if not a.no_step:
        out['infer_crops_step'] = step_rows(a.passes, a.steps, a.batch)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({'out': a.out, 'kernel_us': {r['instances']: round(r['device_us'], 1) for r in out['kernel']},
                      'step': out.get('infer_crops_step', {}).get('share_of_plain_step_percent')}))
    return out


if __name__ == '__main__':
    main()
