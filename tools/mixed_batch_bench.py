"""Mixed batches (labelled crops + crops of unlabelled frames, cfgs['ss']) on one GPU: what the labelled prefix costs
the training step, and what the unlabelled frames cost the sample front end.

Step ('step'): the native HRNet-W48 coordinates step at N = 32 crops, one model, the variants alternated window by
window in one process:
  all_labelled   target and joints for all 32 crops -- bench.py's train_hc workload
  mixed          n_fs = 24 labelled rows of 32 (the heat-map and coordinate terms over the prefix)
  mixed_cr       the same with the cross-ratio term on (w_cr 0.05 over all 32 rows), as a mixed run trains from its
                 second epoch on
Per variant the ms per step of every window (host clock around ``--steps`` steps ending in a synchronise), their
median and their spread (max - min).

Builder ('builder'): ``TrainSampleBuilder`` on batches of 8 KITTI-sized labelled frames (375 x 1242, 4 boxes each),
labelled only and mixed (max_per_img 6: two crops of one unlabelled frame per labelled frame, the record carries the
frame), the unlabelled frames once at KITTI size and once at ApolloScape size (2710 x 3384).  Per configuration the
median over the windows of the means of: host_ms (draws, box math, packing into the pinned buffer), h2d_ms (the one
staging copy), kernel_ms (crop launch + target launch, device events) and wall_ms; and the bytes uploaded.

    python tools/mixed_batch_bench.py [--steps 10] [--warmup 3] [--windows 3] [--out profiles/mixed_batch_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egonet_amd import configs, synth                                    # noqa: E402
from egonet_amd.common import crop_gpu, train_samples as ts              # noqa: E402

CFG = {'train': True,
       'dataset': {'pth_transform': {'mean': list(crop_gpu.IMAGENET_MEAN), 'std': list(crop_gpu.IMAGENET_STD)}},
       'heatmapModel': {'add_xy': False, 'jitter_bbox': True,
                        'jitter_params': {'shift': [0.1, 0.1], 'scaling': [0.4, 0.4]},
                        'input_size': [256, 256], 'heatmap_size': [64, 64], 'num_joints': 33,
                        'target_type': 'gaussian', 'sigma': 1}}
KITTI_HW, APOLLO_HW = (375, 1242), (2710, 3384)


def _summary(windows):
    w = [float(v) for v in windows]
    return {'median': round(float(np.median(w)), 3), 'min': round(min(w), 3), 'max': round(max(w), 3),
            'spread': round(max(w) - min(w), 3), 'windows': [round(v, 3) for v in w]}


def bench_step(n, n_fs, steps, warmup, windows):
    from egonet_amd.model.heatmapModel import hrnet
    from egonet_amd.train_hrnet import HRNetTrainStep
    cfg = configs.w48_config('coordinates')
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=1))
    net = net.cuda().train()
    tr = HRNetTrainStep(net, lr=1e-3, w_cr=0.05)
    g = torch.Generator().manual_seed(100)
    x = synth.synth_crops(n, 3, 256, 256, seed=50).cuda()
    tgt = torch.rand(n, 33, 64, 64, generator=g).cuda()
    jt = (torch.rand(n, 33, 2, generator=g) * 256).cuda()
    tgt_fs, jt_fs = tgt[:n_fs].contiguous(), jt[:n_fs].contiguous()

    def run(variant):
        tr.apply_cr_loss = variant == 'mixed_cr'
        if variant == 'all_labelled':
            return tr.step(x, tgt, jt)
        return tr.step(x, tgt_fs, jt_fs)
    variants = ['all_labelled', 'mixed', 'mixed_cr']
    for v in variants:
        for _ in range(warmup):
            run(v)
    torch.cuda.synchronize()
    ms = {v: [] for v in variants}
    for w in range(windows):
        for v in (variants if w % 2 == 0 else variants[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = run(v)
            torch.cuda.synchronize()
            ms[v].append((time.perf_counter() - t0) * 1e3 / steps)
            assert np.isfinite(float(loss.item())), v
    del tr, net
    torch.cuda.empty_cache()
    out = {'model': 'W48 coordinates, 256x256', 'N': n, 'n_fs': n_fs, 'steps_per_window': steps, 'warmup': warmup,
           'ms_per_step': {v: _summary(ms[v]) for v in variants}}
    a, m = out['ms_per_step']['all_labelled'], out['ms_per_step']['mixed']
    out['mixed_minus_all_labelled_ms'] = round(m['median'] - a['median'], 3)
    out['within_spread'] = bool(m['median'] - a['median'] <= max(a['spread'], m['spread']))
    return out


def builder_batches(unlabelled_hw):
    """8 labelled KITTI-sized frames with 4 boxes; ``unlabelled_hw``: each carries one unlabelled frame of that size
    with 6 boxes (two crops of it are kept under max_per_img 6), None: labelled only."""
    records = synth.synth_frame_records(8, 4, 33, seed=5, hw=KITTI_HW)
    if unlabelled_hw is None:
        return records, dict(CFG)
    pool = synth.synth_frame_records(8, 6, 33, seed=6, hw=unlabelled_hw)
    records = [dict(r, ss={'image': u['image'], 'boxes': u['boxes'], 'path': u['path']})
               for r, u in zip(records, pool)]
    return records, dict(CFG, ss={'flag': True, 'max_per_img': 6})


def bench_builder(name, unlabelled_hw, steps, warmup, windows):
    records, cfg = builder_batches(unlabelled_hw)
    b = ts.TrainSampleBuilder(cfg)
    b.record_timings = True
    np.random.seed(0)
    for _ in range(warmup):
        out = b(records)
    torch.cuda.synchronize()
    n, n_fs = len(out[0]), len(out[1])
    rows = []
    for _ in range(windows):
        win = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = b(records)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            ev = b.last_timings['events']
            win.append([b.last_timings['host_ms'], ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[3]), wall])
        rows.append(np.mean(win, axis=0))
    rows = np.array(rows)
    frames = [r['image'] for r in records] + [r['ss']['image'] for r in records if 'ss' in r]
    up = int(sum(f.nbytes for f in frames))
    h2d = _summary(rows[:, 1])
    return {'config': name, 'labelled_frames': len(records), 'unlabelled_hw': list(unlabelled_hw or []),
            'N': n, 'n_fs': n_fs, 'frames_uploaded': len(frames), 'upload_bytes': up,
            'host_ms': _summary(rows[:, 0]), 'h2d_ms': h2d, 'kernel_ms': _summary(rows[:, 2]),
            'wall_ms': _summary(rows[:, 3]), 'h2d_gb_per_s': round(up / 1e9 / (h2d['median'] / 1e3), 1),
            'batches_per_window': steps, 'warmup': warmup}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=10, help='steps (batches) per window')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--windows', type=int, default=3)
    ap.add_argument('--out', default=os.path.join('profiles', 'mixed_batch_bench.json'))
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mixed_batch_bench needs a GPU: a timing taken elsewhere says nothing')
    torch.cuda.set_device(0)
    result = {'device': torch.cuda.get_device_name(0), 'windows': a.windows, 'builder': []}
    for name, hw in (('labelled_only', None), ('mixed_kitti_size', KITTI_HW), ('mixed_apollo_size', APOLLO_HW)):
        row = bench_builder(name, hw, a.steps, a.warmup, a.windows)
        print(json.dumps(row), flush=True)
        result['builder'].append(row)
    if not a.no_step:
        result['step'] = bench_step(32, 24, a.steps, a.warmup, a.windows)
        print(json.dumps(result['step']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote %s' % a.out)


if __name__ == '__main__':
    main()
