"""Times the KITTI evaluator's device path against the host path of the same tree on a synthetic frame set of the
size of the KITTI validation split (3 769 frames), all three metrics, and checks that the two give the same bits.

    python tools/kitti_eval_bench.py [--frames 3769] [--repeat 5] [--out profiles/kitti_eval3d_bench.json]

Timed: ``evaluate.evaluate_frames`` end to end on packed frames already in host memory (packing to flat arrays, the
copy up, the launches, both synchronisations and the curves are inside; parsing text files is not, it is the same code
on both paths).  The median of ``--repeat`` runs after one warm-up run each.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egonet_amd import evaluate                                        # noqa: E402

NAMES = ['Car', 'Car', 'Car', 'Car', 'Van', 'Pedestrian', 'Pedestrian', 'Person_sitting', 'Cyclist', 'DontCare', 'Truck']


def synthetic_frames(n_frames, seed=0):
    """Frames with 4 .. 14 labelled objects, a jittered detection on most of them and 0 .. 4 strays."""
    rng = np.random.RandomState(seed)
    gts, dets = [], []
    for _ in range(n_frames):
        n = rng.randint(4, 15)
        names = [NAMES[k] for k in rng.randint(0, len(NAMES), n)]
        x1, y1 = rng.uniform(0, 1100, n), rng.uniform(100, 300, n)
        bbox = np.stack([x1, y1, x1 + rng.uniform(20, 200, n), y1 + rng.uniform(15, 120, n)], axis=1)
        dims = np.array([1.5, 1.6, 3.9]) * rng.uniform(0.8, 1.2, (n, 3))
        loc = np.stack([rng.uniform(-25, 25, n), rng.uniform(1.2, 1.9, n), rng.uniform(5, 70, n)], axis=1)
        ry, alpha = rng.uniform(-3.1, 3.1, n), rng.uniform(-3.1, 3.1, n)
        dc = np.array([t == 'DontCare' for t in names])
        dims[dc], loc[dc], ry[dc], alpha[dc] = -1, -1000, -10, -10
        gts.append({'type': names, 'truncation': rng.choice([0.0, 0.1, 0.25, 0.4], n), 'occlusion': rng.randint(0, 3, n),
                    'alpha': alpha, 'bbox': bbox, 'dimensions': dims, 'location': loc, 'rotation_y': ry})
        keep = np.flatnonzero((rng.rand(n) < 0.85) & ~dc)
        m, s = len(keep), rng.randint(0, 5)
        size = bbox[keep, 2:] - bbox[keep, :2]
        d_bbox = bbox[keep] + rng.uniform(-0.1, 0.1, (m, 4)) * np.concatenate([size, size], axis=1)
        sx1, sy1 = rng.uniform(0, 1100, s), rng.uniform(100, 300, s)
        stray = np.stack([sx1, sy1, sx1 + rng.uniform(20, 150, s), sy1 + rng.uniform(10, 90, s)], axis=1)
        d_names = [names[k] if names[k] in ('Car', 'Pedestrian', 'Cyclist') else 'Car' for k in keep]
        dets.append({'type': d_names + ['Car'] * s,
                     'alpha': np.concatenate([alpha[keep] + rng.normal(0, 0.3, m), rng.uniform(-3, 3, s)]),
                     'bbox': np.concatenate([d_bbox, stray]),
                     'dimensions': np.concatenate([dims[keep] * rng.uniform(0.95, 1.05, (m, 3)),
                                                   np.array([1.5, 1.6, 3.9]) * rng.uniform(0.8, 1.2, (s, 3))]),
                     'location': np.concatenate([loc[keep] + rng.normal(0, 0.15, (m, 3)) * np.array([1, 0.3, 1]),
                                                 np.stack([rng.uniform(-25, 25, s), rng.uniform(1.2, 1.9, s),
                                                           rng.uniform(5, 70, s)], axis=1)]),
                     'rotation_y': np.concatenate([ry[keep] + rng.normal(0, 0.05, m), rng.uniform(-3, 3, s)]),
                     'score': rng.uniform(0.05, 1.0, m + s)})
    return gts, dets


def timed(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=3769)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'kitti_eval3d_bench.json'))
    a = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), 'the device path needs a GPU'
    gts, dets = synthetic_frames(a.frames)
    host = evaluate.evaluate_frames(gts, dets, device='cpu')
    dev = evaluate.evaluate_frames(gts, dets, device='cuda')
    for name in evaluate.CLASSES:
        for k in ('precision', 'aos', 'precision_ground', 'precision_3d'):
            assert host[name][k].tobytes() == dev[name][k].tobytes(), (name, k)
    t_host = timed(lambda: evaluate.evaluate_frames(gts, dets, device='cpu'), a.repeat)
    t_dev = timed(lambda: evaluate.evaluate_frames(gts, dets, device='cuda'), a.repeat)
    t_pack = timed(lambda: (evaluate._pack(gts, False), evaluate._pack(dets, True)), a.repeat)
    out = {'frames': a.frames, 'ground_truths': int(sum(len(g['type']) for g in gts)),
           'detections': int(sum(len(d['type']) for d in dets)),
           'pairs': int(sum(len(g['type']) * len(d['type']) for g, d in zip(gts, dets))),
           'metrics': list(evaluate.METRICS), 'repeat': a.repeat, 'device': torch.cuda.get_device_name(0),
           'host_ms': {'median': statistics.median(t_host), 'min': min(t_host), 'max': max(t_host)},
           'device_ms': {'median': statistics.median(t_dev), 'min': min(t_dev), 'max': max(t_dev)},
           'python_packing_ms_inside_both': statistics.median(t_pack),
           'same_bits': True,
           'AP_3d_car': dev['car']['AP_3d'], 'AP_bev_car': dev['car']['AP_bev'], 'AP_car': dev['car']['AP']}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
