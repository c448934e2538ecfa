#!/usr/bin/env python
"""Generate the lifter-metric fixture by RUNNING THE REFERENCE on the CPU (it borrows make_golden's stubs and does not
change that script):

  lifter_metrics.npz   the reference's ``RError3D``, ``RTError3D``, ``JointDistance3D`` ('direct'),
                       ``RotationError3D`` and ``Evaluator(['RError3D'])`` (libs/metric/criterions.py:223-573) fed with
                       seeded rows in batches of 128 + 128 + 44, unnormalised on the host like
                       libs/trainer/trainer.py:474-481.

Rows: 33-point cuboids (centre, 8 corners, 24 edge points) of random size, rotated about y, somewhere in front of
the camera; the target is the cuboid, the prediction the cuboid plus Gaussian noise of 1 mm, 5 cm or 50 cm (row
i % 3), so the errors span almost nothing to several degrees.  Both are stored NORMALISED (float32) with their
float32 statistics, for 'R3d' (96 columns) and 'R3d+T' (99).

Per class: every attribute after the last batch and the ``report()`` lines.  The generator also runs the float64
restatement (tests/lifter_metrics_ref.py) on the same rows and stores ``max |restatement - reference|`` per
attribute under ``gap/``: the reference computes distances, H and the SVD in float32, so this is the reference's own
rounding, and the GPU test's bound is ten times it.  scipy's gimbal-lock warning is an error here: the committed
rows hold no such row.

Usage:  python tests/golden/make_golden_lifter_metrics.py       (from the repo root)
The generation is deterministic: re-running leaves the file byte-identical.
"""
import json
import logging
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402  (the reference's import stubs; sets the repository root on sys.path)
import lifter_metrics_ref as ref  # noqa: E402

N = 300
BATCHES = (128, 128, 44)
NOISE = (0.001, 0.05, 0.5)
COEF = (0.332, 0.667)
EDGES = ((0, 1), (2, 3), (4, 5), (6, 7), (0, 4), (1, 5), (2, 6), (3, 7), (0, 2), (1, 3), (4, 6), (5, 7))


def cuboids(n, rng):
    """[n, 33, 3] camera coordinates: centre first."""
    out = np.zeros((n, 33, 3))
    for i in range(n):
        l, h, w = rng.uniform(3.2, 5.0), rng.uniform(1.3, 1.9), rng.uniform(1.5, 1.9)
        c = np.array([[(l if k < 4 else 0.0) - l / 2, (h if k & 1 else 0.0) - h / 2,
                       (0.0 if (k >> 1) & 1 else w) - w / 2] for k in range(8)])
        pts = [np.zeros(3)] + list(c)
        for coef in COEF:
            pts += [c[a] + coef * (c[b] - c[a]) for a, b in EDGES]
        pts = np.array(pts)
        ry = rng.uniform(-np.pi, np.pi)
        rot = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
        z = rng.uniform(5.0, 50.0)
        out[i] = pts @ rot.T + np.array([z * rng.uniform(-0.6, 0.6), rng.uniform(1.0, 2.0), z])
    return out


def make_rows(layout, seed):
    rng = np.random.RandomState(seed)
    cam = cuboids(N, rng)
    rel = cam[:, 1:] - cam[:, :1]
    gt = rel.reshape(N, -1) if layout == 'R3d' else np.concatenate([cam[:, 0], rel.reshape(N, -1)], axis=1)
    noise = rng.randn(*gt.shape) * np.array(NOISE)[np.arange(N) % 3].reshape(-1, 1)
    gt = gt.astype(np.float32)
    mean = gt.mean(axis=0, keepdims=True).astype(np.float32)
    std = gt.std(axis=0, keepdims=True).astype(np.float32)
    pred = (gt.astype(np.float64) + noise).astype(np.float32)
    return ((pred - mean) / std).astype(np.float32), ((gt - mean) / std).astype(np.float32), mean, std


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def attributes(obj):
    return {k: np.asarray(v, dtype=np.float64) for k, v in vars(obj).items()
            if k.split('_')[0] in ('count', 'mean', 'max', 'min')}


def main():
    warnings.simplefilter('error', UserWarning)          # scipy: "Gimbal lock detected"
    make_golden._install_stubs()
    sys.path.insert(0, make_golden.REF)
    import libs.metric.criterions as rc
    import libs.dataset.normalization.operations as nop

    cfgs = {'metrics': {'R3D': {'T_style': 'direct', 'R_style': 'euler', 'style': 'euler'},
                        'RTError3D': {'T_style': 'direct', 'R_style': 'euler'}, 'JD3D': {'style': 'direct'}},
            'dataset': {'3d_kpt_sample_style': 'bbox9'}, 'FCModel': {'output_size': 96}}
    arrs = {'cfgs': np.array(json.dumps(cfgs)), 'batches': np.array(BATCHES), 'noise': np.array(NOISE)}
    rows, host = {}, {}
    for layout, seed in (('R3d', 31), ('R3d+T', 32)):
        pred, gt, mean, std = make_rows(layout, seed)
        rows[layout] = (pred, gt, mean, std)
        host[layout] = (nop.unnormalize_1d(pred, mean, std), nop.unnormalize_1d(gt, mean, std))
        assert host[layout][0].dtype == np.float32
        assert np.array_equal(host[layout][0], ref.unnormalize_f32(pred, mean, std))
        p = layout + '/'
        arrs[p + 'pred'], arrs[p + 'gt'], arrs[p + 'mean_out'], arrs[p + 'std_out'] = pred, gt, mean, std

    lg = logging.getLogger('make_golden_lifter_metrics')
    lg.setLevel(logging.INFO)
    lg.propagate = False
    cases = {'RError3D': (lambda: rc.RError3D(cfgs, 33), 'R3d'),
             'RTError3D': (lambda: rc.RTError3D(cfgs, 33), 'R3d+T'),
             'JointDistance3D': (lambda: rc.JointDistance3D(cfgs), 'R3d'),
             'RotationError3D': (lambda: rc.RotationError3D(cfgs), 'R3d'),
             'Evaluator': (lambda: rc.Evaluator(['RError3D'], cfgs, 33), 'R3d')}
    print('max |float64 restatement - reference| per attribute:')
    for name, (make, layout) in cases.items():
        obj = make()
        pu, gu = host[layout]
        b0 = 0
        for b in BATCHES:
            obj.update(pu[b0:b0 + b].copy(), ground_truth=gu[b0:b0 + b].copy())
            b0 += b
        assert b0 == N
        h = _Lines()
        lg.handlers = [h]
        obj.report(lg)
        arrs[name + '/report'] = np.array(json.dumps(h.lines))
        arrs[name + '/layout'] = np.array(layout)
        got = attributes(obj.metrics[0] if name == 'Evaluator' else obj)
        want = ref.statistics(ref.rows(*rows[layout][:2], layout, *rows[layout][2:]), layout)
        alias = {'JointDistance3D': '_rT', 'RotationError3D': '_R'}.get(name)
        for k, v in sorted(got.items()):
            arrs['%s/%s' % (name, k)] = v
            w = want[k + alias] if alias else want[k]
            gap = float(np.max(np.abs(np.asarray(w, dtype=np.float64) - v)))
            arrs['gap/%s/%s' % (name, k)] = np.array(gap)
            print('  %-16s %-12s %.3e' % (name, k, gap))
    path = os.path.join(HERE, 'lifter_metrics.npz')
    np.savez_compressed(path, **arrs)
    print('%-28s %8.1f KB' % ('lifter_metrics.npz', os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
