#!/usr/bin/env python
"""Generate tests/golden/angle_baseline.npz by RUNNING THE REFERENCE (the angle-regression baselines,
``exp_type`` 'baselinealpha' / 'baselinetheta').

Runs only where the reference checkout is (``make_golden.py`` explains the stubs: cv2 and torchvision are absent).
It calls the reference's own

  libs.metric.criterions.get_angle_error / AngleError          (:40-55, :145-171)
  libs.loss.function.MSELoss1D / SmoothL1Loss1D                 (:204-228)
  libs.dataset.KITTI.car_instance.KITTI.__getitem__             (:1248-1271; the crop call in front of the target
                                                                lines is replaced by a stand-in, the object is made
                                                                without its constructor)

on three batches of N = 1, 3, 257 rows and a small ``rots`` array, and stores arrays and numbers only.

Usage:  python tests/golden/make_golden_angle.py            (from the repo root)
The generation is deterministic: re-running leaves the committed file byte-identical.
"""
import logging
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                        # noqa: E402  (the stubs, the reference's location)

NS = (1, 3, 257)


class _Last(logging.Handler):
    def emit(self, record):
        self.text = record.getMessage()


def _batches():
    """float32 predictions (any length: atan2 normalises) and float64 angles in [-pi, pi]; every batch with more than
    one row holds rows on both sides of the 180-degree wrap, none within 1e-3 degrees of it."""
    rng = np.random.RandomState(20240607)
    out = []
    for n in NS:
        while True:
            ang = rng.uniform(-np.pi, np.pi, n)
            gt = rng.uniform(-np.pi, np.pi, n)
            if n > 1:
                gt[0], ang[0] = 3.0, -3.0               # |d| = 343.8 degrees: wrapped
                gt[1], ang[1] = 0.5, 0.25               # |d| = 14.3 degrees: not wrapped
            rad = rng.uniform(0.2, 1.5, n)
            pred = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1).astype(np.float32)
            d = np.abs(gt - np.arctan2(pred[:, 1].astype(np.float64), pred[:, 0].astype(np.float64))) * 180 / np.pi
            if np.all(np.abs(d - 180) >= 1e-3):
                break
        if n > 1:
            assert (d > 180).any() and (d < 180).any(), 'both wrap branches in one batch'
        assert np.all(np.abs(d - 180) >= 1e-3), 'no row near the wrap: a float32 / float64 atan2 cannot flip it'
        assert gt.min() >= -np.pi and gt.max() <= np.pi
        out.append((pred, gt))
    return out


def main():
    mg._install_stubs()
    sys.path.insert(0, mg.REF)
    import libs.metric.criterions as ref_metric
    import libs.loss.function as ref_loss
    import libs.dataset.KITTI.car_instance as ref_ds

    data = {'ns': np.array(NS)}
    running = ref_metric.AngleError(None)
    log = logging.getLogger('make_golden_angle')
    log.setLevel(logging.INFO)
    last = _Last()
    log.addHandler(last)
    tgen = np.random.RandomState(7)
    for b, (pred, gt) in enumerate(_batches()):
        avg, cnt, others = ref_metric.get_angle_error(torch.from_numpy(pred), {'angles_gt': gt})
        assert others is None
        running.update(torch.from_numpy(pred), {'angles_gt': gt})
        n = len(pred)
        # targets around the prediction: |d| on both sides of 1 (the SmoothL1 knee) where n allows
        tgt = (pred + tgen.uniform(-2.5, 2.5, pred.shape)).astype(np.float32)
        dd = np.abs(pred - tgt)
        assert n == 1 or ((dd < 1).any() and (dd > 1).any())
        p, t = torch.from_numpy(pred), torch.from_numpy(tgt)
        data.update({'pred%d' % b: pred, 'gt%d' % b: gt, 'tgt%d' % b: tgt,
                     'err%d' % b: np.array([float(avg), float(cnt)]),
                     'running%d' % b: np.array([float(running.mean), float(running.count)]),
                     'mse%d' % b: np.array(float(ref_loss.MSELoss1D()(p, t, torch.ones(1), {}))),
                     'sl1%d' % b: np.array(float(ref_loss.SmoothL1Loss1D()(p, t, torch.ones(1), {})))})
    running.report(log)
    data['report'] = np.array(last.text)

    # car_instance.py:1248-1271 for one frame of five cars
    rots = np.random.RandomState(3).uniform(-np.pi, np.pi, (5, 2))
    rots[0] = [np.pi, -np.pi]
    rots[1] = [0.0, np.pi / 2]
    data['rots'] = rots
    for exp in ('baselinealpha', 'baselinetheta'):
        ds = object.__new__(ref_ds.KITTI)
        ds.split, ds.exp_type, ds.pth_trans, ds._inference_mode = 'train', exp, None, False
        ds.hm_para = {'rf': 0.0, 'sf': 0.0}
        ds.annot_2dpose = {'paths': ['x.png'], 'rots': [rots], 'kpts': [np.zeros((5, 33, 2))],
                           'boxes': [np.zeros((5, 4))]}
        with mock.patch.object(ref_ds.lip, 'get_tensor_from_img', return_value=(None, None, None, {})):
            _, targets, _, meta = ds[0]
        assert targets.dtype == torch.float32 and tuple(targets.shape) == (5, 2)
        data[exp + '_targets'] = targets.numpy()
        data[exp + '_angles_gt'] = np.asarray(meta['angles_gt'], dtype=np.float64)
    path = os.path.join(HERE, 'angle_baseline.npz')
    np.savez(path, **data)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
