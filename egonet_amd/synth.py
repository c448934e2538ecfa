"""Deterministic synthetic checkpoints and inputs.

The reference ships no weights (docs/preparation.md:28-29 points at a
Google-Drive folder), so benchmarks and parity tests run on *synthetic*
checkpoints.  Every tensor is drawn from its own generator seeded by
``crc32(key) ^ seed``; the values therefore depend only on the state_dict key
and shape, never on module construction order, and can be regenerated
bit-identically on the GPU box (torch's CPU Philox/MT generators are
platform independent for a given torch version).

The scales keep activations O(1) through ~70 conv+BN layers (SURVEY.md
section 8c-iii): conv/linear weights U(-1,1)/sqrt(fan_in), BN gamma in
[0.5,1.5], beta/running_mean ~ 0.2*N(0,1), running_var in [0.5,1.5].
"""
import zlib

import numpy as np
import torch


def _gen(key, seed):
    g = torch.Generator()
    g.manual_seed((zlib.crc32(key.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)
    return g


def synth_tensor(key, shape, seed=0):
    shape = tuple(shape)
    g = _gen(key, seed)
    leaf = key.rsplit('.', 1)[-1]
    if leaf == 'num_batches_tracked':
        return torch.zeros(shape, dtype=torch.long)
    if leaf == 'running_var':
        return 0.5 + torch.rand(shape, generator=g)
    if leaf == 'running_mean':
        return 0.2 * torch.randn(shape, generator=g)
    if leaf == 'weight' and len(shape) == 1:          # BN gamma
        return 0.5 + torch.rand(shape, generator=g)
    if leaf == 'bias':
        return 0.2 * torch.randn(shape, generator=g)
    if leaf == 'weight':
        fan_in = int(np.prod(shape[1:]))
        return (torch.rand(shape, generator=g) * 2 - 1) / np.sqrt(fan_in)
    raise KeyError('no synthetic recipe for ' + key)


def synth_state_dict(template, seed=0):
    """template: mapping key -> tensor (shapes are read, values ignored)."""
    out = {}
    for k, v in template.items():
        out[k] = synth_tensor(k, v.shape, seed).to(v.dtype if v.dtype != torch.long else torch.long)
    return out


def synth_crops(n, c=3, h=256, w=256, seed=0):
    g = torch.Generator()
    g.manual_seed(977 + seed)
    return torch.randn(n, c, h, w, generator=g)


def synth_lifter_stats(n_in=66, n_out=96, seed=0):
    """A plausible LS.npy dict (train_lifting.py:54): float64 [1,n] arrays."""
    rng = np.random.RandomState(4242 + seed)
    return {'mean_in': rng.uniform(300, 900, (1, n_in)),
            'std_in': rng.uniform(40, 120, (1, n_in)),
            'mean_out': rng.uniform(-1, 1, (1, n_out)),
            'std_out': rng.uniform(0.3, 1.5, (1, n_out))}


def synth_boxes(n, seed=0, img_w=1242, img_h=375):
    """n KITTI-like 2D boxes [x1,y1,x2,y2] (float64)."""
    rng = np.random.RandomState(99 + seed)
    w = rng.uniform(30, 320, n)
    h = w * rng.uniform(0.4, 1.3, n)
    x1 = rng.uniform(0, img_w - w)
    y1 = rng.uniform(0, np.maximum(img_h - h, 1))
    return np.stack([x1, y1, x1 + w, y1 + h], axis=1)


def synth_frame_records(n_frames, boxes_per_frame, num_joints, seed=0, hw=(375, 1242)):
    """Training records in the form ``common.train_samples.TrainSampleBuilder`` takes: per frame a seeded
    [H,W,3] uint8 RGB image, ``boxes_per_frame`` boxes from ``synth_boxes``, joints [n,K,3] inside and around
    the boxes (up to 20 % of the box size outside) with visibilities 0 / 0.3 / 1, and a path."""
    rng = np.random.RandomState(7177 + seed)
    H, W = int(hw[0]), int(hw[1])
    records = []
    for f in range(n_frames):
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        boxes = synth_boxes(boxes_per_frame, seed=seed * 1000 + f, img_w=W, img_h=H)
        u = rng.uniform(-0.2, 1.2, (boxes_per_frame, num_joints, 2))
        x = boxes[:, None, 0] + u[..., 0] * (boxes[:, None, 2] - boxes[:, None, 0])
        y = boxes[:, None, 1] + u[..., 1] * (boxes[:, None, 3] - boxes[:, None, 1])
        vis = rng.choice(np.array([0.0, 0.3, 1.0]), size=(boxes_per_frame, num_joints), p=[0.2, 0.2, 0.6])
        records.append({'image': img, 'boxes': boxes, 'joints': np.stack([x, y, vis], axis=2),
                        'path': 'synth/%06d_%03d.png' % (seed, f)})
    return records


KITTI_P2 = [[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]]


def synth_kitti_labels(n_labels, seed=0, per_frame=4, size=(1242, 375)):
    """Seeded KITTI-like car labels in the form ``common.lifter_pairs.LifterPairBuilder`` takes: records of
    ``per_frame`` labels [n,7] float64 (l, h, w, x, y, z, rot_y, rounded to the label files' two decimals), a [3,4]
    float32 ``P`` that varies a little from frame to frame, the image ``size`` (width, height) and a path.  Depths run
    from 2.5 m to 60 m and |x| up to 1.1 z, so a share of the samples falls off the image."""
    rng = np.random.RandomState(5150 + seed)
    records, left, f = [], int(n_labels), 0
    while left > 0:
        n = min(per_frame, left)
        z = rng.uniform(2.5, 60.0, n)
        x = z * rng.uniform(-1.1, 1.1, n)
        y = rng.uniform(1.2, 2.2, n)
        dims = np.stack([rng.uniform(3.2, 5.0, n), rng.uniform(1.3, 1.9, n), rng.uniform(1.5, 1.9, n)], axis=1)
        ry = rng.uniform(-np.pi, np.pi, n)
        labels = np.round(np.concatenate([dims, np.stack([x, y, z, ry], axis=1)], axis=1), 2)
        P = np.array(KITTI_P2, dtype=np.float64)
        P[0, 0] = P[1, 1] = P[0, 0] + rng.uniform(-15, 15)
        P[0, 2] += rng.uniform(-8, 8)
        P[1, 2] += rng.uniform(-8, 8)
        records.append({'labels': labels, 'P': P.astype(np.float32), 'size': (int(size[0]), int(size[1])),
                        'path': 'synth/%06d_%06d.png' % (seed, f)})
        left -= n
        f += 1
    return records
