#!/usr/bin/env python
"""Generate the lifter-pair fixture by RUNNING THE REFERENCE on the CPU (like make_golden_train_samples.py; it
borrows make_golden's stubs and does not change that script):

  lifter_pairs.npz   the reference's ``2dto3d`` data set (car_instance.py:1051-1086 -> get_2d_3d_pair :902-1010,
                     then get_statistics_1d / normalize_1d, basic_classes.py:26-44) for seeded label and
                     calibration files and a seeded global ``np.random``.

The reference's own methods run on an instance made with ``object.__new__(KITTI)`` plus the attributes they read;
``get_img_size`` returns the case's size.  ``np.random.randn`` is wrapped to record the reference's own draws.

Cases (prefix '<case>/'):
  train100  T = 100, three labels in two frames (the shipped setting)
  train8    T = 8, seven frames with their own P2, one frame without a Car line, labels at |x| ~ 0.7 z and beyond,
            one label at the image border, near cars with points behind the camera
  valid     train8's labels, split 'valid': no draws, normalised with train8's statistics
  r3dt      lft_out_rep 'R3d+T'
  noaug     lft_aug False, split 'train': one draw per label
Each: the label / calibration text per frame, sizes, the numpy seed, the recorded draws in call order, the
reference's float32 input / output before normalisation, the keep flags, root_list, statistics and the normalised
arrays.

Usage:  python tests/golden/make_golden_lifter_pairs.py       (from the repo root)
The generation is deterministic: re-running leaves the file byte-identical.
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (the reference's import stubs; sets the repository root on sys.path)

COEF = [0.332, 0.667]
SIZE = (1242, 375)
# name: (split, lft_aug, T, out_rep, label set, seed, statistics of)
CASES = {
    'train100': ('train', True, 100, 'R3d', 'few', 1, None),
    'train8': ('train', True, 8, 'R3d', 'wide', 2, None),
    'valid': ('valid', True, 8, 'R3d', 'wide', 2, 'train8'),
    'r3dt': ('train', True, 8, 'R3d+T', 'few', 3, None),
    'noaug': ('train', False, 8, 'R3d', 'wide', 4, None),
}


def _line(kind, lab):
    l, h, w, x, y, z, ry = lab
    return '%s 0.00 0 -1.57 100.00 120.00 300.00 250.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f' % (kind, h, w, l, x, y, z, ry)


def _calib(rng):
    from egonet_amd import synth
    P = np.array(synth.KITTI_P2, dtype=np.float64)
    P[0, 0] = P[1, 1] = P[0, 0] + rng.uniform(-15, 15)
    P[0, 2] += rng.uniform(-8, 8)
    P[1, 2] += rng.uniform(-8, 8)
    rows = ['P0: ' + ' '.join('%.12e' % v for v in np.eye(3, 4).reshape(-1)),
            'P2: ' + ' '.join('%.12e' % v for v in P.reshape(-1)),
            'R0_rect: ' + ' '.join('%.12e' % v for v in np.eye(3).reshape(-1))]
    return '\n'.join(rows) + '\n'


def case_text(kind, seed):
    """(label text, calibration text) per frame, from a seed (a private generator, not the global one)."""
    rng = np.random.RandomState(900 + seed)

    def car(z, xr):
        return [rng.uniform(3.2, 5.0), rng.uniform(1.3, 1.9), rng.uniform(1.5, 1.9), z * xr, rng.uniform(1.3, 2.0), z,
                rng.uniform(-np.pi, np.pi)]
    frames = []
    if kind == 'few':
        plan = [[(14.0, 0.2), (31.0, -0.45)], [(8.5, 0.72)]]
    else:
        plan = [[(12.0, 0.7), (25.0, -0.75), (40.0, 0.1)],
                [(2.0, 0.3), (18.0, 0.92), (9.0, -0.85)],
                [],                                              # no Car line
                [(30.0, 1.0), (6.0, -0.7), (50.0, 0.78)],
                [(1.8, -0.2), (22.0, 0.84), (15.0, -1.05)],
                [(10.0, 0.858), (35.0, -0.9), (4.0, 0.75)],      # 0.858 z: the centre sits at the right border
                [(20.0, -0.8), (7.0, 0.95), (45.0, 0.6)]]
    for cars in plan:
        lines = [_line('Pedestrian', car(10.0, 0.1)), _line('DontCare', [-1, -1, -1, -1000, -1000, -1000, -10])]
        for z, xr in cars:
            lines.insert(1, _line('Car', car(z, xr)))
        frames.append(('\n'.join(lines) + '\n', _calib(rng)))
    return frames


def main():
    make_golden._install_stubs()
    sys.path.insert(0, make_golden.REF)
    import libs.dataset.KITTI.car_instance as ci
    import libs.dataset.normalization.operations as nop

    log = []
    orig = np.random.randn

    def randn(*a):
        v = orig(*a)
        log.append(np.asarray(v, dtype=np.float64).reshape(-1))
        return v
    np.random.randn = randn
    arrs = {'cases': np.array(json.dumps({k: {'split': v[0], 'lft_aug': v[1], 'T': v[2], 'out_rep': v[3],
                                              'seed': 2000 + v[5], 'statistics_of': v[6]}
                                          for k, v in CASES.items()})),
            'coef': np.array(COEF), 'size': np.array(SIZE)}
    stats_of = {}
    for name, (split, aug, T, out_rep, kind, seed, stats_from) in CASES.items():
        frames = case_text(kind, seed)
        ds = object.__new__(ci.KITTI)
        ds.split, ds.exp_type, ds._inference_mode = split, '2dto3d', False
        ds._classes = ['Car']
        ds.interp_params = {'flag': True, 'style': 'bbox12', 'coef': COEF}
        ds.get_img_size = lambda path: SIZE
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, 'label_2'))
            os.makedirs(os.path.join(tmp, 'calib'))
            paths = []
            for f, (lt, ct) in enumerate(frames):
                with open(os.path.join(tmp, 'label_2', '%06d.txt' % f), 'w') as fh:
                    fh.write(lt)
                with open(os.path.join(tmp, 'calib', '%06d.txt' % f), 'w') as fh:
                    fh.write(ct)
                paths.append(os.path.join(tmp, 'image_2', '%06d.png' % f))
            ds._data_config = {'image_path_list': paths, '3d_kpt_sample_style': 'bbox9', 'lft_in_rep': 'coordinates2d',
                               'lft_out_rep': out_rep, 'lft_aug': aug, 'lft_aug_times': T,
                               'label_dir': os.path.join(tmp, 'label_2'), 'calib_dir': os.path.join(tmp, 'calib')}
            del log[:]
            np.random.seed(2000 + seed)
            # all samples, unfiltered, for the keep flags and the conditions below: the same seed, the same draws
            unf2d, unf3d = [], []
            augment = aug if split == 'train' else False
            for p in paths:
                l2, l3, _, _ = ds.get_2d_3d_pair(p, style='bbox9', in_rep='coordinates2d', out_rep='R3d+T',
                                                 augment=augment, augment_times=T, add_visibility=True,
                                                 filter_outlier=False)
                unf2d += l2
                unf3d += l3
            del log[:]
            np.random.seed(2000 + seed)
            ds.generate_pairs()
        draws = np.concatenate(log) if log else np.zeros(0)
        inp, out = ds.input.copy(), ds.output.copy()
        assert inp.dtype == np.float32 and out.dtype == np.float32
        u = np.vstack(unf2d)                                        # [n, J, 3]: u, v, visible
        keep = u[:, :, 2].sum(axis=1) / u.shape[1] >= 0.3
        assert keep.sum() == len(inp), (keep.sum(), len(inp))
        assert np.array_equal(u[keep][:, :, :2].reshape(len(inp), -1).astype(np.float32), inp)
        cam = np.vstack(unf3d).reshape(len(u), -1, 3)
        cam[:, 1:] += cam[:, :1]
        # conditions that make the GPU comparisons well posed
        edge = np.minimum(np.minimum(np.abs(u[..., 0]), np.abs(u[..., 0] - SIZE[0])),
                          np.minimum(np.abs(u[..., 1]), np.abs(u[..., 1] - SIZE[1])))
        assert edge.min() > 1e-6, 'a coordinate within 1e-6 px of a visibility bound'
        assert np.abs(cam[..., 2]).min() > 1e-3, 'a point with |z| < 1e-3'
        if name == 'train8':
            share = 1.0 - keep.mean()
            assert share >= 0.05 and keep.mean() >= 0.5, share
            assert (cam[..., 2] < 0).any(), 'no sample with a point behind the camera'
        ds.normalize() if stats_from is None else ds.normalize(stats_of[stats_from])
        stats_of[name] = ds.statistics
        p = name + '/'
        arrs[p + 'label_text'] = np.array(json.dumps([f[0] for f in frames]))
        arrs[p + 'calib_text'] = np.array(json.dumps([f[1] for f in frames]))
        arrs[p + 'np_seed'] = np.array(2000 + seed)
        arrs[p + 'draws'] = draws
        arrs[p + 'input'] = inp
        arrs[p + 'output'] = out
        arrs[p + 'keep'] = keep
        if hasattr(ds, 'root_list'):
            arrs[p + 'root_list'] = np.asarray(ds.root_list)
        for k in ('mean_in', 'std_in', 'mean_out', 'std_out'):
            arrs[p + k] = np.asarray(ds.statistics[k])
        arrs[p + 'input_norm'] = ds.input
        arrs[p + 'output_norm'] = ds.output
        print('%-9s %4d samples, %4d kept (%.1f %% dropped), %5d draws, behind the camera: %d'
              % (name, len(keep), keep.sum(), 100 * (1 - keep.mean()), len(draws), (cam[..., 2] < 0).any(axis=1).sum()))
    np.random.randn = orig
    path = os.path.join(HERE, 'lifter_pairs.npz')
    np.savez_compressed(path, **arrs)
    print('%-28s %8.1f KB' % ('lifter_pairs.npz', os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
