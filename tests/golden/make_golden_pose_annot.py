#!/usr/bin/env python
"""Generate the 2-D pose annotation fixture by RUNNING THE REFERENCE on the CPU (like make_golden_lifter_pairs.py;
it borrows make_golden's stubs and does not change that script):

  pose_annot.npz   the reference's ``annot_2dpose`` (car_instance.py:221-262 ``_prepare_key_points_custom`` ->
                   get_2d_3d_pair :902-1010, then :304-346 ``_prepare_2d_pose_annot``) for hand-written label and
                   calibration texts.

The reference's own methods run on an instance made with ``object.__new__(KITTI)`` plus the attributes they read;
``get_img_size`` returns the record's size.

Cases (prefix '<case>/'):
  main   33 points (coef 0.332, 0.667), seven frames:
           0  no Car line (a Pedestrian and a DontCare line only)
           1  one car fully inside the image
           2  one car with 9 of 33 points visible (dropped), one with 10 (kept), other classes in between
           3  its own P2 (f = 512, no shift) and size 1024 x 384: a car behind the camera (negative depth), a car
              whose centre projects exactly to u = 0 and one exactly to u = width (not visible: strict comparison; their
              sizes are float32 numbers, so that the centre of the cuboid is exactly its location)
           4  one car far outside: dropped, the frame is skipped
           5  33 cars (more than one block of 32 instances), some outside
           6  a third P2, two cars
  c21    the same texts with coef (0.5,): 21 points
  tiny   three frames of 64 x 48 pixels with a matching P2 (what the training-tool test writes as PNG files)
  main_t13, c21_t9   main / c21 with ``_prepare_2d_pose_annot(threshold=13 / 9)``: the second filter drops instances
         the 30 % filter kept (with the reference's threshold 4 it never does), one frame keeps a part of its raw
         instances, in main_t13 one frame with a raw instance is skipped: kpts and raw_kpts, the per-frame counts and the totals of
         the two levels differ
The texts and sizes are stored once per set ('texts/<set>/...', UTF-8 bytes).  Each case: the reference's five lists (paths as file names; boxes, rots,
kpts, raw_kpts concatenated over the kept frames with the per-frame counts; the float64 rows of kpts and raw_kpts as
row numbers into the raw_kpts of the case with the same texts and coefficients at threshold 4, whose rows they equal
bit for bit), and per label the visible count.

The script refuses to write unless every box corner is farther than 1e-6 from an integer before ``int()`` (the integer
boxes are then compared with array_equal) and the properties above hold.

Usage:  python tests/golden/make_golden_pose_annot.py       (from the repo root)
The generation is deterministic: re-running leaves the file byte-identical.
"""
import json
import logging
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (the reference's import stubs; sets the repository root on sys.path)

ENLARGE = 1.1
P2_B = [512.0, 0.0, 512.0, 0.0, 0.0, 512.0, 192.0, 0.0, 0.0, 0.0, 1.0, 0.0]
P2_TINY = [40.0, 0.0, 32.0, 1.5, 0.0, 40.0, 24.0, 0.25, 0.0, 0.0, 1.0, 0.002]


def _line(kind, lab, alpha=-1.57):
    l, h, w, x, y, z, ry = lab
    return '%s 0.00 0 %.2f 100.00 120.00 300.00 250.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f' \
        % (kind, alpha, h, w, l, x, y, z, ry)


def _calib(P):
    rows = ['P0: ' + ' '.join('%.12e' % v for v in np.eye(3, 4).reshape(-1)),
            'P2: ' + ' '.join('%.12e' % v for v in np.asarray(P, dtype=np.float64).reshape(-1)),
            'R0_rect: ' + ' '.join('%.12e' % v for v in np.eye(3).reshape(-1))]
    return '\n'.join(rows) + '\n'


PED = _line('Pedestrian', [0.8, 1.7, 0.6, 2.0, 1.6, 10.0, 0.3])
DONT = _line('DontCare', [-1, -1, -1, -1000, -1000, -1000, -10], alpha=-10)


def main_frames():
    """(label text, calibration text, (width, height)) per frame of the case 'main'."""
    from egonet_amd import synth
    P_a = np.array(synth.KITTI_P2, dtype=np.float64)
    P_c = P_a.copy()
    P_c[0, 0] = P_c[1, 1] = 707.0493
    P_c[0, 2], P_c[1, 2] = 604.0814, 180.5066
    kitti = (1242, 375)
    rng = np.random.RandomState(517)
    crowd = []
    for i in range(33):
        z = rng.uniform(6.0, 45.0)
        crowd.append(_line('Car', [rng.uniform(3.2, 5.0), rng.uniform(1.3, 1.9), rng.uniform(1.5, 1.9),
                                   z * rng.uniform(-1.05, 1.05), rng.uniform(1.3, 2.0), z, rng.uniform(-3.14, 3.14)],
                           alpha=rng.uniform(-3.14, 3.14)))
    crowd.insert(7, PED)
    crowd.append(DONT)
    frames = [
        ([PED, DONT], P_a, kitti),
        ([_line('Car', [3.9, 1.5, 1.6, 1.0, 1.65, 20.0, -0.4], alpha=-0.45), DONT], P_a, kitti),
        ([_line('Car', [4.2, 1.5, 1.7, 4.24, 1.6, 4.0, -1.5], alpha=-2.1), PED,
          _line('Car', [4.2, 1.5, 1.7, 3.65, 1.6, 4.0, -1.3], alpha=-1.9), DONT], P_a, kitti),
        ([_line('Car', [4.0, 1.5, 1.6, 1.0, 1.0, -8.0, 0.7], alpha=0.6),
          _line('Car', [4.0, 1.5, 1.75, -8.0, 1.0, 8.0, 0.0], alpha=0.8),
          _line('Car', [4.0, 1.5, 1.75, 8.0, 1.0, 8.0, 0.0], alpha=-0.8), DONT], P2_B, (1024, 384)),
        ([PED, _line('Car', [4.1, 1.4, 1.6, 30.0, 1.6, 12.0, 1.0], alpha=0.2)], P_a, kitti),
        (crowd, P_c, (1238, 374)),
        ([_line('Car', [3.5, 1.6, 1.7, -3.0, 1.7, 15.0, 2.8], alpha=2.9),
          _line('Car', [4.6, 1.8, 1.9, 6.0, 1.8, 28.0, -2.0], alpha=-2.2)], P_c, (1224, 370)),
    ]
    return [('\n'.join(lines) + '\n', _calib(P), size) for lines, P, size in frames]


def tiny_frames():
    size = (64, 48)
    frames = [
        ([_line('Car', [4.0, 1.5, 1.7, 0.5, 1.2, 9.0, 0.4], alpha=0.35),
          _line('Car', [3.6, 1.4, 1.6, -2.5, 1.3, 14.0, -1.1], alpha=-0.9), DONT], P2_TINY, size),
        ([PED, _line('Car', [4.4, 1.6, 1.8, 1.5, 1.4, 12.0, 2.2], alpha=2.0)], P2_TINY, size),
        ([_line('Car', [3.8, 1.5, 1.6, -1.0, 1.1, 8.0, -2.6], alpha=-2.5),
          _line('Car', [4.2, 1.5, 1.7, 3.0, 1.3, 16.0, 1.3], alpha=1.1),
          _line('Car', [4.0, 1.5, 1.6, 40.0, 1.3, 10.0, 0.0], alpha=0.0)], P2_TINY, size),
    ]
    return [('\n'.join(lines) + '\n', _calib(P), size) for lines, P, size in frames]


TEXTS = {'main': main_frames, 'tiny': tiny_frames}
# name: (texts, coef, threshold of _prepare_2d_pose_annot)
CASES = {'main': ('main', [0.332, 0.667], 4), 'c21': ('main', [0.5], 4), 'tiny': ('tiny', [0.332, 0.667], 4),
         'main_t13': ('main', [0.332, 0.667], 13), 'c21_t9': ('main', [0.5], 9)}


def run_reference(ci, lip, frames, coef, threshold):
    """The reference's annot_2dpose for the frames, per label the unfiltered visible count, the root's depth and the
    frame, and the box corners before int()."""
    ds = object.__new__(ci.KITTI)
    ds.split, ds.exp_type, ds._inference_mode = 'train', 'instanceto2d', False
    ds._classes = ['Car']
    ds.interp_params = {'flag': True, 'style': 'bbox12', 'coef': coef}
    ds.logger = logging.getLogger('make_golden_pose_annot')
    ds.enlarge_factor = ENLARGE
    with tempfile.TemporaryDirectory() as tmp:
        for d in ('label_2', 'calib', 'kpts'):
            os.makedirs(os.path.join(tmp, d))
        paths, sizes = [], {}
        for f, (lt, ct, size) in enumerate(frames):
            with open(os.path.join(tmp, 'label_2', '%06d.txt' % f), 'w') as fh:
                fh.write(lt)
            with open(os.path.join(tmp, 'calib', '%06d.txt' % f), 'w') as fh:
                fh.write(ct)
            paths.append(os.path.join(tmp, 'image_2', '%06d.png' % f))
            sizes[paths[-1]] = size
        ds.get_img_size = lambda path: sizes[path]
        ds._data_config = {'image_path_list': paths, '3d_kpt_sample_style': 'bbox9',
                           'image_dir': os.path.join(tmp, 'image_2'), 'keypoint_dir': os.path.join(tmp, 'kpts'),
                           'label_dir': os.path.join(tmp, 'label_2'), 'calib_dir': os.path.join(tmp, 'calib')}
        visible, depth, frame_of = [], [], []
        for p in paths:                                  # every label, unfiltered: the visible counts
            l2, l3, _, _ = ds.get_2d_3d_pair(p, style='bbox9', augment=False, add_visibility=True,
                                             filter_outlier=False)
            visible += [int(k[0, :, 2].sum()) for k in l2]
            depth += [float(np.asarray(c).reshape(-1, 3)[0, 2]) for c in l3]
            frame_of += [paths.index(p)] * len(l2)
        ds._prepare_key_points_custom('bbox9', ds.interp_params)
        annot = ds._prepare_2d_pose_annot(threshold=threshold)
    corners = []
    for kpts in annot['kpts']:
        for k in kpts:
            center, crop_size, _, _ = lip.kpts2cs(k, enlarge=ENLARGE)
            corners.append(lip.cs2bbox(center, crop_size))
    annot['paths'] = [os.path.basename(p) for p in annot['paths']]
    return (annot, np.array(visible), np.array(depth), np.array(frame_of),
            np.array(corners, dtype=np.float64).reshape(-1, 4))


def main():
    make_golden._install_stubs()
    sys.path.insert(0, make_golden.REF)
    import libs.common.img_proc as lip
    import libs.dataset.KITTI.car_instance as ci

    arrs = {'cases': np.array(json.dumps({k: {'texts': v[0], 'coef': v[1], 'min_visible': v[2]}
                                          for k, v in CASES.items()})), 'enlarge': np.array(ENLARGE)}
    for tname, make in TEXTS.items():                    # the texts once, as UTF-8 bytes
        frames = make()
        for key, col in (('label_text', 0), ('calib_text', 1)):
            arrs['texts/%s/%s' % (tname, key)] = np.frombuffer(json.dumps([f[col] for f in frames]).encode(), np.uint8)
        arrs['texts/%s/sizes' % tname] = np.array([f[2] for f in frames], dtype=np.int64)
    for name, (tname, coef, threshold) in CASES.items():
        frames = TEXTS[tname]()
        annot, visible, depth, frame_of, corners = run_reference(ci, lip, frames, coef, threshold)
        J = 9 + 12 * len(coef)
        # the conditions that make the comparisons well posed, and the properties the cases are there for
        away = np.abs(corners - np.round(corners))
        assert away.min() > 1e-6, 'a box corner within 1e-6 of an integer before int()'
        assert np.abs(corners).max() < 2 ** 31 - 1
        boxes = np.concatenate(annot['boxes'])
        assert np.array_equal(boxes, np.trunc(corners).astype(boxes.dtype))
        raw = np.concatenate(annot['raw_kpts'])
        kpts = np.concatenate(annot['kpts'])
        assert raw.shape[1:] == (J, 3) and kpts.shape[1:] == (J, 2), (raw.shape, kpts.shape)
        is_raw = visible / J >= 0.3
        is_kept = is_raw & (visible >= threshold)
        frame_kept = np.bincount(frame_of[is_kept], minlength=len(frames))
        frame_raw = np.bincount(frame_of[is_raw], minlength=len(frames))
        assert len(kpts) == is_kept.sum() and len(raw) == frame_raw[frame_kept > 0].sum()
        assert [len(b) for b in annot['boxes']] == list(frame_kept[frame_kept > 0])
        assert [len(r) for r in annot['raw_kpts']] == list(frame_raw[frame_kept > 0])
        if threshold == 4:
            assert np.array_equal(is_raw, is_kept)        # the reference's setting: the second filter drops nothing
        else:
            # the two levels differ: a frame that keeps only a part of its raw instances, and a frame with raw
            # instances that is skipped because none of them is kept
            assert is_kept.sum() < is_raw.sum()
            assert ((frame_kept > 0) & (frame_kept < frame_raw)).any(), (frame_raw, frame_kept)
            if name == 'main_t13':
                assert ((frame_kept == 0) & (frame_raw > 0)).any(), (frame_raw, frame_kept)
        if name in ('main', 'main_t13'):
            assert visible[0] == 33 and list(visible[1:3]) == [9, 10], visible[:3]
        if name == 'main':
            assert annot['paths'] == ['%06d.png' % f for f in (1, 2, 3, 5, 6)], annot['paths']
            assert depth[3] < 0 and visible[3] / J >= 0.3, 'the car behind the camera must be kept'
            f3 = annot['raw_kpts'][2]                     # frame 3: behind, u = 0, u = width
            assert len(f3) == 3, len(f3)
            assert f3[1][0, 0] == 0.0 and f3[1][0, 2] == 0.0, f3[1][0]
            assert f3[2][0, 0] == 1024.0 and f3[2][0, 2] == 0.0, f3[2][0]
            assert 0.0 < f3[1][0, 1] < 384.0 and 0.0 < f3[2][0, 1] < 384.0
            assert len(annot['boxes'][3]) > 1 and len(visible) == 42
            assert len(annot['boxes'][3]) < 33, 'the crowd frame must drop some cars'
        if name == 'tiny':
            assert [len(b) for b in annot['boxes']] == [2, 1, 2], [len(b) for b in annot['boxes']]
        p = name + '/'
        arrs[p + 'paths'] = np.array(json.dumps(annot['paths']))
        arrs[p + 'frame_kept'] = np.array([len(b) for b in annot['boxes']], dtype=np.int64)
        arrs[p + 'frame_raw'] = np.array([len(r) for r in annot['raw_kpts']], dtype=np.int64)
        arrs[p + 'boxes'] = boxes
        arrs[p + 'rots'] = np.concatenate(annot['rots'])
        # float64 rows are stored once: the base case (threshold 4) keeps its raw_kpts, every case names the rows of
        # the base's raw_kpts that its own raw_kpts and kpts ARE, bit for bit (checked here)
        base = [k for k, v in CASES.items() if v[:2] == (tname, coef) and v[2] == 4][0]
        if name == base:
            arrs[p + 'raw_kpts'] = raw
        base_raw = arrs[base + '/raw_kpts']
        key = {r.tobytes(): i for i, r in enumerate(base_raw)}
        assert len(key) == len(base_raw)
        raw_rows = np.array([key[r.tobytes()] for r in raw], dtype=np.int64)
        by_uv = {r[:, :2].tobytes(): i for i, r in enumerate(base_raw)}
        kpts_rows = np.array([by_uv[k.tobytes()] for k in kpts], dtype=np.int64)
        assert np.array_equal(base_raw[raw_rows], raw) and np.array_equal(base_raw[kpts_rows][:, :, :2], kpts)
        arrs[p + 'base'] = np.array(base)
        arrs[p + 'raw_rows'] = raw_rows
        arrs[p + 'kpts_rows'] = kpts_rows
        arrs[p + 'visible'] = visible
        print('%-8s %2d frames, %2d labels, %2d kept at 30 %%, %2d for training, %d frames kept, corners >= %.2e from '
              'an integer' % (name, len(frames), len(visible), len(raw), len(kpts), len(annot['paths']), away.min()))
    path = os.path.join(HERE, 'pose_annot.npz')
    np.savez_compressed(path, **arrs)
    print('%-28s %8.1f KB' % ('pose_annot.npz', os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
