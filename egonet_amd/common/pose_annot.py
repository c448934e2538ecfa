"""2-D pose annotations: KITTI labels + calibration -> the per-frame ``boxes`` / ``kpts`` / ``rots`` records the
key-point model (HC) trains on, built on the device.

It reproduces the reference's ``annot_2dpose`` (libs/dataset/KITTI/car_instance.py:221-262
``_prepare_key_points_custom`` -> ``get_2d_3d_pair`` :902-1010 with ``augment=False, add_visibility=True,
filter_outlier=True, add_rotation=True``, then :304-346 ``_prepare_2d_pose_annot``): per labelled car the 33-point
cuboid, rotated, translated and projected with the frame's own intrinsics; a point is visible when it lies strictly
inside the image; an instance is kept in ``raw_kpts`` when at least 30 % of its points are visible and for training
when at least 4 are; from there on all points count as visible, the crop box is their bounding rectangle enlarged by
``dataset.enlarge_factor`` with each corner through ``int()``, and ``rots`` holds ``[alpha, rot_y]``.

Split of work.  Host: the text parsers and ``K`` / ``shift`` per frame (``lifter_pairs.frame_row``), the image size
from the record or the image header.  Device (csrc/pose_annot.hip): every label's points, both filters, a stable
compaction in label order, the boxes, and the per-frame counts that cut the flat arrays into the reference's per-frame
lists.  ``build_host`` is the same arithmetic in numpy float64: it serves when no GPU is visible (or ``device='cpu'``)
and is the oracle of the device path.

``PoseFrames`` wraps the annotations as the ``Dataset`` ``train_samples.TrainSampleBuilder`` consumes.
"""
import os

import numpy as np
import torch

from .. import _lib
from . import lifter_pairs as lp

INLIER_SHARE = 0.3          # get_inlier_indices (car_instance.py:870-879)
MIN_VISIBLE = 4             # _prepare_2d_pose_annot(threshold=4) (car_instance.py:304)
EDGE_PARENT = (0, 2, 4, 6, 0, 1, 2, 3, 0, 1, 4, 5)      # interp_dict['bbox12'] (car_instance.py:63-70), 0-based corners
EDGE_CHILD = (1, 3, 5, 7, 4, 5, 6, 7, 2, 3, 6, 7)       # like csrc/pose_math.h


def parse_label_text(text, classes):
    """(rows [n,7] float64 (l, h, w, x, y, z, rot_y), alpha [n] float64) of the lines whose type is in ``classes``:
    the lifter pairs' parser (csv_read_annot, car_instance.py:792-829) with its alpha column."""
    return lp.parse_label_text(text, classes, with_alpha=True)


def image_size(path):
    """(width, height) from the image header, without decoding the pixels (get_img_size, car_instance.py:894-900)."""
    from PIL import Image
    with Image.open(path) as image:
        return image.size


def canonical_cuboid(l, h, w, coef):
    """[n,J,3] float64: construct_box_3d + interpolate 'bbox12' (car_instance.py:730-747, 724-728) for n labels."""
    l, h, w = (np.asarray(v, dtype=np.float64) for v in (l, h, w))
    z = np.zeros_like(l)
    x = np.stack([0.5 * l, l, l, l, l, z, z, z, z], axis=1) + (-(l.astype(np.float32) / np.float32(2)))[:, None]
    y = np.stack([0.5 * h, z, h, z, h, z, h, z, h], axis=1) + (-h.astype(np.float32))[:, None]
    zz = np.stack([0.5 * w, w, w, z, z, w, w, z, z], axis=1) + (-(w.astype(np.float32) / np.float32(2)))[:, None]
    box = np.stack([x, y, zz], axis=2)                               # [n,9,3]
    corners = box[:, 1:]
    parents, children = corners[:, list(EDGE_PARENT)], corners[:, list(EDGE_CHILD)]
    lines = children - parents
    return np.concatenate([box] + [parents + c * lines for c in coef], axis=1)


class PoseAnnotBuilder(object):
    """``builder(records)`` -> ``{'paths', 'boxes', 'rots', 'kpts', 'raw_kpts'}``, each a list with one entry per kept
    frame: ``boxes [n,4]`` int64, ``rots [n,2]``, ``kpts [n,J,2]``, ``raw_kpts [m,J,3]`` float64 (the reference's
    ``annot_2dpose``).  Frames whose instances are all dropped are skipped (car_instance.py:334-335).

    A record is ``{'path': str, 'labels_text' | 'label_path', 'calib_text' | 'calib_path', 'size': (width, height)}``;
    without ``'size'`` it is read from the header of the image at ``'path'``.  ``min_visible`` is the reference's
    ``threshold`` (4): with 33 or 21 points the 30 % filter already asks for more, so only a larger value drops
    anything.  ``last_counts`` holds the instance counts of the last call; ``last_src`` the label index (in record
    order) of every kept instance, per kept frame."""

    def __init__(self, cfgs, split='train', device=None, min_visible=MIN_VISIBLE):
        ds = cfgs['dataset']
        for key in ('2d_kpt_style', '3d_kpt_sample_style'):
            style = ds.get(key, 'bbox9')
            if style != 'bbox9':
                raise NotImplementedError('%s %r: the reference builds the 9-point cuboid only '
                                          '(car_instance.py:734-736)' % (key, style))
        interp = ds.get('interpolate') or {}
        if not interp.get('flag', True):
            raise NotImplementedError('interpolate.flag false: 9-point rows (car_instance.py:741) are not built')
        if interp.get('style', 'bbox12') != 'bbox12':
            raise NotImplementedError('interpolate.style %r: the size-aware styles are unreachable in the reference '
                                      '(car_instance.py:745, dimension= is commented out)' % (interp.get('style'),))
        self.coef = [float(c) for c in interp.get('coef', [0.332, 0.667])]
        if len(self.coef) not in (1, 2):
            raise NotImplementedError('interpolate.coef with %d entries (1 or 2; car_instance.py:727)' % len(self.coef))
        self.enlarge = float(ds.get('enlarge_factor', 1.1))             # car_instance.py:267-270
        self.classes = tuple(ds.get('detect_classes', ['Car']))
        self.num_joints = 9 + 12 * len(self.coef)
        self.min_visible = int(min_visible)      # the ``threshold`` of _prepare_2d_pose_annot (car_instance.py:304)
        self.split = split
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else 'cpu'
        self.device = torch.device(device)
        self.last_counts = None
        self.last_src = None

    # -- host: text -> arrays -----------------------------------------------------------------------------------
    def gather(self, records):
        """(labels [A,7] f64, alpha [A] f64, label_frame [A] int32, frames [F,14] f64, paths) in record order."""
        labels, alpha, lf, frames, paths = [], [], [], [], []
        for f, rec in enumerate(records):
            if 'labels_text' in rec:
                text = rec['labels_text']
            else:
                with open(rec['label_path'], 'r') as fh:
                    text = fh.read()
            lab, al = parse_label_text(text, self.classes)
            P = lp.parse_calib_text(rec['calib_text']) if 'calib_text' in rec else lp.read_calib_file(rec['calib_path'])
            size = rec['size'] if rec.get('size') is not None else image_size(rec['path'])
            frames.append(lp.frame_row(P, size))
            labels.append(lab)
            alpha.append(al)
            lf.append(np.full(len(lab), f, dtype=np.int32))
            paths.append(rec['path'])
        if not frames:
            return np.zeros((0, 7)), np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros((0, 14)), paths
        return np.concatenate(labels), np.concatenate(alpha), np.concatenate(lf), np.stack(frames), paths

    # -- the two builds: flat arrays in label order --------------------------------------------------------------
    def build_host(self, labels, alpha, label_frame, frames):
        """numpy float64, the operation order of csrc/pose_annot.hip.  Returns the dict ``build_device`` returns."""
        A, F, J = len(labels), len(frames), self.num_joints
        if A == 0:
            return self._empty(F)
        labels = np.asarray(labels, dtype=np.float64)
        Fm = np.asarray(frames, dtype=np.float64)[label_frame]             # [A,14]
        p = canonical_cuboid(labels[:, 0], labels[:, 1], labels[:, 2], self.coef)
        cs, sn = np.cos(labels[:, 6])[:, None], np.sin(labels[:, 6])[:, None]
        x = cs * p[..., 0] + sn * p[..., 2]
        y = p[..., 1]
        z = -sn * p[..., 0] + cs * p[..., 2]
        x = (x + labels[:, 3:4]) + Fm[:, 9:10]
        y = (y + labels[:, 4:5]) + Fm[:, 10:11]
        z = (z + labels[:, 5:6]) + Fm[:, 11:12]
        with np.errstate(divide='ignore', invalid='ignore'):
            pw = Fm[:, 6:7] * x + Fm[:, 7:8] * y + Fm[:, 8:9] * z
            u = (Fm[:, 0:1] * x + Fm[:, 1:2] * y + Fm[:, 2:3] * z) / pw
            v = (Fm[:, 3:4] * x + Fm[:, 4:5] * y + Fm[:, 5:6] * z) / pw
        vis = (u > 0.0) & (u < Fm[:, 12:13]) & (v > 0.0) & (v < Fm[:, 13:14])
        cnt = vis.sum(axis=1)
        raw = cnt / float(J) >= INLIER_SHARE
        kept = raw & (cnt >= self.min_visible)
        uv = np.stack([u, v], axis=2)
        k = uv[kept]
        mn, mx = k.min(axis=1), k.max(axis=1)
        center = (mn + mx) / 2
        half = (mx - mn) * self.enlarge / 2
        corners = np.concatenate([center - half, center + half], axis=1)
        boxes = np.trunc(np.clip(np.nan_to_num(corners, nan=0.0), -2147483648.0, 2147483647.0)).astype(np.int32)
        return {'raw_kpts': np.concatenate([uv, vis[..., None].astype(np.float64)], axis=2)[raw],
                'kpts': k, 'boxes': boxes, 'rots': np.stack([alpha, labels[:, 6]], axis=1)[kept],
                'src': np.nonzero(kept)[0].astype(np.int32),
                'frame_raw': np.bincount(label_frame[raw], minlength=F).astype(np.int32),
                'frame_kept': np.bincount(label_frame[kept], minlength=F).astype(np.int32),
                'totals': np.array([raw.sum(), kept.sum()], dtype=np.int64)}

    def _empty(self, F):
        J = self.num_joints
        return {'raw_kpts': np.zeros((0, J, 3)), 'kpts': np.zeros((0, J, 2)), 'boxes': np.zeros((0, 4), dtype=np.int32),
                'rots': np.zeros((0, 2)), 'src': np.zeros(0, dtype=np.int32), 'frame_raw': np.zeros(F, dtype=np.int32),
                'frame_kept': np.zeros(F, dtype=np.int32), 'totals': np.zeros(2, dtype=np.int64)}

    def launch(self, labels_d, alpha_d, label_frame_d, frames_d, ws=None):
        """One call of ``egn_pose2d_annot_f64`` on device inputs, on the current stream; no read-back.  Returns the
        device outputs sized for all labels (the first ``totals`` rows of each are written)."""
        A, F, J = int(labels_d.shape[0]), int(frames_d.shape[0]), self.num_joints
        dev = labels_d.device
        L = _lib.lib()
        nb = L.egn_pose2d_annot_ws_bytes(A)
        if nb < 0:
            raise ValueError('%d labels in one build' % A)
        with torch.cuda.device(dev):
            if ws is None:
                ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            out = {'raw_kpts': torch.empty(A, J, 3, dtype=torch.float64, device=dev),
                   'kpts': torch.empty(A, J, 2, dtype=torch.float64, device=dev),
                   'boxes': torch.empty(A, 4, dtype=torch.int32, device=dev),
                   'rots': torch.empty(A, 2, dtype=torch.float64, device=dev),
                   'src': torch.empty(A, dtype=torch.int32, device=dev),
                   'frame_raw': torch.empty(F, dtype=torch.int32, device=dev),
                   'frame_kept': torch.empty(F, dtype=torch.int32, device=dev),
                   'totals': torch.empty(2, dtype=torch.int64, device=dev), 'ws': ws}
            c1 = self.coef[1] if len(self.coef) > 1 else 0.0

            def p(t):
                return _lib.ptr(t) if t.numel() else None
            _lib.check(L.egn_pose2d_annot_f64(p(labels_d), p(alpha_d), p(label_frame_d), A, p(frames_d), F,
                                              self.coef[0], c1, J, INLIER_SHARE, self.min_visible, self.enlarge,
                                              _lib.ptr(ws), ws.numel(), p(out['raw_kpts']), p(out['kpts']),
                                              p(out['boxes']), p(out['rots']), p(out['src']), p(out['frame_raw']),
                                              p(out['frame_kept']), _lib.ptr(out['totals']),
                                              _lib.current_stream(dev)), 'pose annotations')
        return out

    def build_device(self, labels, alpha, label_frame, frames):
        dev = self.device
        with torch.cuda.device(dev):
            up = [torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
                  for a, dt in ((labels, np.float64), (alpha, np.float64), (label_frame, np.int32),
                                (frames, np.float64))]
            out = self.launch(*up)
            n_raw, n = (int(v) for v in out['totals'].cpu().numpy())          # the read-back that sizes the rest
            res = {'raw_kpts': out['raw_kpts'][:n_raw].cpu().numpy()}
            for key in ('kpts', 'boxes', 'rots', 'src'):
                res[key] = out[key][:n].cpu().numpy()
            for key in ('frame_raw', 'frame_kept'):
                res[key] = out[key].cpu().numpy()
            res['totals'] = np.array([n_raw, n], dtype=np.int64)
        return res

    def build(self, labels, alpha, label_frame, frames):
        label_frame = np.asarray(label_frame, dtype=np.int32)
        A = len(labels)
        if len(label_frame) != A or len(alpha) != A or \
                (A and (label_frame.min() < 0 or label_frame.max() >= len(frames))):
            raise ValueError('alpha and label_frame must hold one entry per label, label_frame an index into the %d '
                             'frames' % len(frames))
        if self.device.type == 'cuda':
            res = self.build_device(labels, alpha, label_frame, frames)
        else:
            res = self.build_host(labels, alpha, label_frame, frames)
        if not np.isfinite(res['kpts']).all():
            # the reference's int() raises on such a corner (a point on the camera plane)
            raise ValueError('a kept instance has a key point without a finite projection')
        return res

    # -- flat arrays -> the reference's per-frame lists -----------------------------------------------------------
    def __call__(self, records):
        labels, alpha, lf, frames, paths = self.gather(records)
        res = self.build(labels, alpha, lf, frames)
        raw_end, kept_end = np.cumsum(res['frame_raw']), np.cumsum(res['frame_kept'])
        annot = {'paths': [], 'boxes': [], 'rots': [], 'kpts': [], 'raw_kpts': []}
        src = []
        for f, path in enumerate(paths):
            n = int(res['frame_kept'][f])
            if n == 0:
                continue
            k0, r0 = int(kept_end[f]) - n, int(raw_end[f]) - int(res['frame_raw'][f])
            annot['paths'].append(path)
            annot['boxes'].append(res['boxes'][k0:k0 + n].astype(np.int64))
            annot['rots'].append(res['rots'][k0:k0 + n])
            annot['kpts'].append(res['kpts'][k0:k0 + n])
            annot['raw_kpts'].append(res['raw_kpts'][r0:int(raw_end[f])])
            src.append(res['src'][k0:k0 + n])
        n_raw, n_kept = (int(v) for v in res['totals'])
        self.last_src = src
        self.last_counts = {'frames': len(paths), 'frames_kept': len(annot['paths']), 'labels': int(len(labels)),
                            'kept_inlier': n_raw, 'dropped_inlier': int(len(labels)) - n_raw,
                            'kept_visible': n_kept, 'dropped_visible': n_raw - n_kept}
        return annot


class PoseFrames(torch.utils.data.Dataset):
    """One record per kept frame of ``annotations`` in the form ``TrainSampleBuilder`` documents: ``image`` decoded
    here (in the ``DataLoader`` worker) by ``crop_gpu.load_rgb``, ``boxes [n,4]``, ``joints [n,J,2]`` (no visibility
    column: all visible, car_instance.py:1278-1279), ``path``, and -- when the annotations hold them -- ``rots [n,2]``
    (``alpha``, ``rot_y``: the angle baselines' targets, car_instance.py:1250).  Use it with
    ``train_samples.collate_frames``."""

    def __init__(self, annotations):
        self.paths = list(annotations['paths'])
        self.boxes = list(annotations['boxes'])
        self.joints = list(annotations['kpts'])
        self.rots = list(annotations['rots']) if 'rots' in annotations else None
        if not (len(self.paths) == len(self.boxes) == len(self.joints)) or \
                (self.rots is not None and len(self.rots) != len(self.paths)):
            raise ValueError('paths, boxes, kpts and rots must have one entry per frame')
        self.num_joints = int(self.joints[0].shape[1]) if self.joints else 0

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from . import crop_gpu
        rec = {'image': crop_gpu.load_rgb(self.paths[i]), 'boxes': self.boxes[i], 'joints': self.joints[i],
               'path': self.paths[i]}
        if self.rots is not None:
            rec['rots'] = self.rots[i]
        return rec


def kitti_records(root, stems=None):
    """Records of a KITTI tree ``root`` with ``image_2``, ``label_2`` and ``calib``; ``stems`` (frame names without
    extension) default to every label file.  The size is left to the image header."""
    if stems is None:
        stems = sorted(os.path.splitext(n)[0] for n in os.listdir(os.path.join(root, 'label_2')) if n.endswith('.txt'))
    return [{'path': os.path.join(root, 'image_2', s + '.png'), 'label_path': os.path.join(root, 'label_2', s + '.txt'),
             'calib_path': os.path.join(root, 'calib', s + '.txt')} for s in stems]
