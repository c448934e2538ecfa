"""Training-sample front end: decoded frames + boxes + key points -> the HRNet training batch
``(images, targets, target_weights, meta)`` that ``trainer.train`` consumes.

It reproduces the reference's ``instanceto2d`` dataset (libs/dataset/KITTI/car_instance.py:1272-1299 ->
libs/common/img_proc.py:213-345) followed by ``my_collate_fn`` / ``length_limit`` (car_instance.py:1344-1391):
per box an optional jitter (four draws of the global ``np.random``), ``resize_bbox`` to the input aspect
ratio, the three-point ``get_affine_transform``, ``cv2.warpAffine`` + ToTensor + Normalize, the visible joints
moved into the crop and one Gaussian heat-map per joint (``generate_target``); then a random subset of
``MAX_INS_CNT`` instances when the batch holds more.

Split of work.  The per-box math (4 draws, one resize, one 3x3 solve, 33 two-by-three products) stays on the
host in float64, vectorised over the batch, with the reference's operation order: the same seed gives the same
boxes, affines and subset.  What is heavy runs on the device: the uint8 frames go up once, one launch of
``egn_crop_frames_warp_normalize_u8`` cuts the crops of every kept box of every frame, one launch of
``egn_gaussian_targets_f32`` draws all maps.  ``meta`` is host numpy, computed before the upload, so reading it
needs no device synchronisation.

Upload.  Frames, the frame table, the per-box frame index, the affines, joints and visibilities go up as the
sections of ONE pinned, double-buffered, event-guarded ``non_blocking`` copy on the current stream
(common/staging.py); the kernels and the training step that follow run on that stream.

Decode stays in the ``DataLoader`` workers: a Dataset returns records (see ``INTEGRATION.md``), ``collate_frames``
keeps them as a list, ``TrainSampleBuilder`` turns the list into the batch.

Mixed batches (``cfgs['ss']['flag']``, car_instance.py:1145-1169, 1292-1298, 1353-1380): every labelled frame with
fewer than ``ss.max_per_img`` instances brings crops of one unlabelled frame -- same jitter, resize, affine, warp and
normalisation, no targets and no meta.  The batch holds the ``n_fs`` labelled crops first, then the unlabelled ones;
targets, weights and meta keep ``n_fs`` rows and ``meta['fs_instance_cnt'] = n_fs``.  The unlabelled frames join the
frame table of the one upload and the one crop launch.  ``MixedFrames`` chooses and decodes them in the workers.
"""
import os
import time

import numpy as np
import torch

from .. import _lib
from . import crop_gpu, staging

MAX_INS_CNT = 140              # car_instance.py:33
TARGETS = {'heatmap': None, 'alpha': 0, 'theta': 1}       # the column of a record's ``rots`` an angle mode regresses
EXP_TARGETS = {'baselinealpha': 'alpha', 'baselinetheta': 'theta'}      # cfgs['exp_type'], car_instance.py:1248
SIZE = 200.0


def collate_frames(batch):
    """DataLoader ``collate_fn``: the records of a batch, kept as a list (decoded frames stay uint8 on the host)."""
    return list(batch)


def _hm_value(hm, key, default):
    return hm[key] if key in hm and hm[key] is not None else default


class TrainSampleBuilder(object):
    """``builder(records, rng=np.random)`` -> ``(images [N,3,h,w], targets [N,K,hm_h,hm_w], target_weights [N,K,1],
    meta)``, the first three CUDA fp32, ``meta`` host numpy with the reference's keys.

    A record is ``{'image': [H,W,3] uint8 RGB, 'boxes': [n,4], 'joints': [n,K,2|3], 'path': str}`` (the fields
    ``annot_2dpose`` holds for ``instanceto2d``); a missing visibility column means 1 (car_instance.py:1278-1279).

    ``target``: 'heatmap' (the above), or 'alpha' / 'theta' -- the direct-regression baselines (car_instance.py:
    1248-1271, ``generate_hm=False``); None reads ``cfgs['exp_type']`` ('baselinealpha' / 'baselinetheta', anything else
    means 'heatmap').  In the angle modes every record also holds ``'rots': [n,2]`` (``alpha``, ``rot_y``) and the batch
    is ``(images, targets [N,2] = float32([cos r, sin r]) on the device, torch.ones(1), meta)`` with
    ``meta['angles_gt'] [N]`` float64; no heat-map launch is made.

    ``cfgs['ss']`` (``flag``, ``max_per_img``) switches the mixed batches on for split 'train' in the heat-map mode (the
    angle modes ignore it, like the reference's ``__getitem__``, car_instance.py:1248-1271).  The unlabelled frame of a
    labelled record with fewer than ``max_per_img`` boxes is either the record's own ``'ss'`` entry ``{'image',
    'boxes', 'path'}`` (chosen and decoded ahead, ``MixedFrames``: no draw here) or one of ``builder(records, rng,
    unlabelled=pool)``, picked by ``rng.randint(0, len(pool))`` as ``extract_ss_sample`` does.  The batch is then
    ``(images [N,3,h,w], targets [n_fs,K,hm_h,hm_w], target_weights [n_fs,K,1], meta)`` with ``n_fs <= N``.

    Draw order on ``rng``, per frame of the batch (car_instance.py:1283-1294, img_proc.py:174-191, 302-308): four
    ``rand()`` per labelled box (jitter on); then, where ``max_per_img`` exceeds the frame's box count, the ``randint``
    (pool mode) and four ``rand()`` for EVERY box of the unlabelled frame -- it is cropped whole and cut to the first
    ``max_per_img - n`` crops afterwards (img_proc.py:325-339).  After all frames the ``length_limit`` choice."""

    def __init__(self, cfgs, split='train', device=None, target=None):
        hm = cfgs['heatmapModel']
        if target is None:
            target = EXP_TARGETS.get(cfgs.get('exp_type'), 'heatmap')
        if target not in TARGETS:
            raise ValueError('target %r (one of %s)' % (target, ', '.join(sorted(TARGETS))))
        self.target, self.rot_col = target, TARGETS[target]
        if _hm_value(hm, 'target_type', 'gaussian') != 'gaussian':
            raise NotImplementedError('target_type %r: the reference draws gaussian targets only '
                                      '(img_proc.py:368)' % hm['target_type'])
        if hm.get('use_different_joints_weight'):
            raise NotImplementedError('use_different_joints_weight: the reference never sets hm_para["joints_weight"] '
                                      '(car_instance.py:499-519) and raises KeyError in generate_target')
        if hm.get('add_xy'):
            raise NotImplementedError('add_xy: 5-channel inputs (img_proc.py:232-234) are not built by this front end')
        norm = (cfgs.get('dataset', {}) or {}).get('pth_transform') or {}
        self.mean = tuple(float(v) for v in norm.get('mean', crop_gpu.IMAGENET_MEAN))
        self.std = tuple(float(v) for v in norm.get('std', crop_gpu.IMAGENET_STD))
        if len(self.mean) != 3 or len(self.std) != 3:
            raise ValueError('pth_transform mean/std must have 3 entries (RGB), got %d / %d'
                             % (len(self.mean), len(self.std)))
        # the reference's hm_para holds sizes as (height, width) (car_instance.py:506-509)
        self.input_hw = (int(hm['input_size'][1]), int(hm['input_size'][0]))
        self.heatmap_hw = (int(hm['heatmap_size'][1]), int(hm['heatmap_size'][0]))
        self.num_joints = int(hm['num_joints'])
        self.sigma = float(_hm_value(hm, 'sigma', 1))
        self.jitter = bool(hm.get('jitter_bbox', False)) and split == 'train' and bool(cfgs.get('train', False))
        self.scaling = tuple(hm['jitter_params']['scaling']) if self.jitter else None
        ss = cfgs.get('ss') or {}
        self.mix = bool(ss.get('flag', False)) and split == 'train' and self.rot_col is None
        self.max_per_img = int(ss.get('max_per_img', 0)) if self.mix else 0
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self._staging = staging.PinnedStaging(1 << 20)
        # True: every call keeps {'host_ms', 'events'} in last_timings -- four timing events: before the upload,
        # after it, after the crop launch, after the targets launch (tools/train_samples_bench.py reads them after a synchronise)
        self.record_timings = False
        self.last_timings = None

    # -- host math (float64, vectorised over the batch) -------------------------------------------------------
    def gather(self, records):
        """(boxes [N,4] f64, joints [N,K,3] f64, frame index [N] int64) of all boxes in record order."""
        boxes, joints, frame = [], [], []
        for f, rec in enumerate(records):
            b = np.asarray(rec['boxes'], dtype=np.float64).reshape(-1, 4)
            j = np.asarray(rec['joints'], dtype=np.float64)
            if j.ndim != 3 or len(j) != len(b) or j.shape[2] not in (2, 3):
                raise ValueError('record %d: joints must be [n,K,2|3] for its %d boxes, got %s'
                                 % (f, len(b), j.shape))
            if j.shape[2] == 2:
                j = np.concatenate([j, np.ones(j.shape[:2] + (1,))], axis=2)
            boxes.append(b)
            joints.append(j)
            frame.append(np.full(len(b), f, dtype=np.int64))
        if not boxes or sum(len(b) for b in boxes) == 0:
            raise ValueError('the batch holds no box')
        joints = np.concatenate(joints)
        if joints.shape[1] != self.num_joints:
            raise ValueError('joints have %d key points, heatmapModel.num_joints is %d'
                             % (joints.shape[1], self.num_joints))
        return np.concatenate(boxes), joints, np.concatenate(frame)

    def gather_rots(self, records, n_all):
        """The regressed angle [N] f64 of all boxes in record order (column ``rot_col`` of every record's ``rots``)."""
        rots = []
        for f, rec in enumerate(records):
            if 'rots' not in rec:
                raise ValueError("record %d has no 'rots': target %r needs [n,2] (alpha, rot_y) per frame"
                                 % (f, self.target))
            rots.append(np.asarray(rec['rots'], dtype=np.float64).reshape(-1, 2)[:, self.rot_col])
        rots = np.concatenate(rots)
        if len(rots) != n_all:
            raise ValueError('%d rots for %d boxes' % (len(rots), n_all))
        return rots

    def jitter_boxes(self, boxes, draws):
        """jitter_bbox_with_kpts_no_occlu (img_proc.py:174-191); draws [N,4] = the four rand() of each box."""
        width, height = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
        cx, cy = 0.5 * (boxes[:, 0] + boxes[:, 2]), 0.5 * (boxes[:, 1] + boxes[:, 3])
        sx = self.scaling[0] * draws[:, 0] + 1
        sy = self.scaling[1] * draws[:, 1] + 1
        shift_x = 0.5 * (sx - 1) * width * (draws[:, 2] * 2 - 1)
        shift_y = 0.5 * (sy - 1) * height * (draws[:, 3] * 2 - 1)
        ncx, ncy = cx + shift_x, cy + shift_y
        nw, nh = width * sx, height * sy
        return np.stack([ncx - 0.5 * nw, ncy - 0.5 * nh, ncx + 0.5 * nw, ncy + 0.5 * nh], axis=1)

    def resize_boxes(self, boxes):
        """resize_bbox (img_proc.py:411-435) to target_ar = input h / input w -> (c [N,2], s [N,2])."""
        h, w = self.input_hw
        target_ar = np.float64(h) / np.float64(w)
        left, top, right, bottom = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
        width, height = right - left, bottom - top
        cx, cy = (left + right) / 2, (top + bottom) / 2
        wide = height / width > target_ar
        new_w = height * (1 / target_ar)
        new_h = width * target_ar
        nl = np.where(wide, cx - 0.5 * new_w, left)
        nr = np.where(wide, cx + 0.5 * new_w, right)
        nt = np.where(wide, top, cy - 0.5 * new_h)
        nb = np.where(wide, bottom, cy + 0.5 * new_h)
        return np.stack([cx, cy], axis=1), np.stack([(nr - nl) / SIZE, (nb - nt) / SIZE], axis=1)

    def affines(self, c, s):
        """get_affine_transform(c, s, 0, (h, w)) of every box (img_proc.py:26-64) -> [N,2,3] f64: the float32
        three-point construction, solved exactly like cv2.getAffineTransform."""
        h, w = self.input_hw
        n = len(c)
        src = np.zeros((n, 3, 2), dtype=np.float32)
        src[:, 0] = c
        src[:, 1, 0] = c[:, 0]
        src[:, 1, 1] = c[:, 1] + s[:, 0] * SIZE * -0.5
        dst = np.zeros((3, 2), dtype=np.float32)
        dst[0] = [w * 0.5, h * 0.5]
        dst[1] = np.array([w * 0.5, h * 0.5]) + np.array([0, w * -0.5], np.float32)
        d = src[:, 0] - src[:, 1]
        src[:, 2] = src[:, 1] + np.stack([-d[:, 1], d[:, 0]], axis=1)
        dd = dst[0] - dst[1]
        dst[2] = dst[1] + np.array([-dd[1], dd[0]], dtype=np.float32)
        m = np.concatenate([src.astype(np.float64), np.ones((n, 3, 1))], axis=2)
        rhs = np.broadcast_to(dst.astype(np.float64), (n, 3, 2)).copy()
        return np.linalg.solve(m, rhs).transpose(0, 2, 1)

    @staticmethod
    def transform_joints(joints, trans):
        """Joints with vis > 0 through their box's affine (img_proc.py:240-242); the others keep image coordinates."""
        out = joints.copy()
        x, y = joints[..., 0], joints[..., 1]
        tx = trans[:, None, 0, 0] * x + trans[:, None, 0, 1] * y + trans[:, None, 0, 2]
        ty = trans[:, None, 1, 0] * x + trans[:, None, 1, 1] * y + trans[:, None, 1, 2]
        vis = joints[..., 2] > 0.0
        out[..., 0] = np.where(vis, tx, x)
        out[..., 1] = np.where(vis, ty, y)
        return out

    def plan(self, records, rng=np.random, unlabelled=None):
        """All host work of a batch, in the reference's draw order (per frame, per box: 4 draws; then the
        length_limit choice).  Returns a dict: 'kept' [n] (indices into the batch's boxes), 'frame' [n],
        'trans' [n,2,3], 'draws' [N,4] or None, and 'meta' (the reference's keys); in the angle modes also 'targets'
        [n,2] float32 and meta['angles_gt'] [n].

        Mixed batches: the batch's boxes are the labelled ones in record order followed by the kept crops of the
        unlabelled frames in frame order; 'kept', 'frame' and 'trans' cover all of them, 'n_fs' counts the labelled
        prefix, 'frame' indexes 'sources' (the records followed by the unlabelled frames), 'draws' holds every draw in
        stream order (dropped unlabelled boxes included), 'ss_idx' the ``randint`` draws and 'ss_boxes' (frame, crops
        kept) of every labelled frame that drew."""
        boxes_fs, joints, frame_fs = self.gather(records)
        n_fs = len(boxes_fs)
        counts = np.bincount(frame_fs, minlength=len(records))
        sources, where = list(records), {}
        draws_fs, draws_ss, stream, ss_idx, ss_boxes = [], [], [], [], []
        boxes_ss, frame_ss = [], []
        for f, rec in enumerate(records):
            if self.jitter:
                # (consecutive per-frame calls consume the stream exactly as one rand(n_all, 4) does)
                draws_fs.append(rng.rand(counts[f], 4))
                stream.append(draws_fs[-1])
            want = self.max_per_img - int(counts[f])
            if not self.mix or want <= 0:
                continue                                    # extract_ss_sample :1150-1153: no draw at all
            ss = rec.get('ss')
            if ss is None:
                if unlabelled is None or len(unlabelled) == 0:
                    raise ValueError("record %d has %d boxes (< ss.max_per_img = %d) and no 'ss' entry: wrap the "
                                     'frames in MixedFrames or pass unlabelled=pool' % (f, counts[f], self.max_per_img))
                ss_idx.append(int(rng.randint(0, len(unlabelled))))
                ss = unlabelled[ss_idx[-1]]
            b = np.asarray(ss['boxes'], dtype=np.float64).reshape(-1, 4)
            if self.jitter:
                d = rng.rand(len(b), 4)                       # the frame is cropped whole: every box draws
                stream.append(d)
                draws_ss.append(d[:want])
            b = b[:want]                                    # img_proc.py:325-339 (max_cnt)
            ss_boxes.append((f, len(b)))
            if not len(b):
                continue
            if id(ss) not in where:                         # a pool frame drawn twice goes up once
                where[id(ss)] = len(sources)
                sources.append(ss)
            boxes_ss.append(b)
            frame_ss.append(np.full(len(b), where[id(ss)], dtype=np.int64))
        boxes = np.concatenate([boxes_fs] + boxes_ss)
        frame = np.concatenate([frame_fs] + frame_ss)
        n_all = len(boxes)
        if self.jitter:
            boxes = self.jitter_boxes(boxes, np.concatenate(draws_fs + draws_ss))
        c, s = self.resize_boxes(boxes)
        trans = self.affines(c, s)
        tj = self.transform_joints(joints, trans[:n_fs])
        # length_limit (car_instance.py:1344-1366)
        kept, rows, counted = np.arange(n_all), np.arange(n_fs), self.mix
        if n_all > MAX_INS_CNT and (n_fs == n_all or n_fs > MAX_INS_CNT):
            # a choice among the labelled crops; in a mixed batch every unlabelled crop is dropped and the result has no
            # 'fs_instance_cnt' (:1353-1360).  (With the mix on and n_fs == n_all the reference takes :1345-1352, which
            # indexes the int 'fs_instance_cnt' and raises; the same choice is made here.)
            kept = rows = rng.choice(n_fs, MAX_INS_CNT, replace=False)
            counted = False
        elif n_all > MAX_INS_CNT:
            kept = kept[:MAX_INS_CNT]                       # :1361-1363: targets and meta untouched
        meta = {'path': [r.get('path', '') for r in records],
                'original_joints': joints[rows], 'transformed_joints': tj[rows],
                'center': c[rows], 'scale': s[rows], 'joints_vis': tj[rows][:, :, 2]}
        p = {'kept': kept, 'frame': frame[kept], 'trans': trans[kept],
             'draws': np.concatenate(stream) if stream else None, 'meta': meta}
        if self.mix:
            if counted:
                meta['fs_instance_cnt'] = n_fs
            p.update(n_fs=len(rows), sources=sources, ss_idx=ss_idx, ss_boxes=ss_boxes)
        if self.rot_col is not None:
            # car_instance.py:1264-1270: [cos r, sin r] in float64, rounded to float32 once; ``chosen`` indexes them
            # like every other meta array (length_limit :1344-1352)
            r = self.gather_rots(records, n_all)[kept]
            meta['angles_gt'] = r
            # (one scalar call per angle, as there: at most MAX_INS_CNT of them, and no array loop of numpy's can
            # round differently)
            p['targets'] = np.array([[np.cos(v), np.sin(v)] for v in r], dtype=np.float64).reshape(-1, 2) \
                .astype(np.float32)
        return p

    # -- device work ---------------------------------------------------------------------------------------------
    def pack(self, records, p):
        """The host arrays of a batch's one upload, in staging order (host only): the frames that keep a box as
        ('frame', f), the frame table [offset in the block, rows, columns, row pitch], the per-box frame index, the
        affines, then the targets' inputs."""
        n = len(p['kept'])
        records = p.get('sources', records)                 # mixed batches: the unlabelled frames follow the records
        used = np.unique(p['frame'])
        remap = np.full(len(records), -1, dtype=np.int64)
        remap[used] = np.arange(len(used))
        arrays = {}
        for f in used:
            img = records[f]['image']
            img = img.numpy() if torch.is_tensor(img) else np.asarray(img)
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                raise ValueError('record %d: image must be [H,W,3] uint8 RGB, got %s %s' % (f, img.dtype, img.shape))
            arrays['frame', f] = img
        tab = arrays['tab'] = np.empty((len(used), 4), dtype=np.int64)
        arrays['box_frame'] = remap[p['frame']].astype(np.int32)
        arrays['M'] = np.asarray(p['trans'], dtype=np.float64).reshape(n, 6)
        if self.rot_col is not None:
            arrays['angles'] = np.asarray(p['targets'], dtype=np.float32).reshape(n, 2)
        else:
            arrays['joints'] = np.asarray(p['meta']['transformed_joints'], dtype=np.float64)
            arrays['vis'] = p['meta']['joints_vis'].astype(np.float32)
        where, _ = staging.layout([(name, a.nbytes) for name, a in arrays.items()], staging.ALIGN)
        tab[:] = [[where['frame', f], arrays['frame', f].shape[0], arrays['frame', f].shape[1],
                   3 * arrays['frame', f].shape[1]] for f in used]
        return arrays

    def __call__(self, records, rng=np.random, unlabelled=None):
        t0 = time.perf_counter()
        p = self.plan(records, rng, unlabelled)
        meta, n = p['meta'], len(p['kept'])
        n_fs = p.get('n_fs', n)                             # targets are drawn for the labelled prefix only
        K = self.num_joints
        h, w = self.input_hw
        hm_h, hm_w = self.heatmap_hw
        arrays = self.pack(records, p)
        dev = self.device
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if self.record_timings else None

        def host_part_ends(stream):
            self.last_timings = {'host_ms': (time.perf_counter() - t0) * 1e3, 'events': ev}
            ev[0].record(stream)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            d, staged = self._staging.upload(arrays, dev, views=[k for k in arrays if type(k) is str],
                                             before_copy=host_part_ends if ev else None,
                                             after_copy=ev[1].record if ev else None)
            mean_t, std_t = crop_gpu._norm_consts(self.mean, self.std, dev)
            images = torch.empty(n, 3, h, w, dtype=torch.float32, device=dev)
            L = _lib.lib()
            st = _lib.current_stream(dev)
            _lib.check(L.egn_crop_frames_warp_normalize_u8(_lib.ptr(staged), _lib.ptr(d['tab']), len(arrays['tab']),
                                                           _lib.ptr(d['box_frame']), _lib.ptr(d['M']), n, h, w,
                                                           _lib.ptr(mean_t), _lib.ptr(std_t), _lib.ptr(images), st),
                       'crop frames')
            if ev:
                ev[2].record(stream)
            if self.rot_col is not None:
                # the targets came up with the staging copy; the dummy weight of my_collate_fn (car_instance.py:1388-1390)
                if ev:
                    ev[3].record(stream)
                return images, d['angles'], torch.ones(1), meta
            targets = torch.empty(n_fs, K, hm_h, hm_w, dtype=torch.float32, device=dev)
            weights = torch.empty(n_fs, K, 1, dtype=torch.float32, device=dev)
            # the reference's stride quirk (img_proc.py:376-378): input_size / heatmap_size in (h, w) order, the
            # first of them divides x -- egn_gaussian_targets_f32 takes the two strides in that order
            _lib.check(L.egn_gaussian_targets_f32(_lib.ptr(d['joints']), _lib.ptr(d['vis']), n_fs, K, hm_h, hm_w,
                                                  float(h) / float(hm_h), float(w) / float(hm_w), self.sigma,
                                                  _lib.ptr(targets), _lib.ptr(weights), st), 'gaussian targets')
            if ev:
                ev[3].record(stream)
        return images, targets, weights, meta


class MixedFrames(torch.utils.data.Dataset):
    """``frames`` (``pose_annot.PoseFrames`` or any Dataset of the builder's records) with the unlabelled frame of the
    mixed batches chosen and decoded in the ``DataLoader`` worker, as ``KITTI.extract_ss_sample`` does
    (car_instance.py:1145-1169): a record with fewer than ``max_per_img`` boxes gets ``'ss': {'image', 'boxes',
    'path'}`` -- index ``np.random.randint(0, len(paths))`` of ``ss_record``, the file with the basename of
    ``ss_record['paths'][idx]`` under ``img_root``.  ``ss_record``: the reference's dictionary (``paths``, ``boxes``;
    its ``kpts`` are not read) or the path of its ``.npy`` file."""

    def __init__(self, frames, ss_record, img_root, max_per_img):
        if isinstance(ss_record, (str, bytes, os.PathLike)):
            ss_record = np.load(ss_record, allow_pickle=True).item()      # car_instance.py:180
        self.frames, self.img_root, self.max_per_img = frames, img_root, int(max_per_img)
        self.ss_paths, self.ss_boxes = list(ss_record['paths']), list(ss_record['boxes'])
        if not self.ss_paths or len(self.ss_paths) != len(self.ss_boxes):
            raise ValueError('the unlabelled record needs one boxes entry per path, and at least one frame')
        if hasattr(frames, 'num_joints'):
            self.num_joints = frames.num_joints

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        rec = self.frames[i]
        if self.max_per_img - len(rec['boxes']) <= 0:
            return rec
        idx = np.random.randint(0, len(self.ss_paths))
        path = os.path.join(self.img_root, self.ss_paths[idx].split(os.sep)[-1])
        return dict(rec, ss={'image': crop_gpu.load_rgb(path), 'boxes': self.ss_boxes[idx], 'path': path})
