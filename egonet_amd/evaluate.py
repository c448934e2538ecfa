"""KITTI object evaluation: 2D AP / AOS, bird's-eye-view AP and 3D AP (csrc/kitti_eval.cpp on the host,
csrc/kitti_eval.hip on the GPU; the three blocks of the reference's
``tools/kitti-eval/evaluate_object_3d_offline.cpp`` without Boost).

    res = evaluate_kitti(gt_dir, result_dir)    # result_dir/data/%06d.txt as written by
    res['car']['AP_3d']                         # EgoNet.post_process(save_dict=...)
    -> [easy, moderate, hard] in percent (11-point summary, evaluate...cpp:720-724)

    res = evaluate_frames(gt_frames, det_frames)        # the same on parsed arrays, no files
    res = evaluate_aos(gt_dir, result_dir)              # the IMAGE block alone, host code
"""
import ctypes as C

import numpy as np

from . import _lib

CLASSES = ('car', 'pedestrian', 'cyclist')
LEVELS = ('easy', 'moderate', 'hard')
METRICS = ('image', 'ground', '3d')
TYPE_CODES = {'car': 0, 'pedestrian': 1, 'cyclist': 2, 'van': 3, 'person_sitting': 4, 'dontcare': 5}
_PRECISION_KEY = {'image': 'precision', 'ground': 'precision_ground', '3d': 'precision_3d'}
_SUMMARY_KEY = {'image': 'AP', 'ground': 'AP_bev', '3d': 'AP_3d'}


def evaluate_aos(gt_dir, result_dir):
    L = _lib.lib()
    prec = np.zeros((3, 3, 41), dtype=np.float64)
    aos = np.zeros((3, 3, 41), dtype=np.float64)
    evaluated = (C.c_int * 3)()
    n_frames, aos_valid = C.c_int(0), C.c_int(0)
    rc = L.egn_kitti_eval_image(str(gt_dir).encode(), str(result_dir).encode(), C.byref(n_frames), evaluated,
                                C.byref(aos_valid), prec.ctypes.data_as(C.POINTER(C.c_double)),
                                aos.ctypes.data_as(C.POINTER(C.c_double)))
    if rc == -2:
        raise FileNotFoundError('a result file has no ground-truth file in %s' % gt_dir)
    if rc == -3:
        raise FileNotFoundError('no result files under %s/data' % result_dir)
    if rc != 0:
        raise ValueError('egn_kitti_eval_image: code %d' % rc)
    out = {'n_frames': n_frames.value, 'aos_valid': bool(aos_valid.value)}
    for c, name in enumerate(CLASSES):
        if not evaluated[c]:
            continue
        out[name] = {'precision': prec[c].copy(), 'aos': aos[c].copy() if aos_valid.value else None,
                     'AP': [float(prec[c, l, ::4].sum() / 11 * 100) for l in range(3)],
                     'AOS': [float(aos[c, l, ::4].sum() / 11 * 100) for l in range(3)] if aos_valid.value else None}
    return out


def _on_gpu(device):
    """device None: the GPU when one is visible, else the host path; 'cpu' forces the host path; anything else names
    the GPU to run on (a missing one is an error, not a reason to fall back)."""
    import torch
    if device is None:
        return torch.cuda.is_available(), None
    dev = torch.device(device)
    if dev.type == 'cpu':
        return False, None
    if not torch.cuda.is_available():
        raise _lib.EgonetHipError('evaluate: device %r asked for and no GPU is visible' % (device,))
    return True, dev


def _mask(metrics):
    bad = [m for m in metrics if m not in METRICS]
    if bad or not metrics:
        raise ValueError('metrics: a non-empty subset of %r, got %r' % (METRICS, tuple(metrics)))
    return sum(1 << METRICS.index(m) for m in set(metrics))


class _Out:
    def __init__(self):
        self.evaluated = np.zeros((3, 3), dtype=np.int32)
        self.aos_valid = C.c_int(0)
        self.n_frames = C.c_int(0)
        self.precision = np.zeros((3, 3, 3, 41), dtype=np.float64)
        self.aos = np.zeros((3, 3, 41), dtype=np.float64)
        self.counts = np.zeros((3, 3, 3, 41, 3), dtype=np.int32)
        self.n_thresholds = np.zeros((3, 3, 3), dtype=np.int32)

    def args(self):
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        return [self.evaluated.ctypes.data_as(ip), C.byref(self.aos_valid), self.precision.ctypes.data_as(dp),
                self.aos.ctypes.data_as(dp), self.counts.ctypes.data_as(ip), self.n_thresholds.ctypes.data_as(ip)]

    def result(self, n_frames):
        valid = bool(self.aos_valid.value)
        out = {'n_frames': n_frames, 'aos_valid': valid}
        for c, name in enumerate(CLASSES):
            if not self.evaluated[:, c].any():
                continue
            r = {'counts': {}, 'n_thresholds': {}}
            for m, metric in enumerate(METRICS):
                if not self.evaluated[m, c]:
                    continue                                      # a class not scored in a metric has no key for it
                p = self.precision[m, c].copy()
                r[_PRECISION_KEY[metric]] = p
                r[_SUMMARY_KEY[metric]] = [float(p[l, ::4].sum() / 11 * 100) for l in range(3)]
                r['counts'][metric] = self.counts[m, c].copy()
                r['n_thresholds'][metric] = self.n_thresholds[m, c].copy()
                if m == 0:
                    a = self.aos[c]
                    r['aos'] = a.copy() if valid else None
                    r['AOS'] = [float(a[l, ::4].sum() / 11 * 100) for l in range(3)] if valid else None
            out[name] = r
        return out


def _raise(rc, what, gt_dir=None, result_dir=None):
    if rc == -2:
        raise FileNotFoundError('a result file has no ground-truth file in %s' % gt_dir)
    if rc == -3:
        raise FileNotFoundError('no result files under %s/data' % result_dir)
    _lib.check(rc, what)


def evaluate_kitti(gt_dir, result_dir, metrics=METRICS, device=None):
    """All three metrics of the reference evaluator on label / result directories.

    Per class: today's ``precision`` / ``aos`` / ``AP`` / ``AOS`` (IMAGE) plus ``precision_ground`` / ``AP_bev``
    and ``precision_3d`` / ``AP_3d``, ``counts[metric]`` ([3 levels][41][tp, fp, fn]) and ``n_thresholds[metric]``;
    a class that is not scored in a metric has no key for it."""
    L = _lib.lib()
    mask = _mask(metrics)
    gpu, dev = _on_gpu(device)
    o = _Out()
    head = [str(gt_dir).encode(), str(result_dir).encode(), mask, C.byref(o.n_frames)]
    if gpu:
        import torch
        with torch.cuda.device(dev):
            rc = L.egn_kitti_eval_dirs_dev(*(head + o.args() + [_lib.current_stream()]))
    else:
        rc = L.egn_kitti_eval_dirs_host(*(head + o.args()))
    _raise(rc, 'egn_kitti_eval_dirs', gt_dir, result_dir)
    return o.result(o.n_frames.value)


def _pack(frames, with_score):
    off, box, types, trunc, occ, score = [0], [], [], [], [], []
    for fr in frames:
        names = list(fr['type'])
        n = len(names)
        off.append(off[-1] + n)
        if n == 0:
            continue
        b = np.empty((n, 12), dtype=np.float64)
        b[:, 0:4] = np.asarray(fr['bbox'], dtype=np.float64).reshape(n, 4)
        b[:, 4] = np.asarray(fr['alpha'], dtype=np.float64).reshape(n)
        b[:, 5:8] = np.asarray(fr['dimensions'], dtype=np.float64).reshape(n, 3)        # h w l
        b[:, 8:11] = np.asarray(fr['location'], dtype=np.float64).reshape(n, 3)
        b[:, 11] = np.asarray(fr['rotation_y'], dtype=np.float64).reshape(n)
        box.append(b)
        types += [TYPE_CODES.get(str(t).lower(), 6) for t in names]
        if with_score:
            score.append(np.asarray(fr['score'], dtype=np.float64).reshape(n))
        else:
            trunc.append(np.asarray(fr['truncation'], dtype=np.float64).reshape(n))
            occ.append(np.asarray(fr['occlusion']).reshape(n).astype(np.int32))
    cat = lambda parts, dt, tail=(): (np.ascontiguousarray(np.concatenate(parts), dtype=dt) if parts     # noqa: E731
                                      else np.zeros((0,) + tail, dtype=dt))
    return (np.asarray(off, dtype=np.int32), cat(box, np.float64, (12,)), np.asarray(types, dtype=np.int32),
            cat(score if with_score else trunc, np.float64), cat(occ, np.int32))


def evaluate_frames(gt_frames, det_frames, metrics=METRICS, device=None):
    """``evaluate_kitti`` on parsed frames, without files.  A frame is a dict of per-object arrays: ``type`` (names),
    ``truncation``, ``occlusion``, ``alpha``, ``bbox`` [n, 4], ``dimensions`` [n, 3] (h w l), ``location`` [n, 3],
    ``rotation_y``, and ``score`` for detections (which need no truncation / occlusion)."""
    if len(gt_frames) != len(det_frames):
        raise ValueError('evaluate_frames: %d ground-truth frames, %d detection frames' % (len(gt_frames), len(det_frames)))
    L = _lib.lib()
    mask = _mask(metrics)
    gpu, dev = _on_gpu(device)
    g_off, g_box, g_type, g_trunc, g_occ = _pack(gt_frames, False)
    d_off, d_box, d_type, d_score, _ = _pack(det_frames, True)
    o = _Out()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                                          # noqa: E731
    head = [len(gt_frames), vp(g_off), vp(d_off), vp(g_box), vp(g_type), vp(g_trunc), vp(g_occ), vp(d_box), vp(d_type),
            vp(d_score), mask]
    if gpu:
        import torch
        with torch.cuda.device(dev):
            rc = L.egn_kitti_eval_packed_dev(*(head + o.args() + [_lib.current_stream()]))
    else:
        rc = L.egn_kitti_eval_packed_host(*(head + o.args()))
    _raise(rc, 'egn_kitti_eval_packed')
    return o.result(len(gt_frames))
