"""Validation metrics of the key-point model with the reference's names and return
values (``libs/metric/criterions.py``): ``get_distance`` :17-37, ``get_PCK`` :57-66,
``get_distance_src`` :68-143, ``get_angle_error`` :39-55, ``JointDistance2DSIP``
:173-224, ``AngleError`` :145-171.

The heat-map decode inside ``get_distance_src`` runs on the GPU (csrc/decode.hip, one
wavefront per map: hard arg-max, soft-arg-max, or the numpy-style soft-arg-max); the
rest -- 33 points per instance through a 2x3 inverse crop affine, distances, PCK
counts -- is per-instance host arithmetic in float64 like the reference's.
``JointDistance2DSIP`` with CUDA predictions and ``DistanceSrcMeter`` (the training loop's
``metric_func``) run all of it on the device instead (csrc/kpt_metrics.hip: decode, rescale,
closed-form inverse affine, distances, PCK counts, a device accumulator) and read back once.
Host ``meta`` arrays go up through common/staging.py; every device accumulator is a ``_DeviceAcc``.

``get_angle_error`` / ``AngleError`` with CUDA predictions and ``AngleErrorMeter`` (the angle baselines' ``metric_func``)
run on the device too (csrc/angle_metrics.hip: atan2 in float64, the wrapped difference, a {count, sum} accumulator).

The lifter's 3-D metrics (``RError3D`` :390-449, ``RTError3D`` :451-538, ``JointDistance3D`` :343-388,
``RotationError3D`` :303-341, ``Evaluator`` :540-573; helpers :223-301) keep the reference's constructor arguments,
attribute names (``mean_rT``, ``max_R``, ``count_R``, ... as numpy arrays) and ``report()`` text.  ``update`` takes
two kinds of input:
  CUDA tensors   csrc/lifter_metrics.hip (``egn_lifter_metrics_update_f32``): the rows stay on the device and are
                 folded into one device accumulator per metric object; with ``statistics=`` (or after
                 ``set_statistics``) the unnormalise of trainer.py:474-481 is fused into the kernel.  Nothing is read
                 back until ``report()`` or the first attribute access.
  numpy arrays   host arithmetic in float64 (the reference runs the same formulas in the arrays' float32), so the
                 classes also work without a GPU.
Out of scope, each a ``NotImplementedError``: ``T_style`` / ``style`` 'procrustes' (the reference aligns the
prediction IN PLACE, criterions.py:285-292, so the rotation error after it is that of the aligned points),
``R_style`` other than 'euler' (:266-267) and ``3d_kpt_sample_style`` other than 'bbox9' (:399-402).
"""
import functools

import numpy as np
import torch

from .. import _lib
from ..common import img_proc as lip
from ..common.staging import PinnedStaging

PCK_THRES = np.array([0.1, 0.2, 0.3])


def get_distance(gt, pred):
    """Per-joint Euclidean distances as a list; a third ground-truth column is a
    visibility flag (zero = joint skipped)."""
    gt = np.asarray(gt)
    if gt.shape[1] not in (2, 3):
        raise ValueError('Array shape not supported.')
    dist = np.sqrt(((gt[:, :2] - pred) ** 2).sum(axis=1))
    if gt.shape[1] == 3:
        dist = dist[np.nonzero(gt[:, 2])[0]]
    return list(dist)


def get_PCK(pred, gt):
    """Counts of key-points closer than PCK_THRES x (a third of the instance's vertical
    extent).  Argument order as in the reference: (prediction, ground truth)."""
    distance = np.array(get_distance(gt, pred))
    denominator = (gt[:, 1].max() - gt[:, 1].min()) / 3
    return np.array([float((distance < t * denominator).sum()) for t in PCK_THRES])


def get_angle_error(pred, meta_data, cfgs=None):
    """Mean error in degrees of predicted [cos, sin] rows against ``meta_data['angles_gt']`` (radians), the row count,
    None.  numpy arrays and CPU tensors: host arithmetic like the reference's; a CUDA prediction: csrc/angle_metrics.hip
    and one read-back of the {count, sum} pair."""
    if torch.is_tensor(pred) and pred.is_cuda:
        call = _angle_call(pred.device)
        call.update(pred, meta_data)
        return call.take()[1] / len(pred), len(pred), None
    if not isinstance(pred, np.ndarray):
        pred = pred.data.cpu().numpy()
    dif = np.abs(meta_data['angles_gt'] - np.arctan2(pred[:, 1], pred[:, 0])) * 180 / np.pi
    dif = np.where(dif > 180, 360 - dif, dif)
    return dif.sum() / len(pred), len(pred), None


@functools.lru_cache(maxsize=None)
def _angle_call(device):
    """get_angle_error's device side for CUDA predictions on ``device``: an accumulator (and a pinned staging) of its
    own, kept."""
    return _AngleMetricsDevice()


def _decode(output, arg_max):
    """(local coordinates [N,K,2] numpy, maxvals or None, heat-map width or None)."""
    if type(output) is tuple:                         # (maps, coords in [0,1]): the coordinate head
        return output[1].data.cpu().numpy().astype(np.float32), None, None
    if isinstance(output, torch.Tensor) and not output.is_cuda:
        output = output.cuda()                        # the decode kernels run on the device
    if isinstance(output, np.ndarray) and arg_max == 'soft':
        pred, mv = lip.soft_arg_max_np(output)
        return pred, mv, output.shape[3]
    if isinstance(output, torch.Tensor) and arg_max == 'soft':
        pred, mv = lip.soft_arg_max(output)
        return pred.cpu().numpy(), mv.cpu().numpy(), output.shape[3]
    if isinstance(output, np.ndarray) or (isinstance(output, torch.Tensor) and arg_max == 'hard'):
        pred, mv = lip.get_max_preds(output)          # numpy in -> numpy out; CUDA tensor -> CUDA tensors
        if torch.is_tensor(pred):
            pred, mv = pred.cpu().numpy(), mv.cpu().numpy()
        return pred, mv, output.shape[3]
    raise NotImplementedError


def get_distance_src(output, meta_data, cfgs=None, image_size=(256.0, 256.0), arg_max='hard'):
    """Mean pixel distance, in the SOURCE image, between predicted and annotated
    key-points: decode -> rescale to the crop resolution -> inverse crop affine
    (centre / scale / rotation from meta_data) -> distances + PCK counts.
    Returns (avg distance, number of joints counted, dict of by-products)."""
    pred, max_vals, map_w = _decode(output, arg_max)
    image_size = image_size if cfgs is None else cfgs['heatmapModel']['input_size']
    width, height = image_size
    if map_w is None:
        pred = pred * np.array(image_size).reshape(1, 1, 2)
    else:
        pred = pred * (image_size[0] / map_w)
    centers, scales = meta_data['center'], meta_data['scale']
    used = pred[:len(centers)]                        # extra predictions belong to unlabeled data
    rots = meta_data['rotation'] if 'rotation' in meta_data else [0.] * len(centers)
    originals = meta_data['original_joints']
    distances, correct, src_all = [], np.zeros(len(PCK_THRES)), []
    for i in range(len(used)):
        t_inv = lip.get_affine_transform(centers[i], scales[i], rots[i], (height, width), inv=1)
        src = lip.affine_transform_modified(used[i], t_inv)
        src_all.append(src[None])
        gt = np.asarray(originals[i])
        distances += get_distance(gt, src)
        correct += get_PCK(src, gt)
    cnt = len(distances)
    others = {'src_coord': np.concatenate(src_all, axis=0), 'joints_pred': pred, 'max_vals': max_vals,
              'correct_cnt': correct, 'PCK_batch': correct / cnt}
    return sum(distances) / cnt, cnt, others


# ---- what the device paths share ---------------------------------------------------------------------------------
class _DeviceAcc(object):
    """``n_doubles`` float64 in HBM that a metric's kernels fold into, and the kernels' workspace.
    ``reset_fn(accumulator pointer, stream)`` launches the metric's reset and returns its status; ``what`` names the
    metric in errors.  ``pending``: updates were launched since the last read-back (the owner sets it)."""

    def __init__(self, n_doubles, reset_fn, what):
        self.n_doubles, self._reset_fn, self.what = n_doubles, reset_fn, what
        self.tensor = self._ws = None
        self.pending = False

    def _launch_reset(self, stream):
        _lib.check(self._reset_fn(_lib.ptr(self.tensor), stream), self.what + ' reset')

    def ensure(self, dev, stream):
        """The accumulator on ``dev``, allocated and reset at the first use."""
        if self.tensor is None or self.tensor.device != dev:
            if self.pending:
                raise RuntimeError('the accumulator holds unread updates of another device')
            self.tensor = torch.empty(self.n_doubles, dtype=torch.float64, device=dev)
            self._launch_reset(stream)
        return self.tensor

    def workspace(self, nbytes, dev):
        if self._ws is None or self._ws.device != dev or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self._ws

    def peek(self):
        """The accumulator's float64 on the host (synchronises); zeros before the first update."""
        if self.tensor is None:
            return np.zeros(self.n_doubles)
        return self.tensor.cpu().numpy()

    def reset(self):
        """Reset the accumulator (a launch, no synchronisation)."""
        self.pending = False
        if self.tensor is None:
            return
        with torch.cuda.device(self.tensor.device):
            self._launch_reset(_lib.current_stream(self.tensor.device))

    def take(self):
        """The one read-back: the accumulator's values, and the accumulator reset."""
        acc = self.peek()
        self.reset()
        return acc


class _MetricsDevice(object):
    """The device side of a 2-D metric: one accumulator, whose ``peek`` / ``reset`` / ``take`` / ``pending`` it
    hands out, and the pinned staging of the host ``meta`` arrays."""

    def __init__(self, n_doubles, reset_fn, what):
        acc = self._acc = _DeviceAcc(n_doubles, reset_fn, what)
        self.peek, self.reset, self.take = acc.peek, acc.reset, acc.take
        self._staging = PinnedStaging(1 << 16)

    pending = property(lambda self: self._acc.pending)


def _synced(name):
    """The host attribute ``name`` behind ``self._sync()``: the first access reads the device accumulator back."""
    def get(self):
        self._sync()
        return getattr(self, name)

    def put(self, value):
        self._sync()
        setattr(self, name, value)
    return property(get, put)


class _RunningMean(object):
    """``count`` / ``mean`` of a 2-D metric: host updates, and the updates ``_dev`` folded on the device, merged at the
    first access."""
    count, mean = _synced('_count'), _synced('_mean')

    def _sync(self):
        """The one read-back: the device accumulator is merged into the host attributes and reset.  Returns what was
        merged, None if nothing was counted."""
        if not self._dev.pending:
            return None
        acc = self._dev.take()
        cnt = int(acc[0])
        if cnt == 0:
            return None
        self._mean = (self._mean * self._count + acc[1]) / (self._count + cnt)
        self._count += cnt
        return acc


class _Meter(object):
    """The meter contract of ``trainer.train``: ``accumulate(prediction, meta, cfgs=None)`` only launches; ``read()`` ->
    (running mean, count, ...) since the last ``reset()`` is the read-back.  A subclass holds ``_dev`` and says when a
    prediction is on the device (``_on_device``), what to raise otherwise (``_needs_cuda``) and how to launch
    (``_update``)."""
    _more = staticmethod(lambda acc: ())            # what read() returns after (mean, count)

    def _check(self, prediction):
        if not self._on_device(prediction):
            raise TypeError(self._needs_cuda)

    def accumulate(self, prediction, meta, cfgs=None):
        self._check(prediction)
        self._update(prediction, meta, cfgs)

    def read(self):
        acc = self._dev.peek()
        cnt = int(acc[0])
        return ((acc[1] / cnt if cnt else 0.0), cnt) + self._more(acc)

    def reset(self):
        self._dev.reset()


class AngleError(_RunningMean):
    """Running mean of get_angle_error over an evaluation pass (criterions.py:145-171).  CUDA predictions are folded
    into a device accumulator (csrc/angle_metrics.hip): ``update`` only launches, the one read-back is in ``report()``
    or at the first access of ``count`` / ``mean``; numpy inputs and CPU tensors take the host path.  Both kinds of
    update merge in one object.  ``device_update = False`` sends CUDA predictions down the host path too."""
    device_update = True

    def __init__(self, cfgs, num_joints=None):
        self.name = 'Angle error in degrees'
        self.num_joints, self._count, self._mean = num_joints, 0, 0.
        self._dev = _AngleMetricsDevice()

    def update(self, prediction, meta_data, ground_truth=None, logger=None):
        if self.device_update and torch.is_tensor(prediction) and prediction.is_cuda:
            self._dev.update(prediction, meta_data)
            return
        avg, cnt, _ = get_angle_error(prediction.cpu() if torch.is_tensor(prediction) else prediction, meta_data)
        self.mean = (self.mean * self.count + cnt * avg) / (self.count + cnt)
        self.count += cnt

    def report(self, logger):
        logger.info('Error type: {:s}\tError: {}\t'.format(self.name, self.mean))


# ---- get_distance_src on the device -----------------------------------------------------------------------------
_KPT_ACC_DOUBLES = 8                                # include/egonet_hip.h: count, sum of distances, pck[3]
_KPT_MODES = {'hard': 0, 'soft': 1, 'soft-np': 2}   # the decode modes a CUDA heat-map can take
_KPT_META = ('center', 'scale', 'rotation', 'original_joints')


def _kpt_on_device(prediction):
    """CUDA heat-maps, or a (maps, coordinates) tuple whose coordinates are CUDA: the device path."""
    if type(prediction) is tuple:
        return torch.is_tensor(prediction[1]) and prediction[1].is_cuda
    return torch.is_tensor(prediction) and prediction.is_cuda


class _KptMetricsDevice(_MetricsDevice):
    """The device side of get_distance_src (csrc/kpt_metrics.hip): one accumulator in HBM, two launches per batch,
    nothing read back before ``peek()``."""

    def __init__(self):
        super().__init__(_KPT_ACC_DOUBLES, lambda acc, st: _lib.lib().egn_kpt_metrics_reset(acc, st),
                         'key-point metrics')

    def _labels(self, meta, K, dev):
        """center [n,2], scale [n,2], rotation [n], original_joints [n,K,3] as float64 device tensors."""
        n = len(meta['center'])
        fields = {}
        for key, shape in zip(_KPT_META, ((n, 2), (n, 2), (n,), (n, K, 3))):
            v = meta[key] if key in meta else None          # a missing 'rotation' means zeros
            if torch.is_tensor(v) and v.is_cuda:
                v = v.detach().to(device=dev, dtype=torch.float64)
                if key == 'original_joints' and v.shape[-1] == 2:
                    v = torch.cat([v, torch.ones_like(v[..., :1])], dim=-1)
                fields[key] = v.reshape(shape).contiguous()
                continue
            a = np.zeros(shape) if v is None else np.asarray(v.numpy() if torch.is_tensor(v) else v, dtype=np.float64)
            if key == 'original_joints':
                if a.ndim != 3 or a.shape[:2] != (n, K) or a.shape[2] not in (2, 3):
                    raise ValueError('Array shape not supported.')
                if a.shape[2] == 2:                           # no visibility column: every joint counts
                    a = np.concatenate([a, np.ones((n, K, 1))], axis=2)
            fields[key] = a.reshape(shape)
        host = {k: fields[k] for k in _KPT_META if isinstance(fields[k], np.ndarray)}
        fields.update(self._staging.upload(host, dev)[0] if host and n else dict.fromkeys(host))
        return n, fields

    def update(self, prediction, meta, image_size, arg_max, want=()):
        """Launch only.  ``want``: any of 'src_coord', 'joints_pred', 'max_vals' -> dict of device tensors."""
        if type(prediction) is tuple:
            hm, coords, mode = None, prediction[1].detach().float().contiguous(), 0
            if coords.dim() != 3 or coords.shape[2] != 2:
                raise ValueError('coordinates must be [N, K, 2]')
            N, K, H, W = coords.shape[0], coords.shape[1], 0, 0
            dev = coords.device
        else:
            if arg_max not in _KPT_MODES:
                raise NotImplementedError
            hm, coords, mode = prediction.detach().float().contiguous(), None, _KPT_MODES[arg_max]
            assert hm.dim() == 4, 'batch_images should be 4-ndim'
            N, K, H, W = hm.shape
            dev = hm.device
        L = _lib.lib()
        out = {}
        with torch.cuda.device(dev):
            n, f = self._labels(meta, K, dev)
            if n > N:
                raise ValueError('%d labelled instances for %d predictions' % (n, N))
            st = _lib.current_stream(dev)
            acc = self._acc.ensure(dev, st)
            nb = L.egn_kpt_metrics_ws_bytes(N, K)
            if nb < 0:
                raise ValueError('key-point metrics: %d x %d maps' % (N, K))
            ws = self._acc.workspace(nb, dev)
            if 'src_coord' in want:
                out['src_coord'] = torch.empty(n, K, 2, dtype=torch.float64, device=dev)
            if 'joints_pred' in want:
                out['joints_pred'] = torch.empty(N, K, 2, dtype=torch.float32, device=dev)
            if 'max_vals' in want and hm is not None:
                out['max_vals'] = torch.empty(N, K, 1, dtype=torch.float32, device=dev)
            _lib.check(L.egn_kpt_metrics_update_f32(
                _lib.ptr(hm), _lib.ptr(coords), N, K, H, W, mode, _lib.ptr(f['center']), _lib.ptr(f['scale']),
                _lib.ptr(f['rotation']), _lib.ptr(f['original_joints']), n, float(image_size[0]), float(image_size[1]),
                _lib.ptr(ws), ws.numel(), _lib.ptr(acc), _lib.ptr(out.get('src_coord')),
                _lib.ptr(out.get('joints_pred')), _lib.ptr(out.get('max_vals')), st), 'key-point metrics update')
        self._acc.pending = self._acc.pending or N > 0
        return out


class DistanceSrcMeter(_Meter):
    """get_distance_src as the training loop's ``metric_func`` with the whole metric on the device
    (csrc/kpt_metrics.hip).  ``meter(prediction, meta, cfgs)`` returns ``(avg, cnt, others)`` like get_distance_src
    and synchronises like it: a drop-in replacement.  ``accumulate(prediction, meta, cfgs=None)`` only launches;
    ``read()`` -> (running mean, count, PCK_counts) since the last ``reset()`` is the read-back.  ``trainer.train``
    uses the three when it finds ``accumulate``.  Predictions must be CUDA: heat-maps [N,K,H,W] with ``arg_max``
    'hard' / 'soft' / 'soft-np', or a (maps, coordinates) tuple."""
    _on_device = staticmethod(_kpt_on_device)
    _needs_cuda = 'DistanceSrcMeter needs a CUDA prediction; get_distance_src takes host arrays'
    _more = staticmethod(lambda acc: (acc[2:5].copy(),))         # the PCK counts

    def __init__(self, cfgs=None, image_size=(256., 256.), arg_max='hard'):
        self.image_size = image_size if cfgs is None else cfgs['heatmapModel']['input_size']
        self.arg_max = arg_max
        self._dev = _KptMetricsDevice()
        self._call = _KptMetricsDevice()            # the per-batch figures of __call__: an accumulator of its own

    def _size(self, cfgs):
        return self.image_size if cfgs is None else cfgs['heatmapModel']['input_size']

    def _update(self, prediction, meta, cfgs):
        self._dev.update(prediction, meta, self._size(cfgs), self.arg_max)

    def __call__(self, prediction, meta, cfgs=None):
        self._check(prediction)
        out = self._call.update(prediction, meta, self._size(cfgs), self.arg_max,
                                want=('src_coord', 'joints_pred', 'max_vals'))
        acc = self._call.take()
        cnt = int(acc[0])
        correct = acc[2:5].copy()
        others = {'src_coord': out['src_coord'].cpu().numpy(), 'joints_pred': out['joints_pred'].cpu().numpy(),
                  'max_vals': out['max_vals'].cpu().numpy() if 'max_vals' in out else None,
                  'correct_cnt': correct, 'PCK_batch': correct / cnt if cnt else np.zeros(len(PCK_THRES))}
        return (acc[1] / cnt if cnt else 0.0), cnt, others


# ---- get_angle_error on the device ------------------------------------------------------------------------------
_ANGLE_ACC_DOUBLES = 2                              # include/egonet_hip.h: rows counted, sum of errors in degrees


class _AngleMetricsDevice(_MetricsDevice):
    """The device side of get_angle_error (csrc/angle_metrics.hip): a {count, sum} accumulator in HBM, two launches
    per batch, nothing read back before ``peek()``.  A host ``meta['angles_gt']`` travels in one pinned non-blocking
    copy."""

    def __init__(self):
        super().__init__(_ANGLE_ACC_DOUBLES, lambda acc, st: _lib.lib().egn_angle_metrics_reset(acc, st),
                         'angle metrics')

    def update(self, prediction, meta):
        """Launch only.  ``prediction`` [N, >= 2] float32 CUDA, any row pitch (only [cos, sin] are read)."""
        pred = prediction.detach()
        if pred.dim() != 2 or pred.shape[1] < 2:
            raise ValueError('angle predictions must be [N, 2] rows of [cos, sin], got %s' % (tuple(pred.shape),))
        if pred.dtype != torch.float32 or pred.stride(1) != 1 or (pred.shape[0] > 1 and pred.stride(0) < 2):
            pred = pred.float().contiguous()
        N, dev = pred.shape[0], pred.device
        gt = meta['angles_gt']
        if len(gt) != N:
            raise ValueError('%d angles_gt for %d predictions' % (len(gt), N))
        L = _lib.lib()
        with torch.cuda.device(dev):
            st = _lib.current_stream(dev)
            acc = self._acc.ensure(dev, st)
            if N == 0:
                return
            if torch.is_tensor(gt) and gt.is_cuda:
                gt = gt.detach().to(device=dev, dtype=torch.float64).reshape(N).contiguous()
            else:
                gt = np.asarray(gt.numpy() if torch.is_tensor(gt) else gt, dtype=np.float64).reshape(N)
                gt = self._staging.upload({'angles_gt': gt}, dev)[0]['angles_gt']
            ws = self._acc.workspace(L.egn_angle_metrics_ws_bytes(N), dev)
            _lib.check(L.egn_angle_metrics_update_f32(_lib.ptr(pred), N, pred.stride(0) if N > 1 else 2, _lib.ptr(gt),
                                                      _lib.ptr(ws), ws.numel(), _lib.ptr(acc), st),
                       'angle metrics update')
        self._acc.pending = True


class AngleErrorMeter(_Meter):
    """get_angle_error as the training loop's ``metric_func`` with the metric on the device (csrc/angle_metrics.hip),
    the contract of ``DistanceSrcMeter``: ``accumulate(prediction, meta, cfgs=None)`` only launches; ``read()`` ->
    (running mean in degrees, count) since the last ``reset()`` is the read-back; ``meter(prediction, meta, cfgs)``
    returns ``(avg, cnt, None)`` like get_angle_error and synchronises like it.  Predictions must be CUDA [N, 2]."""
    _on_device = staticmethod(lambda prediction: torch.is_tensor(prediction) and prediction.is_cuda)
    _needs_cuda = 'AngleErrorMeter needs a CUDA prediction; get_angle_error takes host arrays'

    def __init__(self, cfgs=None):
        self._dev = _AngleMetricsDevice()

    def _update(self, prediction, meta, cfgs):
        self._dev.update(prediction, meta)

    def __call__(self, prediction, meta, cfgs=None):
        self._check(prediction)
        return get_angle_error(prediction, meta, cfgs)


class JointDistance2DSIP(_RunningMean):
    """Running mean of get_distance_src + PCK over an evaluation pass.  CUDA predictions (heat-maps, or a tuple whose
    coordinates are CUDA) are folded into a device accumulator (csrc/kpt_metrics.hip) and read back once, at
    ``report()`` or at the first access of ``count`` / ``mean`` / ``PCK_counts``; numpy inputs and CPU tensors take
    the host path of get_distance_src.  Both kinds of update merge in one object.  ``device_update = False`` sends
    CUDA predictions down the host path too (decode on the device, the rest on the host): the comparison of
    tools/kpt_metrics_bench.py."""
    device_update = True

    def __init__(self, cfgs, num_joints=None):
        self.name = 'Joint distance in the source image plane'
        self.num_joints = num_joints if num_joints is not None else cfgs['heatmapModel']['num_joints']
        self.image_size = cfgs['heatmapModel']['input_size']
        self.arg_max = cfgs['testing_settings'].get('arg_max')
        self._count, self._mean, self._pck = 0, 0., np.zeros(len(PCK_THRES))
        self._dev = _KptMetricsDevice()

    PCK_counts = _synced('_pck')

    def _sync(self):
        acc = _RunningMean._sync(self)
        if acc is not None:
            self._pck = self._pck + acc[2:5]

    def update(self, prediction, meta_data, ground_truth=None, logger=None):
        if self.device_update and _kpt_on_device(prediction):
            self._dev.update(prediction, meta_data, self.image_size, self.arg_max)
            return
        avg, cnt, others = get_distance_src(prediction, meta_data, arg_max=self.arg_max, image_size=self.image_size)
        self.mean = (self.mean * self.count + cnt * avg) / (self.count + cnt)
        self.count += cnt
        self.PCK_counts += others['correct_cnt']

    def report(self, logger):
        logger.info('Ealuaton Results:')
        logger.info('Error type: {:s}\tMPJPE: {}\t'.format(self.name, self.mean))
        for thres, value in zip(PCK_THRES, self.PCK_counts):
            logger.info('PCK at threshold {:.2f}: {:.3f}'.format(thres, value / self.count))


# ---- the lifter's 3-D metrics -----------------------------------------------------------------------------------
_LAYOUT_COLS = {0: 35, 1: 39}                       # csrc/metric_math.h: 'R3d' / 'R3d+T' result columns
_ACC_SUM, _ACC_MAX, _ACC_MIN = 8, 48, 88            # include/egonet_hip.h: the accumulator's float64 slots
_ACC_DOUBLES = 128


def _euler_xyz_abs_deg(R):
    """|Rotation.from_matrix(R).as_euler('xyz', degrees=True)| for R [n,3,3] float64: extrinsic x-y-z,
    R = Rz(c) Ry(b) Rx(a); at gimbal lock the third angle is zero like scipy's (csrc/metric_math.h)."""
    cb = np.sqrt(R[:, 0, 0] ** 2 + R[:, 1, 0] ** 2)
    lock = cb <= 1e-7
    a = np.where(lock, np.arctan2(-R[:, 1, 2], R[:, 1, 1]), np.arctan2(R[:, 2, 1], R[:, 2, 2]))
    c = np.where(lock, 0.0, np.arctan2(R[:, 1, 0], R[:, 0, 0]))
    return np.abs(np.stack([a, np.arctan2(-R[:, 2, 0], cb), c], axis=1) * (180.0 / np.pi))


def _rotation_errors(prediction, ground_truth):
    """update_rotation_error style 'euler' (criterions.py:241-269, transformation.py:99-134) for all rows at once."""
    n = len(prediction)
    X = np.asarray(prediction, dtype=np.float64).reshape(n, -1, 3)
    Y = np.asarray(ground_truth, dtype=np.float64).reshape(n, -1, 3)
    Xm = X - X.mean(axis=1, keepdims=True)
    Ym = Y - Y.mean(axis=1, keepdims=True)
    H = np.einsum('nir,nic->nrc', Xm, Ym)
    U, _, Vt = np.linalg.svd(H)
    R = np.einsum('nkr,nck->nrc', Vt, U)                            # Vt.T @ U.T
    flip = np.linalg.det(R) < 0
    Vt[flip, 2, :] *= -1                                            # the reflection fix, transformation.py:125-132
    R[flip] = np.einsum('nkr,nck->nrc', Vt[flip], U[flip])
    return _euler_xyz_abs_deg(R)


def _joint_distances(prediction, ground_truth):
    n = len(prediction)
    p = np.asarray(prediction, dtype=np.float64).reshape(n, -1, 3)
    g = np.asarray(ground_truth, dtype=np.float64).reshape(n, -1, 3)
    return np.sqrt(((g - p) ** 2).sum(axis=2))


class _Stats3D(object):
    """count / mean / max / min per group of error columns (update_statistics, criterions.py:223-239) with a host
    and a device accumulator.  ``_groups``: (name_str, first column, end column) in the kernel's column order."""
    _groups = ()
    device_update = True

    def _init_stats(self, layout):
        self._layout = layout
        self._host = {}
        for name, a, b in self._groups:
            self._host['count' + name] = 0
            self._host['mean' + name] = np.zeros(b - a)
            self._host['max' + name] = -np.ones(b - a)
            self._host['min' + name] = np.ones(b - a) * 1e16
        self._stats_host = self._stats_dev = None
        self._acc = _DeviceAcc(_ACC_DOUBLES, lambda acc, st: _lib.lib().egn_lifter_metrics_reset(acc, layout, st),
                               'metrics')

    def __getattr__(self, key):                     # only reached for names that are not ordinary attributes
        host = self.__dict__.get('_host')
        if host is not None and key in host:
            self._sync()
            return host[key]
        raise AttributeError(key)

    def _fold(self, name, update):
        """update_statistics for one group; ``update`` [n, columns] float64."""
        h, n = self._host, len(update)
        h['mean' + name] = (h['count' + name] * h['mean' + name] + np.sum(update, axis=0)) / (h['count' + name] + n)
        h['count' + name] = h['count' + name] + n
        h['max' + name] = np.maximum(h['max' + name], update.max(axis=0))
        h['min' + name] = np.minimum(h['min' + name], update.min(axis=0))

    def set_statistics(self, mean_out, std_out):
        """The fused unnormalise of the device path (and the float32 one of the host path): ``x * std + mean``."""
        self._stats_host = (np.ascontiguousarray(mean_out, dtype=np.float32).reshape(-1),
                            np.ascontiguousarray(std_out, dtype=np.float32).reshape(-1))
        self._stats_dev = None

    def _use_statistics(self, statistics):
        if statistics is not None:
            cur = self._stats_host
            m = np.ascontiguousarray(statistics['mean_out'], dtype=np.float32).reshape(-1)
            s = np.ascontiguousarray(statistics['std_out'], dtype=np.float32).reshape(-1)
            if cur is None or not (np.array_equal(cur[0], m) and np.array_equal(cur[1], s)):
                self.set_statistics(m, s)
        return self._stats_host

    def _update_device(self, prediction, ground_truth, statistics=None, rows_out=None):
        pred, gt = prediction.detach(), ground_truth.detach()
        if pred.dtype != torch.float32 or gt.dtype != torch.float32 or pred.dim() != 2 or pred.shape != gt.shape:
            raise ValueError('%s: float32 [n, D] prediction and ground truth of one shape' % self.name)
        D = 99 if self._layout else 96
        if pred.shape[1] != D:
            raise ValueError('%s: rows of %d values, the device path takes %d' % (self.name, pred.shape[1], D))
        if pred.stride(1) != 1 or pred.stride(0) != gt.stride(0) or gt.stride(1) != 1 or pred.stride(0) < D:
            pred, gt = pred.contiguous(), gt.contiguous()
        dev, n = pred.device, pred.shape[0]
        if n == 0:
            return
        L = _lib.lib()
        stats = self._use_statistics(statistics)
        with torch.cuda.device(dev):
            st = _lib.current_stream(dev)
            if self._acc.pending and self._acc.tensor.device != dev:
                self._sync()                        # what another device holds goes to the host statistics first
            acc = self._acc.ensure(dev, st)
            ws = self._acc.workspace(L.egn_lifter_metrics_ws_bytes(n), dev)
            mean = std = None
            if stats is not None:
                if stats[0].size != D or stats[1].size != D:
                    raise ValueError('%s: statistics of %d values for rows of %d' % (self.name, stats[0].size, D))
                if self._stats_dev is None or self._stats_dev[0].device != dev:
                    self._stats_dev = tuple(torch.from_numpy(a).to(dev) for a in stats)
                mean, std = self._stats_dev
            if rows_out is not None and (rows_out.dtype != torch.float64 or not rows_out.is_contiguous() or
                                         tuple(rows_out.shape) != (n, _LAYOUT_COLS[self._layout])):
                raise ValueError('rows_out must be contiguous float64 [%d, %d]' % (n, _LAYOUT_COLS[self._layout]))
            _lib.check(L.egn_lifter_metrics_update_f32(
                _lib.ptr(pred), _lib.ptr(gt), n, D, pred.stride(0) if n else D, _lib.ptr(mean), _lib.ptr(std),
                self._layout, _lib.ptr(ws), ws.numel(), _lib.ptr(acc), _lib.ptr(rows_out), st),
                'metrics update')
        self._acc.pending = True

    def _sync(self):
        """The one read-back: the device accumulator is merged into the host attributes and reset."""
        dev = self.__dict__.get('_acc')             # __getattr__ may come here before _init_stats
        if dev is None or not dev.pending:
            return
        acc = dev.take()
        n = int(acc[0])
        if n == 0:
            return
        h = self._host
        for name, a, b in self._groups:
            shape = (1, 3) if name.endswith('_xyz') else (b - a,)      # the reference's [1, 3] arrays, see RTError3D
            h['mean' + name] = (h['count' + name] * h['mean' + name] +
                                acc[_ACC_SUM + a:_ACC_SUM + b].reshape(shape)) / (h['count' + name] + n)
            h['count' + name] = h['count' + name] + n
            h['max' + name] = np.maximum(h['max' + name], acc[_ACC_MAX + a:_ACC_MAX + b].reshape(shape))
            h['min' + name] = np.minimum(h['min' + name], acc[_ACC_MIN + a:_ACC_MIN + b].reshape(shape))

    def _host_arrays(self, prediction, ground_truth, statistics):
        prediction, ground_truth = np.asarray(prediction), np.asarray(ground_truth)
        stats = self._use_statistics(statistics)
        if stats is not None:                       # operations.py:50-52 on float32 arrays
            m, s = stats[0].reshape(1, -1), stats[1].reshape(1, -1)
            prediction = prediction.astype(np.float32) * s + m
            ground_truth = ground_truth.astype(np.float32) * s + m
        return prediction, ground_truth

    def _is_device(self, prediction):
        return torch.is_tensor(prediction) and prediction.is_cuda


def _check_styles(name, T_style, R_style, sample_style):
    if sample_style != 'bbox9':
        raise NotImplementedError('%s: 3d_kpt_sample_style %r (criterions.py:399-402 knows bbox9 only)'
                                  % (name, sample_style))
    if T_style == 'procrustes':
        raise NotImplementedError("%s: T_style 'procrustes' (criterions.py:285-292 aligns the prediction in place, "
                                  'the rotation error that follows is that of the aligned points)' % name)
    if T_style != 'direct':
        raise NotImplementedError('%s: T_style %r (criterions.py:352-357, 465-479)' % (name, T_style))
    if R_style != 'euler':
        raise NotImplementedError('%s: R_style %r (criterions.py:266-267 knows euler only)' % (name, R_style))


class RError3D(_Stats3D):
    """Relative shape error; rows [shape relative to the root] (criterions.py:390-449)."""
    _groups = (('_rT', 0, 32), ('_R', 32, 35))

    def __init__(self, cfgs, num_joints):
        self.name = 'RError3D'
        self.T_style = cfgs['metrics']['R3D']['T_style']
        self.R_style = cfgs['metrics']['R3D']['R_style']
        _check_styles(self.name, self.T_style, self.R_style, cfgs['dataset']['3d_kpt_sample_style'])
        self.num_joints = num_joints - 1            # discount the root joint
        self._groups = (('_rT', 0, self.num_joints), ('_R', 32, 35))
        self._init_stats(0)

    def update(self, prediction, ground_truth=None, meta_data=None, logger=None, statistics=None):
        if self._is_device(prediction):
            if self.num_joints != 32:
                raise NotImplementedError('RError3D on the device: 33-point cuboids (32 points + root)')
            return self._update_device(prediction, ground_truth, statistics)
        prediction, ground_truth = self._host_arrays(prediction, ground_truth, statistics)
        self._fold('_rT', _joint_distances(prediction, ground_truth))
        self._fold('_R', _rotation_errors(prediction, ground_truth))

    def report(self, logger):
        MPJPE = self.mean_rT.sum() / self.num_joints
        logger.info('Error type: {error_type:s}\t'
                    'MPJPE of the shape relative to the root:\t'
                    'MPJPE: {MPJPE}\t'
                    'Rotation error of the shape relative to the root:\t'
                    'Mean error: {mean_R}\t'
                    'Max error: {max_R}\t'
                    'Min error: {min_R}\t'.format(error_type=self.name, MPJPE=MPJPE, mean_R=self.mean_R,
                                                 max_R=self.max_R, min_R=self.min_R))


class RTError3D(_Stats3D):
    """Rotation and translation error combined; rows [root, shape relative to the root] (criterions.py:451-538)."""

    def __init__(self, cfgs, num_joints):
        self.name = 'RTError3D'
        self.T_style = cfgs['metrics']['RTError3D']['T_style']
        self.R_style = cfgs['metrics']['RTError3D']['R_style']
        _check_styles(self.name, self.T_style, self.R_style, cfgs['dataset']['3d_kpt_sample_style'])
        self.num_joints = num_joints - 1
        self._groups = (('_T', 35, 36), ('_T_xyz', 36, 39), ('_rT', 0, self.num_joints), ('_R', 32, 35))
        self._init_stats(1)

    def update(self, prediction, ground_truth=None, meta_data=None, logger=None, statistics=None):
        if self._is_device(prediction):
            if self.num_joints != 32:
                raise NotImplementedError('RTError3D on the device: 33-point cuboids (root + 32 points)')
            return self._update_device(prediction, ground_truth, statistics)
        prediction, ground_truth = self._host_arrays(prediction, ground_truth, statistics)
        self._fold('_T', _joint_distances(prediction[:, :3], ground_truth[:, :3]))
        # [n, 1, 3] like the reference's reshape(n, -1, 3): its _T_xyz attributes are [1, 3] after the first update
        self._fold('_T_xyz', np.abs(ground_truth[:, :3].astype(np.float64) -
                                    prediction[:, :3].astype(np.float64)).reshape(-1, 1, 3))
        self._fold('_rT', _joint_distances(prediction[:, 3:], ground_truth[:, 3:]))
        self._fold('_R', _rotation_errors(prediction[:, 3:], ground_truth[:, 3:]))

    def report(self, logger):
        MPJPE = self.mean_rT.sum() / self.num_joints
        logger.info('Error type: {error_type:s}\t'
                    'Translation error of the root:\t'
                    'Mean error: {mean_T}\t'
                    'Max error: {max_T}\t'
                    'Min error: {min_T}\t'
                    'Translation error of the root in three directions:\t'
                    'Mean error (L1): {mean_T_xyz}\t'
                    'MPJPE of the shape relative to the root:\t'
                    'MPJPE: {MPJPE}\t'
                    'Rotation error of the shape relative to the root:\t'
                    'Mean error: {mean_R}\t'
                    'Max error: {max_R}\t'
                    'Min error: {min_R}\t'.format(error_type=self.name, MPJPE=MPJPE, mean_T=self.mean_T,
                                                 max_T=self.max_T, min_T=self.min_T, mean_T_xyz=self.mean_T_xyz,
                                                 mean_R=self.mean_R, max_R=self.max_R, min_R=self.min_R))


class JointDistance3D(_Stats3D):
    """Joint distance error (criterions.py:343-388); the device path takes the 96-column rows."""

    def __init__(self, cfgs):
        self.name = 'Joint distance'
        self.style = cfgs['metrics']['JD3D']['style']
        if self.style == 'procrustes':
            raise NotImplementedError("JointDistance3D: style 'procrustes' (criterions.py:285-292)")
        if self.style != 'direct':
            raise NotImplementedError('JointDistance3D: style %r (criterions.py:352-357)' % (self.style,))
        self.num_joints = int(cfgs['FCModel']['output_size'] / 3)
        self._groups = (('', 0, self.num_joints),)
        self._init_stats(0)

    def update(self, prediction, ground_truth=None, meta_data=None, logger=None, statistics=None):
        if self._is_device(prediction):
            if self.num_joints != 32:
                raise NotImplementedError('JointDistance3D on the device: 96-column rows (32 points)')
            return self._update_device(prediction, ground_truth, statistics)
        prediction, ground_truth = self._host_arrays(prediction, ground_truth, statistics)
        self._fold('', _joint_distances(prediction, ground_truth))

    def report(self, logger):
        MPJPE = self.mean.sum() / self.num_joints
        logger.info('Error type: {error_type:s}\t'
                    'MPJPE: {MPJPE}\t'
                    'Mean error for each joint: {mean_error}\t'
                    'Max error for each joint: {max_error}\t'
                    'Min error for each joint: {min_error}\t'.format(error_type=self.name, MPJPE=MPJPE,
                                                                    mean_error=self.mean, max_error=self.max,
                                                                    min_error=self.min))


class RotationError3D(_Stats3D):
    """Rotation estimation error (criterions.py:303-341); the device path takes the 96-column rows."""
    _groups = (('', 32, 35),)

    def __init__(self, cfgs):
        self.name = 'Rotation error'
        self.style = cfgs['metrics']['R3D']['style']
        if self.style != 'euler':
            raise NotImplementedError('RotationError3D: style %r (criterions.py:266-267 knows euler only)'
                                      % (self.style,))
        self._init_stats(0)

    def update(self, prediction, ground_truth=None, meta_data=None, logger=None, statistics=None):
        if self._is_device(prediction):
            return self._update_device(prediction, ground_truth, statistics)
        prediction, ground_truth = self._host_arrays(prediction, ground_truth, statistics)
        self._fold('', _rotation_errors(prediction, ground_truth))

    def report(self, logger):
        logger.info('Error type: {error_type:s}\t'
                    'Mean error: {mean_error}\t'
                    'Max error: {max_error}\t'
                    'Min error: {min_error}\t'.format(error_type=self.name, mean_error=self.mean,
                                                     max_error=self.max, min_error=self.min))


def _make_metric(cls):
    import inspect
    takes_joints = 'num_joints' in inspect.signature(cls.__init__).parameters
    return (lambda cfgs, num_joints: cls(cfgs, num_joints)) if takes_joints else (lambda cfgs, num_joints: cls(cfgs))


# the names ``Evaluator`` resolves (the reference evaluates the string, criterions.py:549-550)
METRICS = {c.__name__: _make_metric(c) for c in (RError3D, RTError3D, JointDistance3D, RotationError3D,
                                                 JointDistance2DSIP, AngleError)}


class Evaluator(object):
    """A list of metrics by name (criterions.py:540-573).  ``device_update``: ``trainer.evaluate`` may hand CUDA
    tensors and the set's statistics to ``update`` instead of unnormalised host arrays; it holds when every metric
    of the list has the device path."""

    def __init__(self, metrics, cfgs=None, num_joints=9):
        self.metrics = []
        for metric in metrics:
            if metric not in METRICS:
                raise NotImplementedError('metric %r (known: %s)' % (metric, ', '.join(sorted(METRICS))))
            self.metrics.append(METRICS[metric](cfgs, num_joints))
        self.device_update = bool(self.metrics) and all(isinstance(m, _Stats3D) for m in self.metrics)

    def set_statistics(self, mean_out, std_out):
        for metric in self.metrics:
            metric.set_statistics(mean_out, std_out)

    def update(self, prediction, ground_truth=None, meta_data=None, logger=None, statistics=None):
        for metric in self.metrics:
            if statistics is not None:
                metric.update(prediction, ground_truth=ground_truth, meta_data=meta_data, logger=logger,
                              statistics=statistics)
            else:
                metric.update(prediction, ground_truth=ground_truth, meta_data=meta_data, logger=logger)

    def report(self, logger):
        for metric in self.metrics:
            metric.report(logger)
