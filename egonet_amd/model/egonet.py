"""Ego-Net inference orchestrator -- MI355X build.

Mirrors the reference's ``libs/model/egonet.py`` public surface for the hot
path (``EgoNet(cfgs, pre_trained)``, attributes ``HC, L, LS, resolution,
xy_dict, pth_trans``; methods ``get_keypoints``, ``lift_2d_to_3d``,
``get_6d_rep``, ``get_observation_angle_proj/_trans``, ``forward``,
``post_process``) and adds ``infer_crops``: the whole chain

    crops -> HC -> decode -> x resolution -> inverse crop affine -> normalise
          -> L -> un-normalise -> cuboid template + Kabsch + euler -> alpha

for a whole batch in one stream of HIP launches with no host round trip, where
the reference loops over instances in Python (egonet.py:443-453, 469-486,
279-295).  ``get_keypoints`` / ``lift_2d_to_3d`` are thin record-keeping
wrappers over that batched path and return the reference's dictionaries.

Crop extraction (``crop_instances``) runs on the GPU (common/crop_gpu.py); the
reference's cv2.warpAffine route needs ``cv2`` and imports it lazily.
``post_process(visualize=True)`` draws the predictions on the frames with the
rasteriser of csrc/overlay.hip (egonet_amd/visualization).
"""
import math
from os.path import join as pjoin

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from . import FCmodel
from . import heatmapModel  # noqa: F401  (plugin namespace)
from ..common import img_proc
from ..common.img_proc import modify_bbox, to_npy
from ..common.format import get_pred_str, save_txt_file
import egonet_amd.model as models  # noqa: F401  (eval() lookup below, like the reference)


def _dev_f64(a, device):
    if torch.is_tensor(a):      # already resident (benchmarks keep inputs in HBM)
        return a.to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device)


class EgoNet(nn.Module):
    def __init__(self, cfgs, pre_trained=False, precision=None, activations=None):
        """``precision``: None (what ``cfgs['heatmapModel']['precision']`` says, default 'f32'), 'f32', 'f16', 'f16s2' or 'f16x' -- the
        opt-in fast inference modes of HC's HIP program (PoseHighResolutionNet.precision).  The lifter, training and
        every CPU path compute in fp32 whatever it says.
        ``activations``: None (what ``cfgs['heatmapModel']['activations']`` says, default 'f32'), 'f32' or 'f16' -- f16
        storage between f16-operand convolutions (PoseHighResolutionNet.activations): the same bits, fewer bytes."""
        super().__init__()
        hm = cfgs['heatmapModel']
        self.cfgs = cfgs
        # plugin lookup by name, as in the reference (egonet.py:43-44)
        self.HC = eval('models.heatmapModel.' + hm['name'] + '.get_pose_net')(cfgs, is_train=False)
        if precision is not None:
            if precision not in ('f32', 'f16', 'f16s2', 'f16x'):
                raise ValueError("precision must be 'f32', 'f16', 'f16s2' or 'f16x', got %r" % (precision,))
            self.HC.precision = precision
        if activations is not None:
            if activations not in ('f32', 'f16'):
                raise ValueError("activations must be 'f32' or 'f16', got %r" % (activations,))
            self.HC.activations = activations
        self.resolution = hm['input_size']
        self.xy_dict = {'flag': hm['add_xy']} if 'add_xy' in hm else None
        fc = cfgs['FCModel']
        self.L = FCmodel.get_fc_model(stage_id=1, cfgs=cfgs, input_size=fc['input_size'],
                                      output_size=fc['output_size'])
        self.LS = None
        self.pth_trans = None
        if pre_trained:
            ckpt = cfgs['dirs']['ckpt']
            self.HC.load_state_dict(torch.load(pjoin(ckpt, 'HC.pth')))
            self.LS = np.load(pjoin(ckpt, 'LS.npy'), allow_pickle=True).item()
            self.L.load_state_dict(torch.load(pjoin(ckpt, 'L.pth')))

    # ------------------------------------------------------------------
    # batched device pipeline
    # ------------------------------------------------------------------
    @torch.no_grad()
    def infer_crops(self, instances, centers, scales, K=None, kpts_x_for_alpha=None,
                    alpha_mode='proj', decode='auto', to_host=True, slot=0, refine=None, roots=None, max_shift=5.0):
        """instances [n,C,H,W] fp32 CUDA crops; centers/scales [n,2] float64
        (``modify_bbox`` outputs).  Returns a dict with
          kpts_2d [n,2J] f64 (screen), kpts_3d [n,J-1,3] f64, euler [n,3],
          translation [n,3], alpha [n] (if K is given), local [n,J,2] fp32
        as numpy arrays (``to_host``) or device tensors.
        decode: 'coords' (coordinate head, the shipped configs), 'soft' /
        'hard' (heat-map arg-max), 'auto' = by ``HC.head_type``.
        slot: which copy of the launch programs to use -- a serving loop that keeps two batches in flight on two
        streams alternates slot 0 / 1 (engine.HRNetEngine.program).
        refine: None, or 'pnp' (needs K, [3,3] or [n,3,3]): one more launch between the un-normalisation and the pose
        solve fits the lifted cuboid rigidly to its own key points (``refine_pnp``; ``roots`` [n,3] = initial roots,
        default the weak-perspective start; ``max_shift`` as there).  The pose solve then runs on the refined relative
        shape, ``translation`` is the refined root ('trans' alpha uses it), and the dict gains ``kpts_3d_refined``
        [n,J,3], ``refine_status`` [n] and ``dims`` [n,3] = (l, h, w).
        """
        if refine not in (None, 'pnp'):
            raise ValueError("refine must be None or 'pnp', got %r" % (refine,))
        if refine == 'pnp' and K is None:
            raise ValueError("refine='pnp' needs the intrinsics K")
        if not instances.is_cuda:
            raise ValueError('infer_crops is the GPU pipeline; pass CUDA crops')
        if self.LS is None:
            raise ValueError('lifter statistics LS are not loaded')
        dev = instances.device
        n = instances.shape[0]
        L = _lib.lib()
        HC = self.HC
        J = HC.num_joints
        width, height = self.resolution
        if decode == 'auto':
            decode = 'coords' if HC.head_type == 'coordinates' else 'soft'
        with torch.cuda.device(dev):
            stream = _lib.current_stream(dev)
            if decode == 'coords':
                _, local = HC._hip_engine().forward(instances.float(), slot=slot)
                mul = (float(width), float(height))
            else:
                mode = 1 if decode == 'soft' else 0
                out, (local, _, _) = HC._hip_engine().forward(instances.float(), decode_mode=mode, slot=slot)
                maps = out[0] if isinstance(out, tuple) else out
                mul = (float(width) / maps.shape[3], float(height) / maps.shape[2])
            key = ('ls', dev)
            if getattr(self, '_ls_dev_key', None) != key:
                self._ls_dev = {k: _dev_f64(v, dev).reshape(-1) for k, v in self.LS.items()}
                self._ls_dev_key = key
            ls = self._ls_dev
            ld_in = (2 * J + 3) // 4 * 4
            c_d = _dev_f64(centers, dev)
            s_d = _dev_f64(scales, dev)
            screen = torch.empty(n, 2 * J, dtype=torch.float64, device=dev)
            lin = torch.zeros(n, ld_in, dtype=torch.float32, device=dev)
            _lib.check(L.egn_keypoints_to_screen_f64(
                _lib.ptr(local), n, J, mul[0], mul[1], _lib.ptr(c_d), _lib.ptr(s_d), int(width),
                int(height), _lib.ptr(screen), _lib.ptr(ls['mean_in']), _lib.ptr(ls['std_in']),
                _lib.ptr(lin), ld_in, stream), 'keypoints_to_screen')
            y = self.L._hip_engine().forward(lin, ld_in=ld_in, slot=slot)
            D = y.shape[1]
            pred3d = torch.empty(n, D, dtype=torch.float64, device=dev)
            _lib.check(L.egn_unnormalize_f64(_lib.ptr(y), n, D, D, _lib.ptr(ls['mean_out']),
                                             _lib.ptr(ls['std_out']), _lib.ptr(pred3d), stream))
            res = {'local': local, 'kpts_2d': screen, 'kpts_3d': pred3d.view(n, -1, 3)}
            if refine == 'pnp' and D != 96:
                raise ValueError("refine='pnp' needs the 96-output lifter (a cuboid of 32 points + root)")
            if D == 96 and refine == 'pnp':
                # a host K is uploaded once, not per step: a copy from pageable memory makes the host wait for the
                # stream, i.e. for HC and the lifter above
                ikey = (K.tobytes(), K.shape, n, dev) if isinstance(K, np.ndarray) else None
                if ikey is None or getattr(self, '_intr_dev_key', None) != ikey:
                    self._intr_dev, self._intr_dev_key = self._intrinsics(K, n, dev), ikey
                intr = self._intr_dev
                ref = self._refine_device(pred3d.view(n, -1, 3), screen, intr, roots, None, max_shift)
                refined = ref['kpts_3d_refined']
                rel = (refined[:, 1:] - refined[:, :1]).contiguous()
                euler = torch.empty(n, 3, dtype=torch.float64, device=dev)
                alpha = torch.empty(n, dtype=torch.float64, device=dev)
                kx = screen[:, 0] if kpts_x_for_alpha is None else _dev_f64(kpts_x_for_alpha, dev)
                # the solve takes one (fx, cx); per-instance intrinsics go in through its argument instead:
                # atan2(-fx, kx - cx) is the angle of atan2(-1, (kx - cx) / fx)
                kx = ((kx - intr[:, 2]) / intr[:, 0]).contiguous()
                amode = 0 if alpha_mode == 'proj' else 1
                _lib.check(L.egn_pose_solve_f64(_lib.ptr(rel), n, _lib.ptr(kx), 1.0, 0.0, amode,
                                                _lib.ptr(euler), _lib.ptr(alpha), stream), 'pose_solve')
                if amode == 1:      # 'trans' on the refined root, not on the first relative point
                    alpha = euler[:, 1] - torch.atan2(-refined[:, 0, 2], refined[:, 0, 0]) - 0.5 * math.pi
                    alpha = torch.remainder(alpha + math.pi, 2 * math.pi) - math.pi
                res.update(euler=euler, alpha=alpha, translation=refined[:, 0, :], kpts_3d_refined=refined,
                           refine_status=ref['status'], dims=ref['dims'])
            elif D == 96:
                euler = torch.empty(n, 3, dtype=torch.float64, device=dev)
                alpha = torch.empty(n, dtype=torch.float64, device=dev)
                amode = 0 if (alpha_mode == 'proj' and K is not None) else 1
                kx = screen[:, 0].contiguous() if kpts_x_for_alpha is None else _dev_f64(kpts_x_for_alpha, dev)
                fx, cx = (float(K[0, 0]), float(K[0, 2])) if K is not None else (1.0, 0.0)
                _lib.check(L.egn_pose_solve_f64(_lib.ptr(pred3d), n, _lib.ptr(kx), fx, cx, amode,
                                                _lib.ptr(euler), _lib.ptr(alpha), stream), 'pose_solve')
                res.update(euler=euler, alpha=alpha, translation=pred3d.view(n, -1, 3)[:, 0, :])
        if to_host:
            res = {k: v.cpu().numpy() for k, v in res.items()}
        return res

    # ------------------------------------------------------------------
    # reference-shaped API
    # ------------------------------------------------------------------
    def new_img_dict(self):
        return {k: [] for k in ('center', 'scale', 'rotation', 'bbox_resize', 'kpts_2d_pred',
                                'label', 'score')}

    @torch.no_grad()
    def get_keypoints(self, instances, records, is_cuda=True):
        """Reference egonet.py:424-467 (coordinates head): fills
        ``records[i]['kpts']`` and returns the per-image dictionary.
        ``is_cuda=False`` is the reference's CPU plumbing (BASELINE config 1): HC runs through
        torch on the CPU (where the model lives) and the crop->screen affine through the host twin
        of the device kernel (same pose_math.h arithmetic)."""
        if is_cuda:
            instances = instances.cuda()
        width, height = self.resolution
        centers = np.ascontiguousarray(np.stack([np.asarray(r['center'], dtype=np.float64) for r in records]))
        scales = np.ascontiguousarray(np.stack([np.asarray(r['scale'], dtype=np.float64) for r in records]))
        out = self.HC(instances.float())
        local = out[1].contiguous()
        n, J = local.shape[:2]
        if instances.is_cuda:
            dev = local.device
            screen = torch.empty(n, 2 * J, dtype=torch.float64, device=dev)
            c_d, s_d = _dev_f64(centers, dev), _dev_f64(scales, dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().egn_keypoints_to_screen_f64(
                    _lib.ptr(local), n, J, float(width), float(height), _lib.ptr(c_d), _lib.ptr(s_d),
                    int(width), int(height), _lib.ptr(screen), None, None, None, 0,
                    _lib.current_stream(dev)), 'keypoints_to_screen')
            screen = screen.cpu().numpy().reshape(n, J, 2)
        else:
            loc = np.ascontiguousarray(local.numpy(), dtype=np.float32)
            screen = np.empty((n, J, 2), dtype=np.float64)
            _lib.check(_lib.lib().egn_keypoints_to_screen_host_f64(
                loc.ctypes.data, n, J, float(width), float(height), centers.ctypes.data, scales.ctypes.data,
                int(width), int(height), screen.ctypes.data), 'keypoints_to_screen_host')
        # Records with a rotation (egonet.py:442-452 passes records[i]['rotation'] to get_affine_transform; the shipped
        # inference path only makes rot = 0 crops, the device kernel's case): the reference's own host arithmetic --
        # local *= resolution in float32, the exact three-point affine (common.img_proc.get_affine_transform, inv = 1),
        # float64 product.  A handful of 33-point products per rotated record, on the host as in the reference.
        rots = [float(r.get('rotation', 0.)) for r in records]
        if any(rots):
            loc = np.array(local.detach().cpu().numpy(), dtype=np.float32, copy=True)
            loc *= np.array([width, height]).reshape(1, 1, 2)
            screen = np.array(screen, dtype=np.float64, copy=True)
            for i, rot in enumerate(rots):
                if rot != 0.:
                    t_inv = img_proc.get_affine_transform(centers[i], scales[i], rot, (height, width), inv=1)
                    screen[i] = img_proc.affine_transform_modified(loc[i], t_inv)
        ret = {}
        for i, record in enumerate(records):
            record['kpts'] = screen[i]
            d = ret.setdefault(record['path'], self.new_img_dict())
            d['kpts_2d_pred'].append(record['kpts'].reshape(1, -1))
            for k in ('center', 'scale', 'bbox_resize', 'label', 'score', 'rotation'):
                d[k].append(record[k])
        return ret

    def lift_2d_to_3d(self, records, cuda=True):
        """Reference egonet.py:469-486, but ONE lifter launch for all images."""
        paths = list(records.keys())
        if not paths:
            return records
        data = np.concatenate([np.concatenate(records[p]['kpts_2d_pred'], axis=0) for p in paths])
        counts = [len(records[p]['kpts_2d_pred']) for p in paths]
        x = ((data - self.LS['mean_in']) / self.LS['std_in']).astype(np.float32)
        x = torch.from_numpy(x)
        if cuda:
            x = x.cuda()
        with torch.no_grad():
            pred = self.L(x).data.cpu().numpy()
        pred = pred * self.LS['std_out'] + self.LS['mean_out']
        o = 0
        for p, c in zip(paths, counts):
            records[p]['kpts_3d_pred'] = pred[o:o + c].reshape(c, -1, 3)
            o += c
        return records

    def get_6d_rep(self, predictions, ax=None, color='black'):
        """Reference egonet.py:279-295, batched on the GPU."""
        predictions = np.asarray(predictions, dtype=np.float64).reshape(len(predictions), -1, 3)
        euler, _ = self._pose(predictions, None, None, 1)
        return euler, predictions[:, 0, :]

    def _pose(self, pred3d, kpt_x, K, amode):
        dev = next(self.parameters()).device
        n = len(pred3d)
        if dev.type != 'cuda':       # CPU model (BASELINE config 1): the host twin, same arithmetic
            p = np.ascontiguousarray(np.asarray(pred3d, dtype=np.float64).reshape(n, -1))
            euler = np.empty((n, 3), dtype=np.float64)
            alpha = np.empty(n, dtype=np.float64)
            kx = None if kpt_x is None else np.ascontiguousarray(kpt_x, dtype=np.float64)
            fx, cx = (float(K[0, 0]), float(K[0, 2])) if K is not None else (1.0, 0.0)
            _lib.check(_lib.lib().egn_pose_solve_host_f64(
                p.ctypes.data, n, None if kx is None else kx.ctypes.data, fx, cx, amode,
                euler.ctypes.data, alpha.ctypes.data), 'pose_solve_host')
            return euler, alpha
        p = _dev_f64(pred3d.reshape(n, -1), dev)
        euler = torch.empty(n, 3, dtype=torch.float64, device=dev)
        alpha = torch.empty(n, dtype=torch.float64, device=dev)
        kx = _dev_f64(kpt_x, dev) if kpt_x is not None else None
        fx, cx = (float(K[0, 0]), float(K[0, 2])) if K is not None else (1.0, 0.0)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().egn_pose_solve_f64(_lib.ptr(p), n, _lib.ptr(kx), fx, cx, amode,
                                                     _lib.ptr(euler), _lib.ptr(alpha),
                                                     _lib.current_stream(dev)), 'pose_solve')
        return euler.cpu().numpy(), alpha.cpu().numpy()

    # ------------------------------------------------------------------
    # reprojection refinement of the lifted cuboid (the reference's pnp_refine, transformation.py:143-157, without cv2)
    # ------------------------------------------------------------------
    @staticmethod
    def _intrinsics(K, n, device=None):
        """K [3,3] | [n,3,3] -> [n,4] float64 rows (fx, fy, cx, cy); a device tensor when ``device`` is given."""
        if device is None:
            K = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64)
        else:
            K = _dev_f64(K, device)
        if tuple(K.shape) not in ((3, 3), (n, 3, 3)):
            raise ValueError('K must be [3,3] or [n,3,3], got %s' % (tuple(K.shape),))
        K = K.reshape(-1, 3, 3)
        rows = [K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]]
        intr = np.stack(rows, 1) if device is None else torch.stack(rows, 1)
        if len(intr) != n:
            intr = np.tile(intr, (n, 1)) if device is None else intr.expand(n, 4)
        return np.ascontiguousarray(intr) if device is None else intr.contiguous()

    @staticmethod
    def _refine_device(shape, kpts_2d, intr, roots, weights, max_shift):
        """One launch of egn_pnp_refine_f64 on the current stream of ``shape``'s device; no synchronisation."""
        dev = shape.device
        n = shape.shape[0]
        J = shape.shape[1] + 1
        shape = _dev_f64(shape, dev)
        k = _dev_f64(kpts_2d, dev).reshape(n, J, 2)
        r0 = None if roots is None else _dev_f64(roots, dev).reshape(n, 3)
        w = None if weights is None else _dev_f64(weights, dev).reshape(n, J)
        out = {'kpts_3d_refined': torch.empty(n, J, 3, dtype=torch.float64, device=dev),
               'rt': torch.empty(n, 12, dtype=torch.float64, device=dev),
               'cost': torch.empty(n, 2, dtype=torch.float64, device=dev),
               'iters': torch.empty(n, dtype=torch.int32, device=dev),
               'status': torch.empty(n, dtype=torch.int32, device=dev),
               'dims': torch.empty(n, 3, dtype=torch.float64, device=dev)}
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().egn_pnp_refine_f64(
                _lib.ptr(shape), _lib.ptr(k), _lib.ptr(intr), _lib.ptr(w), _lib.ptr(r0), n, J, float(max_shift),
                _lib.ptr(out['kpts_3d_refined']), _lib.ptr(out['rt']), _lib.ptr(out['cost']), _lib.ptr(out['iters']),
                _lib.ptr(out['status']), _lib.ptr(out['dims']), _lib.current_stream(dev)), 'pnp_refine')
        return out

    @staticmethod
    def _refine_host(shape, kpts_2d, intr, roots, weights, max_shift):
        """The host twin (egn_pnp_refine_host_f64, the same pnp_math.h) on numpy arrays."""
        def arr(a, shp):
            a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
            return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shp))
        n = len(shape)
        shape = arr(shape, (n, -1, 3))
        J = shape.shape[1] + 1
        k = arr(kpts_2d, (n, J, 2))
        r0 = None if roots is None else arr(roots, (n, 3))
        w = None if weights is None else arr(weights, (n, J))
        out = {'kpts_3d_refined': np.empty((n, J, 3)), 'rt': np.empty((n, 12)), 'cost': np.empty((n, 2)),
               'iters': np.empty(n, dtype=np.int32), 'status': np.empty(n, dtype=np.int32), 'dims': np.empty((n, 3))}
        _lib.check(_lib.lib().egn_pnp_refine_host_f64(
            shape.ctypes.data, k.ctypes.data, intr.ctypes.data, None if w is None else w.ctypes.data,
            None if r0 is None else r0.ctypes.data, n, J, float(max_shift), out['kpts_3d_refined'].ctypes.data,
            out['rt'].ctypes.data, out['cost'].ctypes.data, out['iters'].ctypes.data, out['status'].ctypes.data,
            out['dims'].ctypes.data), 'pnp_refine_host')
        return out

    def refine_pnp(self, kpts_3d, kpts_2d, K, roots=None, weights=None, max_shift=5.0):
        """Fit each lifted cuboid rigidly to its own screen key points: minimise the (weighted) squared reprojection
        error over a rotation and a translation, from R = I and T = ``roots`` (default: a weak-perspective start).
          kpts_3d [n,J-1,3] shape relative to the root; kpts_2d [n,J,2] | [n,2J], key point 0 = the root's;
          K [3,3] | [n,3,3]; roots [n,3]; weights [n,J] (0 drops a correspondence);
          max_shift: a fit whose root moved further than this from ``roots`` is discarded (status 0).
        Returns ``kpts_3d_refined`` [n,J,3] (camera coordinates, root first), ``rt`` [n,12] (R row-major, T),
        ``cost`` [n,2] (squared pixel error before / after), ``iters`` [n], ``status`` [n] (1 refined, 0 discarded
        by ``max_shift``, -1 not usable; for 0 / -1 the unrefined placement comes back) and ``dims`` [n,3] = (l, h, w).
        CUDA tensors in give CUDA tensors out: one launch on the current stream, no synchronisation.  numpy inputs
        (or CPU tensors) run the same arithmetic on the host and give numpy arrays.
        This is the optimum of the objective from the prediction, not cv2.solvePnP's result: on an instance with
        several minima the two can differ."""
        if torch.is_tensor(kpts_3d) and kpts_3d.is_cuda:
            n = kpts_3d.shape[0]
            shape = kpts_3d.reshape(n, -1, 3)
            return self._refine_device(shape, kpts_2d, self._intrinsics(K, n, kpts_3d.device), roots, weights,
                                       max_shift)
        n = len(kpts_3d)
        return self._refine_host(kpts_3d, kpts_2d, self._intrinsics(K, n), roots, weights, max_shift)

    def _refine_record(self, record, max_shift):
        """``refine=True`` of gather_lifting_results: initial roots from the record's 3-D boxes where it has usable
        ones (box centre = locations - (0, h/2, 0), car_instance.py:734-739, 761), else the weak-perspective start.
        A CUDA model runs the kernel, a CPU model the host twin (like ``_pose``)."""
        if 'K' not in record:
            raise ValueError("refine needs record['K']")
        shape = np.asarray(record['kpts_3d_pred'], dtype=np.float64)
        n = len(shape)
        shape = shape.reshape(n, -1, 3)
        k2d = np.concatenate([np.asarray(k, dtype=np.float64).reshape(1, -1) for k in record['kpts_2d_pred']])
        rows = record.get('raw_txt_format')
        has_box = np.zeros(n, dtype=bool)
        roots = np.zeros((n, 3))
        if rows is not None and len(rows) == n:
            for i, r in enumerate(rows):
                if 'locations' in r and 'dimensions' in r and r['locations'][2] > 0:
                    has_box[i] = True
                    roots[i] = (r['locations'][0], r['locations'][1] - 0.5 * r['dimensions'][1], r['locations'][2])
        dev = next(self.parameters()).device
        intr = self._intrinsics(record['K'], n)

        def run(sel, r0):
            if dev.type != 'cuda':
                return self._refine_host(shape[sel], k2d[sel], intr[sel], r0, None, max_shift)
            out = self._refine_device(_dev_f64(shape[sel], dev), k2d[sel], _dev_f64(intr[sel], dev), r0, None,
                                      max_shift)
            return {k: v.cpu().numpy() for k, v in out.items()}
        if has_box.all() or not has_box.any():      # the usual case: one call
            return run(slice(None), roots if has_box.all() and n else None)
        with_box, without = run(has_box, roots[has_box]), run(~has_box, None)
        out = {}
        for key, a in with_box.items():
            out[key] = np.empty((n,) + a.shape[1:], dtype=a.dtype)
            out[key][has_box], out[key][~has_box] = a, without[key]
        return out

    @staticmethod
    def _wrap(alpha):
        while alpha > math.pi:
            alpha -= math.pi * 2
        while alpha < -math.pi:
            alpha += math.pi * 2
        return alpha

    def get_observation_angle_trans(self, euler_angles, translations):
        """egonet.py:203-217 (host, trivial)."""
        return np.array([self._wrap(e[1] - math.atan2(-t[2], t[0]) - 0.5 * math.pi)
                         for e, t in zip(euler_angles, translations)])

    def get_observation_angle_proj(self, euler_angles, kpts, K):
        """egonet.py:219-236 (host, trivial)."""
        f, cx = K[0, 0], K[0, 2]
        return np.array([self._wrap(e[1] - math.atan2(-f, k[0, 0] - cx) - 0.5 * math.pi)
                         for e, k in zip(euler_angles, kpts)])

    def gather_lifting_results(self, record, alpha_mode='trans', get_str=False, refine=False, max_shift=5.0):
        """egonet.py:297-339 without plotting.  ``refine``: the reference's switch (egonet.py:297-311 with the flow of
        tools/inference_legacy.py:518-547) -- the lifted cuboid is fitted to ``record['kpts_2d_pred']`` under
        ``record['K']`` first (``refine_pnp``); angles come from the refined points, ``translation`` is the refined
        root, and the record gains ``kpts_3d_refined``, ``refine_status`` and ``refine_dims``."""
        if refine:
            ref = self._refine_record(record, max_shift)
            refined = ref['kpts_3d_refined']
            record['kpts_3d_refined'], record['refine_status'] = refined, ref['status']
            record['refine_dims'], record['refine_rt'] = ref['dims'], ref['rt']
            record['euler_angles'], _ = self.get_6d_rep(refined[:, 1:] - refined[:, :1])
            record['translation'] = refined[:, 0, :].copy()
        else:
            record['euler_angles'], record['translation'] = self.get_6d_rep(record['kpts_3d_pred'])
        if alpha_mode == 'trans':
            record['alphas'] = self.get_observation_angle_trans(record['euler_angles'],
                                                                record['translation'])
        elif alpha_mode == 'proj':
            record['alphas'] = self.get_observation_angle_proj(record['euler_angles'],
                                                               record['kpts_2d_pred'], record['K'])
        else:
            raise NotImplementedError
        if get_str:
            record['pred_str'] = get_pred_str(record)
        return record

    def post_process(self, records, visualize=False, color_dict=None, save_dict=None,
                     alpha_mode='trans', refine=False, max_shift=5.0, images=None, gt_rows=None):
        """egonet.py:385-408 (+ plot_one_image :341-383): pose angles
        per image and, with ``save_dict = {'flag': True, 'save_dir': ...}``, one KITTI
        result file per image (needs ``raw_txt_format`` in the record).  ``refine`` / ``max_shift``: see
        ``gather_lifting_results``.
        ``visualize``: draw every record on its frame (``draw_records``); ``images`` optionally maps a path to its
        [H,W,3] uint8 RGB frame (array or CUDA tensor), ``gt_rows`` a path to label rows for the top view."""
        save = bool(save_dict and save_dict.get('flag'))
        for path in records:
            records[path] = self.gather_lifting_results(records[path], alpha_mode=alpha_mode, get_str=save,
                                                        refine=refine, max_shift=max_shift)
            if save:
                save_txt_file(path, records[path], save_dict)
        if visualize and records:
            self.draw_records(records, color_dict, save_dict, images, gt_rows)
        return records

    def draw_records(self, records, color_dict=None, save_dict=None, images=None, gt_rows=None):
        """``post_process(visualize=True)``, for records that have their angles: 2-D boxes, projected cuboids and key points on every frame
        (visualization.build_primitives) and a top view for records with placed boxes (build_bev_primitives), all
        frames and canvases of the call in ONE launch of the rasteriser (csrc/overlay.hip).  A CUDA model draws on the
        device -- frames that are not there yet are uploaded, the drawn ones read back -- a CPU model runs the host
        twin (like ``_pose``).  Sets ``records[path]['plots'] = {'image': uint8 [H,W,3], 'bev': uint8 [h,w,3] or
        None}`` (numpy; the key the reference keeps its figures under) and, with ``save_dict['vis_dir']``, writes
        ``<vis_dir>/<stem>.png`` and ``<stem>_bev.png``.  The frames in ``images`` are not modified."""
        import os
        from ..common import crop_gpu
        from ..visualization import OverlayRenderer, build_bev_primitives, build_primitives
        dev = next(self.parameters()).device
        frames, prims, colors, ranges, slots, n_prims = [], [], [], [], [], 0

        def add(frame, p, c):
            nonlocal n_prims
            frames.append(frame)
            prims.append(p)
            colors.append(c)
            ranges.append((n_prims, n_prims + len(p)))
            n_prims += len(p)
        for path, rec in records.items():
            img = images[path] if images is not None and path in images else crop_gpu.load_rgb(path)
            if dev.type == 'cuda':
                img = torch.as_tensor(img).to(dev, copy=True).contiguous()
            else:
                img = np.ascontiguousarray(img.cpu().numpy() if torch.is_tensor(img) else img)
            add(img, *build_primitives(rec, color_dict))
            slots.append((path, 'image'))
            p, c, (h, w), n = build_bev_primitives(rec, gt_rows=None if gt_rows is None else gt_rows.get(path),
                                                   color_dict=color_dict)
            if n:
                canvas = torch.full((h, w, 3), 255, dtype=torch.uint8, device=dev)
                add(canvas if dev.type == 'cuda' else canvas.numpy(), p, c)
                slots.append((path, 'bev'))
        if not hasattr(self, '_overlay') or self._overlay.device != dev:
            self._overlay = OverlayRenderer(dev)
        drawn = self._overlay.draw(frames, np.concatenate(prims), np.concatenate(colors), ranges)
        for rec in records.values():
            rec['plots'] = {'image': None, 'bev': None}
        for (path, key), frame in zip(slots, drawn):
            records[path]['plots'][key] = frame.cpu().numpy() if torch.is_tensor(frame) else frame
        vis_dir = save_dict.get('vis_dir') if save_dict else None
        if vis_dir:
            from PIL import Image
            os.makedirs(vis_dir, exist_ok=True)
            for path, rec in records.items():
                stem = os.path.splitext(os.path.basename(path))[0]
                Image.fromarray(rec['plots']['image']).save(os.path.join(vis_dir, stem + '.png'))
                if rec['plots']['bev'] is not None:
                    Image.fromarray(rec['plots']['bev']).save(os.path.join(vis_dir, stem + '_bev.png'))

    # ------------------------------------------------------------------
    # crop extraction (adjacent to the hot path; needs cv2 like the reference)
    # ------------------------------------------------------------------
    def make_records(self, annot_dict):
        """Per-instance records from an annotation dict (egonet.py:105-155
        minus the image work)."""
        width, height = self.resolution
        target_ar = height / width
        records = []
        for i, path in enumerate(annot_dict['path']):
            boxes = annot_dict['boxes'][i]
            labels = annot_dict['labels'][i] if 'labels' in annot_dict else -np.ones(len(boxes), dtype=np.int64)
            scores = annot_dict['scores'][i] if 'scores' in annot_dict else -np.ones(len(boxes))
            for j, bbox in enumerate(boxes):
                bbox = to_npy(bbox)
                ret = modify_bbox(bbox, target_ar)
                records.append({'path': path, 'center': ret['c'], 'scale': ret['s'], 'bbox': bbox,
                                'bbox_resize': ret['bbox'], 'rotation': 0., 'label': labels[j],
                                'score': scores[j]})
        return records

    def forward(self, annot_dict, images=None):
        """egonet.py:488-504.  Instances are cropped on the GPU (common/crop_gpu.py: one
        launch per image for warp + ToTensor + Normalize); ``images`` optionally maps a
        path to an [H,W,3] uint8 RGB array, otherwise the files are read with PIL.
        When the caller has set ``pth_trans`` (tools/inference.py:147) and cv2 is
        importable, the reference's host-side cv2 route is used instead."""
        if self.pth_trans is not None:
            from ..common import crop_cv2
            instances, records = crop_cv2.crop_instances(self, annot_dict)
        else:
            from ..common import crop_gpu
            instances, records = crop_gpu.crop_instances(self, annot_dict, images)
        recs = self.get_keypoints(instances, records)
        recs = self.lift_2d_to_3d(recs)
        for idx, path in enumerate(annot_dict['path']):
            for k_src, k_dst in (('boxes', 'boxes'), ('kpts', 'kpts_2d_gt'), ('kpts_3d_gt', 'kpts_3d_gt'),
                                 ('pose_vecs_gt', 'pose_vecs_gt'), ('kpts_3d_before', 'kpts_3d_before')):
                if k_src in annot_dict and path in recs:
                    recs[path][k_dst] = to_npy(annot_dict[k_src][idx])
            for k in ('raw_txt_format', 'K'):
                if k in annot_dict and path in recs:
                    recs[path][k] = annot_dict[k][idx]
        return recs
