"""Lifter training pairs: KITTI labels + calibration -> the (2-D key points, 3-D cuboid) rows ``LifterTrainStep``
trains on, built on the device and left there.

It reproduces the reference's ``2dto3d`` data set (libs/dataset/KITTI/car_instance.py:1051-1086 ->
``get_2d_3d_pair`` :902-1010 -> ``augment_pose_vector`` :611-644, ``get_cam_cord`` :749-790,
``construct_box_3d`` :730-747; then ``SupervisedDataset.normalize``, basic_classes.py:26-44): per labelled car
a 33-point cuboid, ``lft_aug_times`` random pose augmentations, rotation, translation, projection with the frame's
own intrinsics, the visibility filter, the column statistics that become ``LS.npy`` and the normalisation.

Split of work.  Host: the two text parsers, ``K`` / ``shift`` per frame in float32 like the reference
(``shift = inv(K) @ P[:, 3]``), and the random draws -- ONE ``rng.randn(A, 7T + 1)`` whose stream equals the
reference's per-label calls (``randn(T, 3)``, ``randn(T, 3)``, then ``T + 1`` single draws), so the same seed
gives the reference's pairs.  Device (csrc/lifter_pairs.hip): every sample of every label, the filter, a stable
compaction, the statistics (float64 sums, fixed order), the normalisation and the per-batch row fetch.  The
draws are an input of the kernel: a device-side generator can replace the producer without a new kernel.

``LifterPairs.device_loader`` replaces the ``DataLoader``: it consumes the global torch generator exactly like
``DataLoader(dataset, batch_size, shuffle=shuffle)`` does (one ``int64`` base seed per epoch, then a
``randperm`` of a private generator seeded with it), uploads the epoch's index once and fetches every batch with
two launches of ``egn_gather_rows_f32``.
"""
import numpy as np
import torch

from .. import _lib

# column order of a KITTI label line (car_instance.py:42-56): the dimensions are stored h, w, l
FIELDNAMES = ['type', 'truncated', 'occluded', 'alpha', 'xmin', 'ymin', 'xmax', 'ymax', 'dh', 'dw', 'dl',
              'lx', 'ly', 'lz', 'ry']
_COL = {k: i for i, k in enumerate(FIELDNAMES)}
LABEL_COLUMNS = ('dl', 'dh', 'dw', 'lx', 'ly', 'lz', 'ry')      # -> l h w x y z rot_y, the order of a label row


def parse_label_text(text, classes, with_alpha=False):
    """Label rows [n,7] float64 (l, h, w, x, y, z, rot_y) of the lines whose type is in ``classes``
    (csv_read_annot, car_instance.py:792-829: space separated, other classes skipped).  ``with_alpha``: the pair
    (rows, alpha [n] float64), for ``common.pose_annot``."""
    rows, alpha = [], []
    for line in text.splitlines():
        f = line.split(' ')
        if not f or f[0] not in classes:
            continue
        rows.append([float(f[_COL[k]]) for k in LABEL_COLUMNS])
        if with_alpha:
            alpha.append(float(f[_COL['alpha']]))
    rows = np.array(rows, dtype=np.float64).reshape(-1, 7)
    return (rows, np.array(alpha, dtype=np.float64)) if with_alpha else rows


def parse_calib_text(text):
    """The ``P2:`` row as a [3,4] float32 matrix (csv_read_calib, car_instance.py:831-843)."""
    for line in text.splitlines():
        f = line.split(' ')
        if f[0] == 'P2:':
            return np.array([float(v) for v in f[1:] if v != ''], dtype=np.float32).reshape(3, 4)
    raise ValueError('no P2: row in the calibration text')


def read_label_file(path, classes):
    with open(path, 'r') as fh:
        return parse_label_text(fh.read(), classes)


def read_calib_file(path):
    with open(path, 'r') as fh:
        return parse_calib_text(fh.read())


def frame_row(P, size):
    """[14] float64 of a frame: K (row major), shift, width, height -- K and shift as the reference computes them
    (car_instance.py:841, 931-936): P float32, K = P[:, :3], shift = inv(K) @ P[:, 3] in float32, then widened."""
    P = np.asarray(P, dtype=np.float32).reshape(3, 4)
    K = P[:, :3]
    shift = np.linalg.inv(K) @ P[:, 3].reshape(3, 1)
    return np.concatenate([K.astype(np.float64).reshape(-1), shift.astype(np.float64).reshape(-1),
                           [float(size[0]), float(size[1])]])


def epoch_indices(n, shuffle):
    """The row order ``DataLoader(dataset, shuffle=shuffle)`` yields for the current state of the global torch
    generator, consuming it the same way: the iterator draws its base seed (dataloader.py, ``_BaseDataLoaderIter``),
    then ``RandomSampler`` draws its own seed and permutes with a private generator (sampler.py)."""
    torch.empty((), dtype=torch.int64).random_()                  # the iterator's _base_seed
    if not shuffle:
        return torch.arange(n, dtype=torch.int64)
    seed = int(torch.empty((), dtype=torch.int64).random_().item())
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g)


def _gather(src, idx, out):
    _lib.check(_lib.lib().egn_gather_rows_f32(_lib.ptr(src), src.shape[0], src.shape[1], _lib.ptr(idx), idx.numel(),
                                              _lib.ptr(out), _lib.current_stream(src.device)), 'gather rows')
    return out


class DeviceLoader(object):
    """Iterable over ``(data, target, weights, meta)`` batches of a ``LifterPairs`` set, ``drop_last=False``; see
    the module docstring for the order contract.  ``weights`` is the reference's empty array collated
    ([batch, 0, 1] float64, host), ``meta['roots']`` the batch's roots where the set keeps them."""

    def __init__(self, dataset, batch_size, shuffle):
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), bool(shuffle)
        if self.batch_size <= 0:
            raise ValueError('batch_size must be positive')

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        ds = self.dataset
        n = len(ds)
        order = epoch_indices(n, self.shuffle)
        dev = ds.input.device
        # the device context is entered around the launches only: a generator that yields inside it would leave the
        # consumer on this device between batches
        with torch.cuda.device(dev):
            order_d = order.pin_memory().to(dev, non_blocking=True)          # one index upload per epoch
        roots = ds.root_list[order.numpy()] if ds.root_list is not None else None     # once per epoch, host
        for b in range(0, n, self.batch_size):
            idx = order_d[b:b + self.batch_size]
            m = idx.numel()
            data = torch.empty(m, ds.input.shape[1], dtype=torch.float32, device=dev)
            target = torch.empty(m, ds.output.shape[1], dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _gather(ds.input, idx, data)
                _gather(ds.output, idx, target)
            meta = {'roots': roots[b:b + m]} if roots is not None else {}
            yield data, target, torch.zeros(m, 0, 1, dtype=torch.float64), meta


class LifterPairs(object):
    """The data set: ``input [N,2J]`` / ``output [N,3(J-1)|3J]`` CUDA float32, ``root_list [N,3]`` host float64
    ('R3d' only, like the reference), ``keep`` (host bool over all generated samples), ``statistics`` after
    ``normalize``."""

    def __init__(self, input, output, roots, keep, out_rep):
        self.input, self.output = input, output
        self.keep = keep
        self.out_rep = out_rep
        self.root_list = roots if out_rep == 'R3d' else None      # the reference keeps root_list for 'R3d' only
        self.num_joints = int(input.shape[1] // 2)
        self.total_data = int(input.shape[0])
        self.statistics = None
        self._stats_dev = None

    def __len__(self):
        return self.total_data

    def get_input_output_size(self):
        return int(self.input.shape[1]), int(self.output.shape[1])

    def column_statistics(self, x):
        """(mean, std) [C] CUDA float32 of the rows of ``x``: float64 sums in a fixed order on the device."""
        L = _lib.lib()
        C = x.shape[1]
        nb = L.egn_col_mean_std_ws_bytes(C)
        if nb < 0:
            raise ValueError('column statistics: %d columns (at most 128)' % C)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        std = torch.empty(C, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(L.egn_col_mean_std_f32(_lib.ptr(x), x.shape[0], C, _lib.ptr(ws), nb, _lib.ptr(mean),
                                              _lib.ptr(std), _lib.current_stream(x.device)), 'column statistics')
        return mean, std

    def normalize(self, statistics=None):
        """basic_classes.py:26-44: with the set's own statistics (train) or the given ones (valid,
        car_instance.py:1329).  ``statistics`` holds four [1,n] arrays; they are used as float32."""
        if self.statistics is not None:
            raise RuntimeError('the set is normalised already')
        dev = self.input.device
        if statistics is None:
            mi, si = self.column_statistics(self.input)
            mo, so = self.column_statistics(self.output)
            host = [t.cpu().numpy().reshape(1, -1) for t in (mi, si, mo, so)]
            statistics = {'mean_in': host[0], 'std_in': host[1], 'mean_out': host[2], 'std_out': host[3]}
        else:
            for key, n in (('mean_in', self.input.shape[1]), ('std_in', self.input.shape[1]),
                           ('mean_out', self.output.shape[1]), ('std_out', self.output.shape[1])):
                if np.asarray(statistics[key]).size != n:
                    raise ValueError('statistics[%r] has %d values, the rows have %d'
                                     % (key, np.asarray(statistics[key]).size, n))
            mi, si, mo, so = (torch.from_numpy(np.ascontiguousarray(statistics[k], dtype=np.float32).reshape(-1)).to(dev)
                              for k in ('mean_in', 'std_in', 'mean_out', 'std_out'))
        L = _lib.lib()
        with torch.cuda.device(dev):
            st = _lib.current_stream(dev)
            _lib.check(L.egn_normalize_rows_f32(_lib.ptr(self.input), self.input.shape[0], self.input.shape[1],
                                                _lib.ptr(mi), _lib.ptr(si), st), 'normalise inputs')
            _lib.check(L.egn_normalize_rows_f32(_lib.ptr(self.output), self.output.shape[0], self.output.shape[1],
                                                _lib.ptr(mo), _lib.ptr(so), st), 'normalise outputs')
        self.statistics = statistics
        self._stats_dev = (mi, si, mo, so)          # alive until the launches above have run
        return self

    def unnormalize(self, data, mean, std):
        return data * std + mean                    # operations.py:50-52

    def __getitem__(self, idx):
        """The reference's item (car_instance.py:1241-1247), host numpy: for code that still indexes the set."""
        meta = {}
        if self.root_list is not None:
            meta['roots'] = self.root_list[idx]
        return self.input[idx].cpu().numpy(), self.output[idx].cpu().numpy(), np.zeros((0, 1)), meta

    def device_loader(self, batch_size, shuffle):
        return DeviceLoader(self, batch_size, shuffle)


class LifterPairBuilder(object):
    """``builder(records, rng=np.random)`` -> ``LifterPairs`` (not yet normalised).

    A record is ``{'labels': [n,7] (l, h, w, x, y, z, rot_y), 'P': [3,4], 'size': (width, height), 'path': str}``;
    ``'label_path'`` / ``'calib_path'`` may stand in for ``'labels'`` / ``'P'``."""

    def __init__(self, cfgs, split='train', device=None):
        ds = cfgs['dataset']
        style = ds.get('3d_kpt_sample_style', 'bbox9')
        if style != 'bbox9':
            raise NotImplementedError('3d_kpt_sample_style %r: the reference builds the 9-point cuboid only '
                                      '(car_instance.py:734-736)' % (style,))
        interp = ds.get('interpolate') or {}
        if not interp.get('flag', True):
            raise NotImplementedError('interpolate.flag false: 9-point rows (car_instance.py:741) are not built')
        if interp.get('style', 'bbox12') != 'bbox12':
            raise NotImplementedError('interpolate.style %r: the size-aware styles are unreachable in the reference '
                                      '(car_instance.py:745, dimension= is commented out)' % (interp.get('style'),))
        self.coef = [float(c) for c in interp.get('coef', [0.332, 0.667])]
        if len(self.coef) not in (1, 2):
            raise NotImplementedError('interpolate.coef with %d entries (1 or 2; car_instance.py:727)' % len(self.coef))
        if ds.get('lft_in_rep', 'coordinates2d') != 'coordinates2d':
            raise NotImplementedError('lft_in_rep %r (car_instance.py:654-661): coordinates2d only'
                                      % (ds.get('lft_in_rep'),))
        self.out_rep = ds.get('lft_out_rep', 'R3d')
        if self.out_rep not in ('R3d', 'R3d+T'):
            raise NotImplementedError('lft_out_rep %r (car_instance.py:663-685)' % (self.out_rep,))
        ts = cfgs.get('training_settings', {}) or {}
        aug = ts['lft_aug'] if 'lft_aug' in ts else ds.get('lft_aug', False)
        times = ts['lft_aug_times'] if 'lft_aug_times' in ts else ds.get('lft_aug_times', 1)
        self.split = split
        self.augment = bool(aug) and split == 'train'                   # car_instance.py:1063
        self.T = int(times) if self.augment else 0
        self.yaw_draws = split == 'train'                               # car_instance.py:767-768
        self.classes = tuple(ds.get('detect_classes', ['Car']))
        self.num_joints = 9 + 12 * len(self.coef)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)

    def gather(self, records):
        """(labels [A,7] f64, label_frame [A] int32, frames [F,14] f64) in record order; frames with no label of the
        classes contribute nothing."""
        labels, lf, frames = [], [], []
        for f, rec in enumerate(records):
            lab = rec['labels'] if 'labels' in rec else read_label_file(rec['label_path'], self.classes)
            lab = np.asarray(lab, dtype=np.float64).reshape(-1, 7)
            P = rec['P'] if 'P' in rec else read_calib_file(rec['calib_path'])
            frames.append(frame_row(P, rec['size']))
            labels.append(lab)
            lf.append(np.full(len(lab), f, dtype=np.int32))
        if not labels or sum(len(x) for x in labels) == 0:
            raise ValueError('the records hold no label of %s' % (self.classes,))
        return np.concatenate(labels), np.concatenate(lf), np.stack(frames)

    def draw(self, n_labels, rng=np.random):
        """[A, 7T+1] float64: per label T x 3 rotation, T x 3 translation and T + 1 yaw draws, in the order the
        reference consumes the generator (car_instance.py:634-637, 768); None for a split that draws nothing."""
        if not self.yaw_draws:
            return None
        return rng.randn(n_labels, 7 * self.T + 1)

    def __call__(self, records, rng=np.random):
        labels, lf, frames = self.gather(records)
        draws = self.draw(len(labels), rng)
        return self.build(labels, lf, frames, draws)

    def build(self, labels, label_frame, frames, draws):
        A, T, J = len(labels), self.T, self.num_joints
        label_frame = np.asarray(label_frame)
        if len(label_frame) != A or label_frame.min() < 0 or label_frame.max() >= len(frames):
            raise ValueError('label_frame must hold one index into the %d frames per label' % len(frames))
        S = T + 1
        L = _lib.lib()
        nb = L.egn_lifter_pairs_ws_bytes(A, T)
        if nb < 0:
            raise ValueError('%d labels x %d samples: more than 2^31 - 1 samples in one build, split the records'
                             % (A, S))
        dev = self.device
        NS = A * S
        OC = 3 * J if self.out_rep == 'R3d+T' else 3 * (J - 1)
        with torch.cuda.device(dev):
            up = [torch.from_numpy(np.ascontiguousarray(labels, dtype=np.float64)),
                  torch.from_numpy(np.ascontiguousarray(label_frame, dtype=np.int32)),
                  torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float64))]
            if draws is not None:
                draws = np.ascontiguousarray(draws, dtype=np.float64)
                if draws.shape != (A, 7 * T + 1):
                    raise ValueError('draws must be [%d, %d], got %s' % (A, 7 * T + 1, draws.shape))
                up.append(torch.from_numpy(draws))
            up = [t.to(dev) for t in up]
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            in2d = torch.empty(NS, 2 * J, dtype=torch.float32, device=dev)
            out3d = torch.empty(NS, OC, dtype=torch.float32, device=dev)
            roots = torch.empty(NS, 3, dtype=torch.float64, device=dev)
            c1 = self.coef[1] if len(self.coef) > 1 else 0.0
            _lib.check(L.egn_lifter_pairs_f64(_lib.ptr(up[0]), _lib.ptr(up[1]), A, _lib.ptr(up[2]), len(frames),
                                              _lib.ptr(up[3]) if draws is not None else None, T, self.coef[0], c1,
                                              len(self.coef), 1 if self.out_rep == 'R3d+T' else 0, _lib.ptr(ws), nb,
                                              _lib.ptr(in2d), _lib.ptr(out3d), _lib.ptr(roots),
                                              _lib.current_stream(dev)), 'lifter pairs')
            n = int(ws[:8].view(torch.int64).item())                    # the one read-back of the build
            keep = ws[nb - NS:].cpu().numpy().astype(bool)
        if n == 0:
            raise ValueError('no sample passed the visibility filter')
        # the rows are views of the buffers sized for all samples: the dropped share is small and a copy of ~1 GB
        # would cost more than it frees
        return LifterPairs(in2d[:n], out3d[:n], roots[:n].cpu().numpy() if self.out_rep == 'R3d' else None, keep,
                           self.out_rep)
