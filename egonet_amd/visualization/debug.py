"""The training debug pictures of the reference's ``libs/visualization/debug.py`` with its names and arguments: per
report batch the grid of crops with predicted and ground-truth key points (``<epoch>_<batch>_keypoints.jpg``) and the
heat-map mosaics of the targets and of the prediction (``_hm_gt.jpg``, ``_hm_pred.jpg``).

CUDA tensors are composed on the device (csrc/debug_pictures.hip: the range of the crops, the grid, the mosaic; the
markers through ``OverlayRenderer``, drawn in place), and the finished uint8 pictures travel to a background writer in
one pinned, asynchronous copy.  CPU tensors and numpy arrays go through the host twins of the same kernels: the same
bytes.  The pictures follow csrc/debug_pictures_math.h, not cv2's or torchvision's pixels;
colours are true RGB, every joint tile carries its own arg-max marker only and the thumbnail all of them, and the joint
numbers are seven-segment digits built from capsules.
"""
import functools
import math
import os
import queue
import threading

import numpy as np
import torch

from .. import _lib
from .overlay import OverlayRenderer, parse_color

RED, CYAN = (255, 0, 0), (0, 255, 255)
ALIGN = 256                      # byte alignment of each picture inside the block that travels to the host
DIGIT_HEIGHT = 10.0              # pixels, of the joint numbers on the grid


def jet_lut():
    """The 256 x 3 uint8 colour table of the mosaic (RGB): with t = q / 255, channel = floor(255 c + 0.5) for
    c = clamp01(1.5 - |4 t - k|), k = 3 (red), 2 (green), 1 (blue); lut[0] = (0, 0, 128), lut[255] = (128, 0, 0)."""
    t = np.arange(256, dtype=np.float64) / 255.0
    lut = np.empty((256, 3), dtype=np.uint8)
    for ch, k in enumerate((3.0, 2.0, 1.0)):
        c = np.minimum(1.0, np.maximum(0.0, 1.5 - np.abs(4.0 * t - k)))
        lut[:, ch] = np.floor(255.0 * c + 0.5).astype(np.uint8)
    return lut


def grid_layout(n, height, width, nrow=8, padding=2):
    """``make_grid``'s numbers: ``(xmaps, ymaps, picture height, picture width)``."""
    xmaps = min(nrow, n)
    ymaps = int(math.ceil(float(n) / xmaps))
    return xmaps, ymaps, ymaps * (height + padding) + padding, xmaps * (width + padding) + padding


# seven-segment digits on the unit cell x in [0, 1], y in [0, 2] (y down): a top, b / c right, d bottom, e / f left,
# g middle
_SEGMENTS = {'a': ((0, 0), (1, 0)), 'b': ((1, 0), (1, 1)), 'c': ((1, 1), (1, 2)), 'd': ((0, 2), (1, 2)),
             'e': ((0, 1), (0, 2)), 'f': ((0, 0), (0, 1)), 'g': ((0, 1), (1, 1))}
DIGIT_SEGMENTS = {0: 'abcdef', 1: 'bc', 2: 'abged', 3: 'abgcd', 4: 'fgbc', 5: 'afgcd', 6: 'afgedc', 7: 'abc',
                  8: 'abcdefg', 9: 'abcdfg'}


@functools.lru_cache(maxsize=256)
def _digit_rows(number, height):
    """The capsules of ``number`` relative to the origin of its first digit, float64 [P, 6] (cached: read only)."""
    height = float(height)
    half, rad = 0.5 * height, max(0.5, height / 16.0)
    rows = []
    for i, d in enumerate(str(int(number))):
        ox, oy = 0.75 * height * i, -height
        for s in DIGIT_SEGMENTS[int(d)]:
            (u0, v0), (u1, v1) = _SEGMENTS[s]
            rows.append((ox + u0 * half, oy + v0 * half, ox + u1 * half, oy + v1 * half, rad, 1.0))
    return np.asarray(rows, dtype=np.float64).reshape(-1, 6)


def build_digit_primitives(number, x, y, height, colour):
    """The decimal digits of ``number`` >= 0 as capsules -> ``(prims [P,6] float32, colors [P] uint32)``.  (x, y) is
    the bottom-left corner of the first digit (``cv2.putText``'s origin).  A digit cell is ``height / 2`` wide and
    ``height`` high, cells follow each other every ``0.75 height``; segment end point (u, v) of the unit cell of digit
    i lies at ``(x + 0.75 height i + u height / 2, y - height + v height / 2)``; every capsule has radius
    ``max(0.5, height / 16)`` and opacity 1.  Digits left to right, segments in the order of ``DIGIT_SEGMENTS``."""
    rows = _digit_rows(number, height) + np.array([float(x), float(y), float(x), float(y), 0.0, 0.0])
    return rows.astype(np.float32), np.full(len(rows), parse_color(colour), dtype=np.uint32)


def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _place(templates, px, py, ok):
    """``templates``: per joint a float64 [P_j, 6] list relative to the joint's pixel; ``px`` / ``py`` / ``ok`` [n, J]
    -> the rows of all crops, crop by crop and joint by joint, those of joints with ``ok`` False left out."""
    zero = np.zeros_like(px)
    at = np.stack([px, py, px, py, zero, zero], axis=2)                       # [n, J, 6]
    rows = np.concatenate([t[None, :, :] + at[:, j, None, :] for j, t in enumerate(templates)], axis=1)
    keep = np.concatenate([np.repeat(ok[:, j, None], len(t), axis=1) for j, t in enumerate(templates)], axis=1)
    return rows[keep].astype(np.float32)


def build_grid_markers(joints, n_images, height, width, nrow=8, padding=2, colour=RED, add_idx=True, radius=3.0,
                       digit_height=DIGIT_HEIGHT):
    """``draw_circles`` (debug.py:18-48) as primitives: for crop k < min(n_images, len(joints)) in cell
    (k // xmaps, k % xmaps) and every joint, visible or not, a disc at ``(int(cx (W + pad) + pad + x),
    int(cy (H + pad) + pad + y))`` -- truncated like the reference -- and, with ``add_idx``, the joint's number 1..J
    with that point as its origin; crop by crop, joint by joint, the disc before its number.  A joint with a
    non-finite coordinate is left out."""
    joints = _np(joints)
    n = min(n_images, len(joints))
    if n <= 0 or joints.shape[1] == 0:
        return np.zeros((0, 6), dtype=np.float32), np.zeros(0, dtype=np.uint32)
    xy = joints[:n, :, :2].astype(np.float64)
    k = np.arange(n)
    xmaps = min(nrow, n_images)
    xpos = ((k % xmaps) * (width + padding) + padding)[:, None] + xy[:, :, 0]
    ypos = ((k // xmaps) * (height + padding) + padding)[:, None] + xy[:, :, 1]
    ok = np.isfinite(xpos) & np.isfinite(ypos)
    px, py = np.trunc(np.where(ok, xpos, 0.0)), np.trunc(np.where(ok, ypos, 0.0))
    disc = np.array([[0.0, 0.0, 0.0, 0.0, float(radius), 1.0]])
    templates = [np.concatenate([disc, _digit_rows(j + 1, digit_height)]) if add_idx else disc
                 for j in range(xy.shape[1])]
    prims = _place(templates, px, py, ok)
    return prims, np.full(len(prims), parse_color(colour), dtype=np.uint32)


def build_mosaic_markers(preds, map_h, map_w, colour=RED, radius=1.0):
    """The arg-max markers of a mosaic: ``preds`` [n, J, 2] (x, y) in map pixels, as ``get_max_preds`` gives them
    (zeros where the maximum is <= 0).  Per crop i and joint j a disc at the truncated position on the thumbnail
    (tile 0) and one on tile j + 1; no other tile carries joint j's marker."""
    preds = _np(preds).astype(np.float64)
    n, J = preds.shape[:2]
    if n == 0 or J == 0:
        return np.zeros((0, 6), dtype=np.float32), np.zeros(0, dtype=np.uint32)
    ok = np.isfinite(preds[:, :, 0]) & np.isfinite(preds[:, :, 1])
    px = np.trunc(np.where(ok, preds[:, :, 0], 0.0))
    py = np.trunc(np.where(ok, preds[:, :, 1], 0.0)) + (np.arange(n) * map_h)[:, None]
    r = float(radius)
    templates = [np.array([[0.0, 0.0, 0.0, 0.0, r, 1.0], [(j + 1.0) * map_w, 0.0, (j + 1.0) * map_w, 0.0, r, 1.0]])
                 for j in range(J)]
    prims = _place(templates, px, py, ok)
    return prims, np.full(len(prims), parse_color(colour), dtype=np.uint32)


# ---------------------------------------------------------------------------------------------------------------
# composition: the device kernels for CUDA tensors, their host twins for everything else
# ---------------------------------------------------------------------------------------------------------------

def _on_device(t):
    return torch.is_tensor(t) and t.is_cuda


def _images(batch_image):
    """-> (float32 [N, C, H, W] with C >= 3 whose first three planes are the picture: a CUDA tensor or a numpy array,
    C).  A channel slice ``x[:, :3]`` of a contiguous batch is read in place through its batch stride."""
    x = batch_image
    if not _on_device(x):
        x = np.ascontiguousarray(_np(x), dtype=np.float32)
        if x.ndim != 4 or x.shape[1] < 3:
            raise ValueError('debug pictures need [N, C >= 3, H, W] crops, got %s' % (x.shape,))
        return x, x.shape[1]
    if x.dim() != 4 or x.shape[1] < 3:
        raise ValueError('debug pictures need [N, C >= 3, H, W] crops, got %s' % (tuple(x.shape),))
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    n, c, h, w = x.shape
    plane = h * w
    if x.numel() and not x.is_contiguous():
        if x.stride(3) == 1 and x.stride(2) == w and x.stride(1) == plane and x.stride(0) % plane == 0 \
                and x.stride(0) >= c * plane:
            return x, x.stride(0) // plane
        x = x.contiguous()
    return x, c


def _maps(m):
    if _on_device(m):
        m = m.detach()
        return (m if m.dtype == torch.float32 else m.float()).contiguous()
    return np.ascontiguousarray(_np(m), dtype=np.float32)


def _ptr(a):
    return _lib.ptr(a) if torch.is_tensor(a) else a.ctypes.data


def image_range(images, channels, normalize=True):
    """(lo, hi) of the first three planes of all crops, NaNs ignored, as float32 [2]: a device tensor for CUDA crops
    (two launches, no read-back), else a numpy array.  ``normalize=False``: the fixed pair (0, 0.99999), which makes
    the quantiser ``trunc(clamp(255 x))`` to within 1e-9."""
    n, _, h, w = images.shape
    L = _lib.lib()
    if _on_device(images):
        if not normalize:
            return torch.tensor([0.0, 0.99999], dtype=torch.float32, device=images.device)
        lohi = torch.zeros(2, dtype=torch.float32, device=images.device)
        ws = torch.empty(max(8, L.egn_debug_range_ws_bytes(n, 3, h * w)), dtype=torch.uint8, device=images.device)
        with torch.cuda.device(images.device):
            _lib.check(L.egn_debug_range_f32(_lib.ptr(images), n, channels, 3, h * w, _lib.ptr(ws), ws.numel(),
                                             _lib.ptr(lohi), _lib.current_stream(images.device)), 'debug range')
        return lohi
    lohi = np.zeros(2, dtype=np.float32)
    if not normalize:
        lohi[:] = (0.0, 0.99999)
        return lohi
    _lib.check(L.egn_debug_range_host_f32(images.ctypes.data, n, channels, 3, h * w, lohi.ctypes.data), 'debug range')
    return lohi


def compose_grid(images, channels, lohi, out, nrow=8, padding=2):
    """The grid of crops into ``out`` uint8 [gh, gw, 3] (``grid_layout``), of the same kind as ``images``."""
    n, _, h, w = images.shape
    L = _lib.lib()
    if _on_device(images):
        with torch.cuda.device(images.device):
            _lib.check(L.egn_debug_grid_u8(_lib.ptr(images), n, channels, h, w, nrow, padding, _lib.ptr(lohi),
                                           _lib.ptr(out), out.stride(0), _lib.current_stream(images.device)),
                       'debug grid')
    else:
        _lib.check(L.egn_debug_grid_host_u8(images.ctypes.data, n, channels, h, w, nrow, padding, lohi.ctypes.data,
                                            out.ctypes.data, out.strides[0]), 'debug grid')
    return out


def compose_mosaic(images, channels, maps, lohi, lut, out):
    """The heat-map mosaic of ``maps`` [n, J, h, w] over the first n crops into ``out`` uint8 [n h, (J + 1) w, 3]."""
    n, J, h, w = maps.shape
    if n > images.shape[0]:
        raise ValueError('mosaic: %d maps for %d crops' % (n, images.shape[0]))
    H, W = images.shape[2:]
    L = _lib.lib()
    if _on_device(images):
        with torch.cuda.device(images.device):
            _lib.check(L.egn_debug_mosaic_u8(_lib.ptr(images), channels, H, W, _lib.ptr(maps), n, J, h, w,
                                             _lib.ptr(lohi), _lib.ptr(lut), _lib.ptr(out), out.stride(0),
                                             _lib.current_stream(images.device)), 'debug mosaic')
    else:
        _lib.check(L.egn_debug_mosaic_host_u8(images.ctypes.data, channels, H, W, maps.ctypes.data, n, J, h, w,
                                              lohi.ctypes.data, lut.ctypes.data, out.ctypes.data, out.strides[0]),
                   'debug mosaic')
    return out


def max_preds_host(maps):
    """``get_max_preds`` on a numpy [n, J, h, w]: the first flat arg-max as (x, y), zeros where the maximum is <= 0."""
    n, J, h, w = maps.shape
    flat = maps.reshape(n, J, h * w)
    if h * w == 0:
        return np.zeros((n, J, 2), dtype=np.float32)
    idx = flat.argmax(axis=2)
    mx = np.take_along_axis(flat, idx[:, :, None], axis=2)[:, :, 0]
    xy = np.stack([idx % w, idx // w], axis=2).astype(np.float32)
    return xy * (mx > 0)[:, :, None].astype(np.float32)


def _read_back(tensors):
    """Small device tensors -> numpy arrays in ONE copy."""
    if not tensors:
        return []
    flat = torch.cat([t.reshape(-1).float() for t in tensors]).cpu().numpy()
    out, at = [], 0
    for t in tensors:
        out.append(flat[at:at + t.numel()].reshape(tuple(t.shape)))
        at += t.numel()
    return out


# ---------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------

def _encode_jpeg(path, array, quality=95):
    """uint8 [H, W, 3] RGB -> a JPEG file, complete or absent (written beside and renamed)."""
    from PIL import Image
    tmp = path + '.tmp'
    Image.fromarray(np.ascontiguousarray(array), 'RGB').save(tmp, format='JPEG', quality=quality)
    os.replace(tmp, path)


class DebugPictureWriter(object):
    """Encodes and writes finished pictures on one background thread.  At most one report is in flight: a second one
    waits for the first, no picture is dropped.  ``flush()`` waits for the report in flight and raises what it
    raised; ``close()`` flushes and ends the thread."""

    def __init__(self, quality=95):
        self.quality = quality
        self._queue = queue.Queue()
        self._idle = threading.Event()
        self._idle.set()
        self._thread = None
        self._error = None
        self._pinned = None
        self._closed = False
        self.reports = 0

    def _run(self):
        while True:
            job = self._queue.get()
            if job is None:
                return
            event, pictures = job
            try:
                if event is not None:
                    event.synchronize()              # the pinned copy has landed
                for path, array in pictures:
                    _encode_jpeg(path, array, self.quality)
            except BaseException as e:               # kept for the caller: flush() raises it
                self._error = e
            finally:
                self._idle.set()

    def _submit(self, event, pictures):
        if self._closed:
            raise RuntimeError('DebugPictureWriter is closed')
        if self._thread is None:
            self._thread = threading.Thread(target=self._run, name='debug-pictures', daemon=True)
            self._thread.start()
        self._idle.clear()
        self.reports += 1
        self._queue.put((event, pictures))

    def write_host(self, pictures):
        """``pictures``: [(path, uint8 [H, W, 3] numpy array)]; the arrays are the writer's from here on."""
        self.flush()
        self._submit(None, list(pictures))

    def write_device(self, block, entries):
        """``block``: a uint8 CUDA tensor holding the finished pictures; ``entries``: [(path, byte offset, (H, W))].
        One non-blocking copy into the pinned buffer on the current stream, an event behind it; returns at once."""
        self.flush()                                 # the pinned buffer is free again
        n = block.numel()
        if self._pinned is None or self._pinned.numel() < n:
            self._pinned = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        self._pinned[:n].copy_(block, non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(block.device))
        host = self._pinned.numpy()
        self._submit(event, [(path, host[off:off + 3 * h * w].reshape(h, w, 3)) for path, off, (h, w) in entries])

    def flush(self):
        self._idle.wait()
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    def close(self):
        if self._closed:
            return
        try:
            self.flush()
        finally:
            self._closed = True
            if self._thread is not None:
                self._queue.put(None)
                self._thread.join()
                self._thread = None


# ---------------------------------------------------------------------------------------------------------------
# the reference's three functions
# ---------------------------------------------------------------------------------------------------------------

_RENDERERS, _LUTS = {}, {}


def _renderer(device):
    key = str(device)
    if key not in _RENDERERS:
        _RENDERERS[key] = OverlayRenderer(device)
    return _RENDERERS[key]


def _render(batch_image, jobs, writer, normalize=True):
    """``jobs``: dicts with 'path' and either 'maps' (a mosaic) or 'pred' / 'gt' / 'nrow' / 'padding' / 'add_idx' (the
    grid; a tensor among 'pred' / 'gt' is read back with the arg-max positions).  Range once, every picture composed
    into one block, all markers in one overlay launch, one hand-over to the writer."""
    if not jobs:
        return
    images, channels = _images(batch_image)
    N, _, H, W = images.shape
    on_dev = _on_device(images)
    dev = images.device if on_dev else torch.device('cpu')
    shapes = []
    for job in jobs:
        if 'maps' in job:
            job['maps'] = m = _maps(job['maps'])
            if _on_device(m) != on_dev:
                raise ValueError('debug pictures: crops and heat-maps must live on the same side')
            shapes.append((m.shape[0] * m.shape[2], (m.shape[1] + 1) * m.shape[3]))
        else:
            shapes.append(grid_layout(N, H, W, job['nrow'], job['padding'])[2:] if N else (0, 0))
    offsets, total = [], 0
    for h, w in shapes:
        offsets.append(total)
        total += (3 * h * w + ALIGN - 1) // ALIGN * ALIGN
    if on_dev:
        block = torch.empty(total, dtype=torch.uint8, device=dev)
        if str(dev) not in _LUTS:
            _LUTS[str(dev)] = torch.from_numpy(jet_lut()).to(dev)
        lut = _LUTS[str(dev)]
    else:
        block = np.empty(total, dtype=np.uint8)
        lut = jet_lut()
    views = [block[o:o + 3 * h * w].reshape(h, w, 3) for o, (h, w) in zip(offsets, shapes)]
    lohi = image_range(images, channels, normalize)
    wanted = []                                      # device tensors the markers need on the host
    for job, view in zip(jobs, views):
        if view.shape[0] == 0 or view.shape[1] == 0:
            continue
        if 'maps' in job:
            compose_mosaic(images, channels, job['maps'], lohi, lut, view)
            if on_dev:
                from ..common.img_proc import hard_arg_max
                job['preds'] = len(wanted)
                wanted.append(hard_arg_max(job['maps'])[0])
        else:
            compose_grid(images, channels, lohi, view, job['nrow'], job['padding'])
            for key in ('pred', 'gt'):
                if _on_device(job.get(key)):
                    job[key + '_at'] = len(wanted)
                    wanted.append(job[key].detach())
    host = _read_back(wanted)                        # the one small read-back
    prims, cols, ranges, at = [], [], [], 0
    for job, view in zip(jobs, views):
        if 'maps' in job:
            m = job['maps']
            preds = host[job['preds']] if on_dev else max_preds_host(m)
            p, c = build_mosaic_markers(preds, m.shape[2], m.shape[3])
        else:
            parts = []
            for key, colour in (('pred', RED), ('gt', CYAN)):
                if job.get(key) is None:
                    continue
                j = host[job[key + '_at']] if key + '_at' in job else _np(job[key])
                parts.append(build_grid_markers(j, N, H, W, job['nrow'], job['padding'], colour, job['add_idx']))
            p = np.concatenate([q[0] for q in parts]) if parts else np.zeros((0, 6), dtype=np.float32)
            c = np.concatenate([q[1] for q in parts]) if parts else np.zeros(0, dtype=np.uint32)
        prims.append(p)
        cols.append(c)
        ranges.append((at, at + len(p)))
        at += len(p)
    prims, cols = np.concatenate(prims), np.concatenate(cols)
    live = [k for k, v in enumerate(views) if v.shape[0] and v.shape[1]]
    if not live:
        return
    drawn = _renderer(dev).draw([views[k] for k in live], prims, cols, [ranges[k] for k in live])
    own = writer is None
    writer = DebugPictureWriter() if own else writer
    try:
        if on_dev:                                   # drawn in place in the block
            writer.write_device(block, [(jobs[k]['path'], offsets[k], shapes[k]) for k in live])
        else:
            writer.write_host([(jobs[k]['path'], d) for k, d in zip(live, drawn)])
    finally:
        if own:
            writer.close()


def save_batch_image_with_joints(batch_image, record_dict, file_name, nrow=8, padding=2, add_idx=True, writer=None):
    """debug.py:51-81.  ``batch_image`` [N, C >= 3, H, W]; ``record_dict['pred']`` = (joints [N, J, >= 2], visibility)
    in red and, when present, ``record_dict['gt']`` = (joints [n <= N, J, >= 2], visibility) in cyan -- every joint is
    drawn, visible or not, ground truth for the labelled prefix only.  Without a ``writer`` the file exists on
    return."""
    job = {'path': file_name, 'nrow': nrow, 'padding': padding, 'add_idx': add_idx, 'pred': record_dict['pred'][0]}
    if 'gt' in record_dict:
        job['gt'] = record_dict['gt'][0]
    _render(batch_image, [job], writer)


def save_batch_heatmaps(batch_image, batch_heatmaps, file_name, normalize=True, writer=None):
    """debug.py:83-149.  ``batch_heatmaps`` [n <= N, J, h, w]: one row of tiles per map row."""
    _render(batch_image, [{'path': file_name, 'maps': batch_heatmaps}], writer, normalize)


def decode_joints_pred(output, input_size):
    """The predicted joints in crop pixels [N, J, 2] when no metric handed them over: the coordinate head's
    ``coords * input_size`` (``input_size`` = (width, height)), the heat-map head's hard arg-max times input / heat-map
    size.  Of the same kind as ``output``."""
    if type(output) is tuple:
        coords = output[1]
        if torch.is_tensor(coords):
            return coords.detach().float() * torch.tensor([float(input_size[0]), float(input_size[1])],
                                                          dtype=torch.float32, device=coords.device)
        return np.asarray(coords, dtype=np.float32) * np.asarray(input_size, dtype=np.float32).reshape(1, 1, 2)
    h, w = output.shape[2:]
    scale = (float(input_size[0]) / w, float(input_size[1]) / h)
    if _on_device(output):
        from ..common.img_proc import hard_arg_max
        xy = hard_arg_max(output.detach())[0]
        return xy * torch.tensor(scale, dtype=torch.float32, device=xy.device)
    return max_preds_host(_maps(output)) * np.asarray(scale, dtype=np.float32).reshape(1, 1, 2)


def save_debug_images(epoch, batch_index, cfgs, input, meta, target, others, output, split, writer=None):
    """debug.py:151-188: gated by ``training_settings.debug.save`` and its ``save_images_kpts`` / ``save_hms_gt`` /
    ``save_hms_pred``; files ``<dirs.output>/intermediate_results/<split>/<epoch>_<batch>_{keypoints,hm_gt,hm_pred}.jpg``.
    ``others`` may be None or lack 'joints_pred' (``decode_joints_pred``).  ``target`` has the labelled prefix's
    ``n <= N`` rows; ``output`` is the maps or the tuple (maps, coords).  With a ``writer`` the call returns once the
    pictures are on their way (``writer.flush()`` waits for the files), without one the files exist on return."""
    debug_cfgs = cfgs['training_settings']['debug']
    if not debug_cfgs['save']:
        return
    prefix = os.path.join(cfgs['dirs']['output'], 'intermediate_results', split, '{}_{}'.format(epoch, batch_index))
    jobs = []
    if debug_cfgs['save_images_kpts']:
        joints_pred = others.get('joints_pred') if others else None
        if joints_pred is None:
            size = cfgs.get('heatmapModel', {}).get('input_size') or (input.shape[3], input.shape[2])
            joints_pred = decode_joints_pred(output, size)
        job = {'path': '{}_keypoints.jpg'.format(prefix), 'nrow': 8, 'padding': 2, 'add_idx': True, 'pred': joints_pred}
        if meta is not None and 'transformed_joints' in meta:
            job['gt'] = meta['transformed_joints']
        jobs.append(job)
    if debug_cfgs['save_hms_gt']:
        jobs.append({'path': '{}_hm_gt.jpg'.format(prefix), 'maps': target})
    if debug_cfgs['save_hms_pred']:
        jobs.append({'path': '{}_hm_pred.jpg'.format(prefix), 'maps': output[0] if type(output) is tuple else output})
    if jobs:
        os.makedirs(os.path.dirname(prefix), exist_ok=True)
        _render(input, jobs, writer)
