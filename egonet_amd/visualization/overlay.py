"""Predictions drawn on the frames (the reference's ``plot_2d_objects`` / top view, libs/visualization/egonet_utils.py)
without matplotlib or cv2: the host lists capsules -- segments with a radius, a colour and an opacity; a zero-length one
is a disc -- and csrc/overlay.hip rasterises a whole batch of frames in one launch (definition: csrc/overlay_math.h).

    prims  float32 [P, 6]   x0 y0 x1 y1 r a, drawn in list order
    colors uint32  [P]      R | G << 8 | B << 16

Not drawn: text labels (there is no font; the debug pictures' joint numbers are seven-segment capsules,
visualization/debug.py), dash-dot line styles (the ground-truth cuboid is solid green) and the matplotlib 3-D scene.
"""
import math

import numpy as np
import torch

from .. import _lib
from ..common.staging import PinnedStaging

# the reference's plot_3d_bbox.connections: index pairs into the eight cuboid corners (key points 1..8)
CUBOID_EDGES = ((0, 1), (0, 2), (1, 3), (2, 3), (4, 5), (5, 7), (4, 6), (6, 7), (0, 4), (1, 5), (2, 6), (3, 7))
BOX_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0))
_LETTERS = {'r': (255, 0, 0), 'g': (0, 255, 0), 'b': (0, 0, 255), 'c': (0, 255, 255), 'm': (255, 0, 255),
            'y': (255, 255, 0), 'k': (0, 0, 0), 'w': (255, 255, 255)}
DEFAULT_COLORS = {'bbox_2d': 'r', 'kpts': ['ro', 'b']}      # the reference's post_process defaults
GRID_GREY = (211, 211, 211)


def parse_color(c):
    """A matplotlib one-letter code, optionally followed by a marker ('rx', 'ro': the marker is ignored), or an RGB
    triple of 0..255 -> the colour word R | G << 8 | B << 16."""
    if isinstance(c, str):
        if not c or c[0] not in _LETTERS:
            raise ValueError('colour %r: expected one of %s' % (c, ' '.join(_LETTERS)))
        rgb = _LETTERS[c[0]]
    else:
        rgb = tuple(int(v) for v in c)
        if len(rgb) != 3 or min(rgb) < 0 or max(rgb) > 255:
            raise ValueError('colour %r: expected three values in 0..255' % (c,))
    return rgb[0] | rgb[1] << 8 | rgb[2] << 16


class _List(object):
    def __init__(self):
        self.rows, self.cols = [], []

    def segments(self, pts, pairs, radius, col):
        for a, b in pairs:
            self.rows.append((pts[a][0], pts[a][1], pts[b][0], pts[b][1], radius, 1.0))
            self.cols.append(col)

    def discs(self, pts, radius, col):
        for p in pts:
            self.rows.append((p[0], p[1], p[0], p[1], radius, 1.0))
            self.cols.append(col)

    def arrays(self):
        return (np.asarray(self.rows, dtype=np.float32).reshape(-1, 6), np.asarray(self.cols, dtype=np.uint32))


def build_primitives(record, color_dict=None, line_width=2.0, point_radius=2.0):
    """The overlay of one per-image record -> ``(prims, colors)``.  Per instance, in this order: the 2-D box
    ``bbox_resize[i]`` (4 segments, colour ``bbox_2d``), the predicted cuboid (12 segments between key points 1..8 of
    ``kpts_2d_pred[i]``, colour ``bbox_3d``, default ``bbox_2d``'s), the J key points as discs of ``point_radius`` in
    the colour of ``kpts[0]``.  After all instances, the 12 edges of every ground-truth cuboid (``kpts_2d_gt``) in
    green, as plot_2d_objects orders them.  Segments have radius ``line_width / 2``; every opacity is 1."""
    cd = dict(DEFAULT_COLORS if color_dict is None else color_dict)
    c_box = parse_color(cd['bbox_2d'])
    c_cub = parse_color(cd.get('bbox_3d', cd['bbox_2d']))
    kp = cd.get('kpts', DEFAULT_COLORS['kpts'])
    c_kpt = parse_color(kp if isinstance(kp, str) else kp[0])
    rad = 0.5 * float(line_width)
    out = _List()
    for i in range(len(record['kpts_2d_pred'])):
        x1, y1, x2, y2 = (float(v) for v in np.asarray(record['bbox_resize'][i]).reshape(-1)[:4])
        out.segments(((x1, y1), (x2, y1), (x2, y2), (x1, y2)), BOX_EDGES, rad, c_box)
        kpts = np.asarray(record['kpts_2d_pred'][i], dtype=np.float64).reshape(-1, 2)
        out.segments(kpts[1:9], CUBOID_EDGES, rad, c_cub)
        out.discs(kpts, float(point_radius), c_kpt)
    for gt in record.get('kpts_2d_gt', ()):
        gt = np.asarray(gt, dtype=np.float64)
        gt = gt.reshape(-1, gt.shape[-1] if gt.ndim >= 2 and gt.shape[-1] in (2, 3) else 3)
        out.segments(gt[1:9, :2], CUBOID_EDGES, rad, parse_color('g'))
    return out.arrays()


def _footprint(x, z, l, w, rho):
    """Corners centre + (cos r dx + sin r dz, -sin r dx + cos r dz) for dx = +-l/2, dz = +-w/2 (KITTI's rotation about
    y, csrc/cuboid_math.h), in the order front-left, front-right, rear-right, rear-left, and the middle of the front
    side (dx = +l/2)."""
    c, s = math.cos(rho), math.sin(rho)

    def at(dx, dz):
        return (x + c * dx + s * dz, z - s * dx + c * dz)
    hl, hw = 0.5 * l, 0.5 * w
    return [at(hl, hw), at(hl, -hw), at(-hl, -hw), at(-hl, hw)], at(hl, 0.0)


def build_bev_primitives(record, extent=(-25, 25, 0, 60), px_per_m=10, gt_rows=None, color_dict=None,
                         line_width=2.0):
    """The top view of one record -> ``(prims, colors, (rows, cols), n)``: a canvas of (z1 - z0) s rows by (x1 - x0) s
    columns (to be drawn on white), u = (x - x0) s, v = (z1 - z) s, a light-grey grid line every 10 m, then per box a
    footprint rectangle and a heading tick from the centre to the middle of the front side, in three layers: ground
    truth (``gt_rows``: dicts with locations / dimensions (l, h, w) / rot_y; black), the input box of
    ``raw_txt_format`` with its own ``rot_y`` (magenta, "without Ego-Net") and the same box with the predicted yaw
    ``euler_angles[i][1]`` -- or, for a refined instance (``refine_status == 1``), the fit's own placement and size
    -- in the colour ``bbox_3d`` ("with Ego-Net").  An instance takes part when its row has usable ``locations`` /
    ``dimensions`` (locations[2] > 0) or it is refined; ``n`` counts them."""
    cd = dict(DEFAULT_COLORS if color_dict is None else color_dict)
    c_with = parse_color(cd.get('bbox_3d', cd['bbox_2d']))
    x0, x1, z0, z1 = (float(v) for v in extent)
    s = float(px_per_m)
    rows_px, cols_px = int(round((z1 - z0) * s)), int(round((x1 - x0) * s))
    rad = 0.5 * float(line_width)
    out = _List()
    grey = parse_color(GRID_GREY)
    for gx in np.arange(math.ceil(x0 / 10.0) * 10.0, x1 + 1e-9, 10.0):
        out.segments((((gx - x0) * s, 0.0), ((gx - x0) * s, float(rows_px - 1))), ((0, 1),), 0.5, grey)
    for gz in np.arange(math.ceil(z0 / 10.0) * 10.0, z1 + 1e-9, 10.0):
        out.segments(((0.0, (z1 - gz) * s), (float(cols_px - 1), (z1 - gz) * s)), ((0, 1),), 0.5, grey)

    def box(x, z, l, w, rho, col):
        corners, front = _footprint(x, z, l, w, rho)
        pts = [((px - x0) * s, (z1 - pz) * s) for px, pz in corners + [(x, z), front]]
        out.segments(pts, BOX_EDGES + ((4, 5),), rad, col)

    def usable(r):
        return 'locations' in r and 'dimensions' in r and r['locations'][2] > 0

    for r in gt_rows or ():
        if usable(r):
            box(r['locations'][0], r['locations'][2], r['dimensions'][0], r['dimensions'][2], r['rot_y'],
                parse_color('k'))
    raw = record.get('raw_txt_format')
    n_inst = len(record['kpts_2d_pred'])
    status = record.get('refine_status')
    has_raw = [raw is not None and len(raw) == n_inst and usable(raw[i]) for i in range(n_inst)]
    refined = [status is not None and int(status[i]) == 1 for i in range(n_inst)]
    for i in range(n_inst):
        if has_raw[i]:
            r = raw[i]
            box(r['locations'][0], r['locations'][2], r['dimensions'][0], r['dimensions'][2], r['rot_y'],
                parse_color('m'))
    n = 0
    for i in range(n_inst):
        yaw = float(record['euler_angles'][i][1])
        if refined[i]:
            l, h, w = (float(v) for v in record['refine_dims'][i])
            rt = np.asarray(record['refine_rt'][i], dtype=np.float64)
            loc = rt[9:12] + rt[:9].reshape(3, 3) @ np.array([0., 0.5 * h, 0.])
            box(loc[0], loc[2], l, w, yaw, c_with)
        elif has_raw[i]:
            r = raw[i]
            box(r['locations'][0], r['locations'][2], r['dimensions'][0], r['dimensions'][2], yaw, c_with)
        else:
            continue
        n += 1
    prims, colors = out.arrays()
    return prims, colors, (rows_px, cols_px), n


def _frame_table(shapes, offsets, strides, ranges, n_prims):
    """The int64 [n, 6] table of egn_overlay_draw_u8, checked while it is on the host (the device entry cannot)."""
    tab = np.zeros((len(shapes), 6), dtype=np.int64)
    for i, ((h, w), off, st, (b, e)) in enumerate(zip(shapes, offsets, strides, ranges)):
        if not (0 <= b <= e <= n_prims):
            raise ValueError('frame %d: primitive range (%d, %d) outside [0, %d]' % (i, b, e, n_prims))
        if st < 3 * w:
            raise ValueError('frame %d: row stride %d below 3 W = %d' % (i, st, 3 * w))
        tab[i] = (off, h, w, st, b, e)
    return tab


class OverlayRenderer(object):
    """Draws primitive lists into batches of uint8 [H, W, 3] RGB frames: one launch per ``draw``."""

    def __init__(self, device=None, antialias=True):
        """``device``: 'cpu' = always the host twin; None = the current GPU when one is visible, else the host twin."""
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else 'cpu'
        self.device = torch.device(device)
        self.antialias = bool(antialias)
        self._staging = PinnedStaging(1 << 20)

    @staticmethod
    def _check(frames, prims, colors, ranges):
        prims = np.ascontiguousarray(prims, dtype=np.float32).reshape(-1, 6)
        colors = np.ascontiguousarray(colors, dtype=np.uint32).reshape(-1)
        if len(prims) != len(colors) or len(frames) != len(ranges):
            raise ValueError('draw: %d primitives / %d colours, %d frames / %d ranges'
                             % (len(prims), len(colors), len(frames), len(ranges)))
        for f in frames:
            if tuple(f.shape[2:]) != (3,) or len(f.shape) != 3 or str(f.dtype).split('.')[-1] != 'uint8':
                raise ValueError('draw expects [H,W,3] uint8 frames, got %s %s' % (f.dtype, tuple(f.shape)))
        return prims, colors, [(int(b), int(e)) for b, e in ranges]

    def draw(self, frames, prims, colors, ranges):
        """``frames``: a list of [H,W,3] uint8 frames, all numpy arrays, all CPU tensors or all CUDA tensors of one
        device; ``ranges[i] = (begin, end)``: the primitives of frame i.  Returns the drawn frames, of the same kind.
        CUDA frames are drawn in place on the current stream without synchronisation (table and primitives travel in
        one pinned upload).  Host frames are left as they are and copies come back: drawn by the host twin on a 'cpu'
        renderer, else uploaded with the table in one copy, drawn and read back in one copy."""
        frames = list(frames)
        prims, colors, ranges = self._check(frames, prims, colors, ranges)
        if not frames:
            return []
        on_gpu = [torch.is_tensor(f) and f.is_cuda for f in frames]
        if any(on_gpu):
            if not all(on_gpu) or len({f.device for f in frames}) != 1:
                raise ValueError('draw: CUDA frames must all live on one device')
            self._draw_resident(frames, prims, colors, ranges)
            return frames
        as_tensor = torch.is_tensor(frames[0])
        arrays = [np.ascontiguousarray(f.numpy() if torch.is_tensor(f) else f) for f in frames]
        shapes = [a.shape[:2] for a in arrays]
        sizes = [a.size for a in arrays]
        offsets = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
        packed = np.concatenate([a.reshape(-1) for a in arrays]) if sum(sizes) else np.zeros(0, dtype=np.uint8)
        tab = _frame_table(shapes, offsets, [3 * w for _, w in shapes], ranges, len(prims))
        if self.device.type == 'cpu':
            if packed.size:
                _lib.check(_lib.lib().egn_overlay_draw_host_u8(
                    packed.ctypes.data, tab.ctypes.data, len(tab), prims.ctypes.data, colors.ctypes.data, len(prims),
                    int(self.antialias)), 'overlay_draw_host')
        elif packed.size:
            with torch.cuda.device(self.device):
                views, _ = self._staging.upload({'frames': packed, 'table': tab, 'prims': prims,
                                                 'colors': colors.view(np.int32)}, self.device)
                self._launch(views['frames'], views['table'], len(tab), max(h for h, _ in shapes),
                             max(w for _, w in shapes), views['prims'], views['colors'], len(prims))
                packed = views['frames'].cpu().numpy()      # one copy back; waits for the launch
        out = [packed[o:o + n].reshape(h, w, 3) for o, n, (h, w) in zip(offsets, sizes, shapes)]
        return [torch.from_numpy(a) for a in out] if as_tensor else out

    def _draw_resident(self, frames, prims, colors, ranges):
        dev = frames[0].device
        for f in frames:
            if f.numel() and (f.stride(2) != 1 or f.stride(1) != 3):
                raise ValueError('draw: a CUDA frame must be RGB-interleaved (strides (row, 3, 1)), got %s'
                                 % (f.stride(),))
        live = [f for f in frames if f.numel()]
        if not live:
            return
        base = min(f.data_ptr() for f in live)
        shapes = [tuple(f.shape[:2]) for f in frames]
        tab = _frame_table(shapes, [f.data_ptr() - base if f.numel() else 0 for f in frames],
                           [f.stride(0) if f.numel() else 3 * f.shape[1] for f in frames], ranges, len(prims))
        with torch.cuda.device(dev):
            views, _ = self._staging.upload({'table': tab, 'prims': prims, 'colors': colors.view(np.int32)}, dev)
            self._launch(base, views['table'], len(tab), max(h for h, _ in shapes), max(w for _, w in shapes),
                         views['prims'], views['colors'], len(prims))

    def _launch(self, base, table, n_frames, max_h, max_w, prims, colors, n_prims):
        base = _lib.ptr(base) if torch.is_tensor(base) else base
        _lib.check(_lib.lib().egn_overlay_draw_u8(
            base, _lib.ptr(table), n_frames, int(max_h), int(max_w), _lib.ptr(prims), _lib.ptr(colors), n_prims,
            int(self.antialias), 1, _lib.current_stream(table.device)), 'overlay_draw')
