"""The overlay rasteriser's definition restated in numpy float64, independent of csrc/overlay_math.h, and the cases
that the CPU and GPU tests share.

A primitive is (x0 y0 x1 y1 r a) plus a colour word R | G << 8 | B << 16; a pixel has its centre at integer
coordinates; primitives are applied in list order and the frame is rounded to uint8 after each.
"""
import numpy as np


def draw(frame, prims, colors, antialias=True):
    """frame uint8 [H,W,3] -> (drawn copy, reach [H,W] bool): ``reach`` marks the pixels within r + 0.5 of some valid
    primitive's segment -- outside it nothing may change."""
    img = np.array(frame, dtype=np.uint8, copy=True)
    H, W = img.shape[:2]
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    reach = np.zeros((H, W), dtype=bool)
    for p, col in zip(np.asarray(prims, dtype=np.float32).reshape(-1, 6), np.asarray(colors).reshape(-1)):
        if not np.all(np.isfinite(p)) or p[4] < 0:
            continue
        x0, y0, x1, y1, r, a = (float(v) for v in p)
        a = min(1.0, max(0.0, a))
        dx, dy = x1 - x0, y1 - y0
        px, py = x - x0, y - y0
        len2 = dx * dx + dy * dy
        t = (px * dx + py * dy) / len2 if len2 > 0 else np.zeros_like(px)
        t = np.minimum(1.0, np.maximum(0.0, t))
        ex, ey = px - t * dx, py - t * dy
        d = np.sqrt(ex * ex + ey * ey)
        c = np.minimum(1.0, np.maximum(0.0, r + 0.5 - d)) if antialias else (d <= r).astype(np.float64)
        reach |= d <= r + 0.5
        w = c * a
        hit = w > 0
        rgb = np.array([int(col) & 255, (int(col) >> 8) & 255, (int(col) >> 16) & 255], dtype=np.float64)
        v = img.astype(np.float64)
        v = np.floor(v + (rgb[None, None, :] - v) * w[:, :, None] + 0.5)
        img[hit] = v[hit].astype(np.uint8)
    return img, reach


def rgb(r, g, b):
    return r | g << 8 | b << 16


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def varied_prims(h, w, seed=0):
    """Horizontal, vertical, diagonal, zero-length, fully outside, half outside with negative coordinates, end points
    at +-1e9, radius 100 (every tile), fractional opacities, and a few random ones."""
    rs = np.random.RandomState(seed)
    p = [
        (2.0, 5.0, w - 3.0, 5.0, 1.0, 1.0),                  # horizontal
        (7.0, 1.0, 7.0, h - 2.0, 0.5, 0.7),                  # vertical
        (1.0, 1.0, w - 2.0, h - 2.0, 1.5, 0.5),              # diagonal
        (w / 2.0, h / 2.0, w / 2.0, h / 2.0, 3.0, 1.0),      # zero length: a disc
        (w / 3.0 + 0.25, h / 3.0 + 0.4, w / 3.0 + 0.25, h / 3.0 + 0.4, 0.0, 1.0),   # radius 0, off-centre
        (-500.0, -40.0, -300.0, -20.0, 2.0, 1.0),            # fully outside
        (-10.5, -7.25, w / 2.0, h / 2.0, 1.0, 0.9),          # half outside, negative coordinates
        (-1e9, -1e9, 1e9, 1e9, 1.0, 0.6),                    # end points at +-1e9, through the frame
        (-1e9, h / 2.0, 1e9, h / 2.0 + 3.0, 0.75, 1.0),
        (1e9, 1e9, 1e9 + 5.0, 1e9, 4.0, 1.0),                # far away altogether
        (w / 2.0, h / 2.0, w / 2.0 + 1.0, h / 2.0, 100.0, 0.25),   # radius 100: covers every tile
        (3.0, 3.0, 9.0, 4.0, 1.0, 2.5),                      # opacity above 1: clamped
        (3.0, 8.0, 9.0, 9.0, 1.0, -0.5),                     # below 0: clamped, draws nothing
    ]
    for _ in range(12):
        x0, x1 = rs.uniform(-5, w + 5, 2)
        y0, y1 = rs.uniform(-5, h + 5, 2)
        p.append((x0, y0, x1, y1, rs.uniform(0, 3), rs.uniform(0, 1)))
    prims = np.asarray(p, dtype=np.float32)
    colors = rs.randint(0, 1 << 24, len(prims)).astype(np.uint32)
    return prims, colors


def dropped_prims():
    """Primitives that must leave no trace: a NaN, an infinity, a negative radius."""
    p = np.asarray([(np.nan, 2.0, 9.0, 9.0, 2.0, 1.0), (2.0, 2.0, np.inf, 9.0, 2.0, 1.0),
                    (2.0, 2.0, 9.0, 9.0, -1.0, 1.0), (2.0, 2.0, 9.0, 9.0, 2.0, np.nan),
                    (2.0, 2.0, 9.0, -np.inf, 2.0, 1.0)], dtype=np.float32)
    return p, np.full(len(p), rgb(255, 255, 255), dtype=np.uint32)


# (name, frame sizes (h, w), seed, row strides or None = tight, frames with an empty primitive range): every other
# frame gets varied_prims of its own.  45 * 3 = 135 is no multiple of 4; 144 leaves padding bytes that must survive.
CASES = [('one_pixel', [(1, 1)], 1, None, ()),
         ('stride_135', [(33, 45)], 2, [135], ()),
         ('stride_144', [(33, 45)], 2, [144], ()),
         ('three_frames', [(33, 45), (8, 70), (40, 17)], 3, None, (1,)),
         ('tile_edges', [(65, 67)], 4, [205], ())]


def table(shapes, strides, counts):
    """The int64 [n,6] frame table for frames packed back to back: (offset, H, W, stride, begin, end)."""
    tab, off, b = [], 0, 0
    for (h, w), st, n in zip(shapes, strides, counts):
        tab.append((off, h, w, st, b, b + n))
        off += h * st
        b += n
    return np.asarray(tab, dtype=np.int64).reshape(-1, 6), off


def pack(frames, strides):
    """Frames -> one uint8 buffer with the given row strides (padding bytes = 0xA5) and their table offsets."""
    parts = []
    for f, st in zip(frames, strides):
        h, w = f.shape[:2]
        rows = np.full((h, st), 0xA5, dtype=np.uint8)
        rows[:, :3 * w] = f.reshape(h, 3 * w)
        parts.append(rows.reshape(-1))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def unpack(buf, tab):
    """-> ([H,W,3] frames, the padding bytes of all rows)."""
    frames, pad = [], []
    for off, h, w, st, _, _ in tab:
        rows = buf[off:off + h * st].reshape(h, st)
        frames.append(rows[:, :3 * w].reshape(h, w, 3).copy())
        pad.append(rows[:, 3 * w:].reshape(-1))
    return frames, np.concatenate(pad) if pad else np.zeros(0, dtype=np.uint8)


def host_twin(buf, tab, prims, colors, antialias=1):
    """egn_overlay_draw_host_u8 on a copy of ``buf`` -> (return code, drawn buffer)."""
    from egonet_amd import _lib
    out = np.array(buf, dtype=np.uint8, copy=True)
    tab = np.ascontiguousarray(tab, dtype=np.int64)
    prims = np.ascontiguousarray(prims, dtype=np.float32)
    colors = np.ascontiguousarray(colors, dtype=np.uint32)
    code = _lib.lib().egn_overlay_draw_host_u8(out.ctypes.data, tab.ctypes.data, len(tab), prims.ctypes.data,
                                               colors.ctypes.data, len(colors), int(antialias))
    return code, out


def build_case(sizes, seed, strides=None, empty=()):
    """-> (frames, packed buffer, table, prims, colors); frames listed in ``empty`` get an empty primitive range."""
    frames = [noise(h, w, seed + 10 * i) for i, (h, w) in enumerate(sizes)]
    lists = [varied_prims(h, w, seed + i) for i, (h, w) in enumerate(sizes)]
    lists = [(p[:0], c[:0]) if i in empty else (p, c) for i, (p, c) in enumerate(lists)]
    strides = [3 * w for _, w in sizes] if strides is None else strides
    tab, _ = table(sizes, strides, [len(p) for p, _ in lists])
    prims = np.concatenate([p for p, _ in lists])
    colors = np.concatenate([c for _, c in lists])
    return frames, pack(frames, strides), tab, prims, colors
