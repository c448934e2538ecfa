"""The debug pictures' definition restated in numpy float64, independent of
csrc/debug_pictures_math.h, and the seeded cases the CPU and GPU tests share.

    range      lo / hi = min / max over the first three planes of all crops, NaNs ignored; 0 0 when all are NaNs
    crop       q = trunc(min(255, max(0, 255 (x - lo) / (hi - lo + 1e-5)))), 0 for a NaN
    grid       make_grid's layout, padding and empty cells 0
    thumbnail  bilinear on the uint8 levels, half-pixel centres, indices clamped, floor(v + 0.5)
    tile       (7 lut[trunc(min(255, max(0, 255 m)))] + 3 thumbnail) // 10
"""
import math

import numpy as np


def image_range(x, c_used=3):
    v = np.asarray(x, dtype=np.float32)[:, :c_used]
    if v.size == 0 or np.isnan(v).all():
        return np.zeros(2, dtype=np.float32)
    return np.array([np.nanmin(v), np.nanmax(v)], dtype=np.float32) + np.float32(0.0)


def level(s):
    """trunc(min(255, max(0, s))) with NaN -> 0, on a float64 array."""
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        ok = s >= 0
        return np.where(ok, np.minimum(np.where(ok, s, 0.0), 255.0), 0.0).astype(np.uint8)


def quant_crop(x, lohi):
    lo, hi = float(lohi[0]), float(lohi[1])
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        v = (np.asarray(x, dtype=np.float32).astype(np.float64) - lo) / (hi - lo + 1e-5)
        return level(255.0 * v)


def quant_map(m):
    with np.errstate(invalid='ignore', over='ignore'):
        return level(255.0 * np.asarray(m, dtype=np.float32).astype(np.float64))


def grid(x, lohi, nrow=8, pad=2):
    x = np.asarray(x, dtype=np.float32)
    N, _, H, W = x.shape
    xmaps = min(nrow, N)
    ymaps = int(math.ceil(N / xmaps))
    out = np.zeros((ymaps * (H + pad) + pad, xmaps * (W + pad) + pad, 3), dtype=np.uint8)
    for k in range(N):
        r, c = (k // xmaps) * (H + pad) + pad, (k % xmaps) * (W + pad) + pad
        out[r:r + H, c:c + W] = quant_crop(x[k, :3], lohi).transpose(1, 2, 0)
    return out


def _taps(src, dst):
    d = np.arange(dst, dtype=np.float64)
    x = (d + 0.5) * (float(src) / float(dst)) - 0.5
    x0 = np.floor(x)
    i = x0.astype(np.int64)
    return np.clip(i, 0, src - 1), np.clip(i + 1, 0, src - 1), x - x0


def thumbnail(levels, h, w):
    """uint8 [H, W, 3] -> uint8 [h, w, 3]."""
    H, W = levels.shape[:2]
    y0, y1, fy = _taps(H, h)
    x0, x1, fx = _taps(W, w)
    q = levels.astype(np.float64)
    fx_, fy_ = fx[None, :, None], fy[:, None, None]
    a, b = q[y0][:, x0], q[y0][:, x1]
    c, d = q[y1][:, x0], q[y1][:, x1]
    top = a * (1.0 - fx_) + b * fx_
    bot = c * (1.0 - fx_) + d * fx_
    v = top * (1.0 - fy_) + bot * fy_
    return np.floor(v + 0.5).astype(np.uint8)


def mosaic(x, maps, lohi, lut):
    x, maps = np.asarray(x, dtype=np.float32), np.asarray(maps, dtype=np.float32)
    n, J, h, w = maps.shape
    out = np.zeros((n * h, (J + 1) * w, 3), dtype=np.uint8)
    for i in range(n):
        th = thumbnail(quant_crop(x[i, :3], lohi).transpose(1, 2, 0), h, w)
        out[i * h:(i + 1) * h, :w] = th
        for j in range(J):
            col = lut[quant_map(maps[i, j])].astype(np.uint32)
            out[i * h:(i + 1) * h, (j + 1) * w:(j + 2) * w] = ((7 * col + 3 * th.astype(np.uint32)) // 10).astype(np.uint8)
    return out


def jet_lut():
    lut = np.zeros((256, 3), dtype=np.uint8)
    for q in range(256):
        t = q / 255.0
        for ch, k in enumerate((3, 2, 1)):
            c = min(1.0, max(0.0, 1.5 - abs(4 * t - k)))
            lut[q, ch] = int(math.floor(255 * c + 0.5))
    return lut


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, 3.4e38, -3.4e38, 1e-30], dtype=np.float32)


def build_case(N, C, H, W, n, J, h, w, seed, kind='normal'):
    """-> (crops [N,C,H,W] float32, maps [n,J,h,w] float32).  kinds: 'normal' (crops ~ N(0, 1), maps in [-0.2, 1.2]:
    values outside [0, 1] on both sides), 'constant' (every crop value 0.25: hi == lo), 'special' (NaN, +-inf, -0 and
    huge values sprinkled into crops and maps), 'special_finite' (NaN and huge finite values, no infinity, so the range
    stays finite and the levels spread)."""
    rs = np.random.RandomState(seed)
    x = rs.randn(N, C, H, W).astype(np.float32)
    m = rs.uniform(-0.2, 1.2, (n, J, h, w)).astype(np.float32)
    if kind == 'constant':
        x[:] = 0.25
    elif kind in ('special', 'special_finite'):
        pool = SPECIALS if kind == 'special' else np.array([np.nan, -0.0, 7.5, -6.0, 1e-30], dtype=np.float32)
        for a in (x, m):
            flat = a.reshape(-1)
            where = rs.choice(flat.size, max(1, flat.size // 7), replace=False)
            flat[where] = pool[rs.randint(0, len(pool), len(where))]
        mpool = SPECIALS
        flat = m.reshape(-1)
        where = rs.choice(flat.size, max(1, flat.size // 9), replace=False)
        flat[where] = mpool[rs.randint(0, len(mpool), len(where))]
    return x, m


# (name, N, C, H, W, nrow, n, J, h, w, kind): the smallest shapes at which the composers take another path -- a ragged
# last grid row with an empty cell (N = 3, nrow = 2), a channel stride (C = 5), thumbnail ratios 4 / 2 / 1, a map width
# that is no multiple of 4 (scalar loads, byte stores), one and several joints, more joints than joint shares (J = 11),
# a labelled prefix (n < N), a strip shorter than the map (h = 70 rows of 8), a map wider than a block's LDS strip
# (w = 1030), an up-sampled thumbnail (taps clamped at both ends)
CASES = [
    ('ratio4_tail', 3, 5, 16, 24, 2, 3, 5, 4, 6, 'normal'),
    ('ratio2', 3, 5, 16, 24, 2, 3, 5, 8, 12, 'normal'),
    ('ratio1', 3, 5, 16, 24, 2, 2, 1, 16, 24, 'normal'),
    ('prefix_j1', 3, 3, 16, 24, 8, 2, 1, 4, 6, 'normal'),
    ('j11', 2, 3, 16, 24, 8, 2, 11, 4, 6, 'normal'),
    ('constant', 3, 5, 16, 24, 2, 3, 5, 4, 6, 'constant'),
    ('special', 3, 5, 16, 24, 2, 3, 5, 4, 6, 'special'),
    ('special_finite', 3, 5, 16, 24, 2, 3, 5, 8, 12, 'special_finite'),
    ('strips', 1, 3, 35, 8, 8, 1, 2, 70, 8, 'normal'),
    ('wide_map', 1, 3, 2, 5, 8, 1, 1, 1, 1030, 'normal'),
    ('one_pixel', 1, 3, 1, 1, 1, 1, 1, 1, 1, 'normal'),
]
