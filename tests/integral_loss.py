"""The heat-map head's integral terms, restated (TEST INFRASTRUCTURE ONLY; shared by tests/test_integral_loss_cpu.py and
tests/test_gpu_integral_loss.py).

1. ``composite_loss_maps``: libs/loss/function.py:170-202 for a model that returns heat-maps only, in whatever dtype
   the maps have (float64 in the tests), torch autograd: the heat-map term, ``soft_arg_max`` (img_proc.py:678-707)
   divided by hm_size with the reference's index quirk, L_2d over the labelled prefix, L_cr.  Pinned on the
   reference's own class by tests/golden/integral_loss.npz.
2. ``softargmax64`` / ``softargmax_bwd64``: the soft-arg-max and its Jacobian product on the padded NHWC layout of
   csrc/softargmax.hip, float64 numpy, with the sum of absolute terms of every output (the scale of the bound).
3. ``emulate_fp32``: the kernel's summation order (csrc/softargmax_math.h) in numpy float32 -- the slices, the halving
   tree, one rounding per operation -- with a correctly rounded float32 exp.  It is NOT the kernel: it measures how far
   float32 arithmetic in that order lands from float64, in units of 2^-24 x the sum of absolute terms.  C_BOUND is 4 x
   the worst ratio it measures over SWEEP_CASES (``measure_ratio``; the CPU test re-measures and holds the number).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.hrnet_train_oracle import cross_ratio_loss

EPS = 2.0 ** -24
_CRIT = {'mse': F.mse_loss, 'l1': F.l1_loss, 'sl1': F.smooth_l1_loss}

# worst ratio |fp32 emulation - float64| / (2^-24 x sum of absolute terms) over SWEEP_CASES, forward and backward
# (measure_ratio(), re-measured by test_integral_loss_cpu.py::test_bound_constant_is_four_times_the_emulation), and the
# bound's constant: 4 x that, rounded up.  Neither number comes from the device or from the host twins.
MEASURED_RATIO = {'fwd': 10.72, 'bwd': 46.58}
C_BOUND = {'fwd': 43.0, 'bwd': 187.0}

# (N, K, h, w, cs, logit scale): the GPU test's shapes plus the edge shapes of the CPU test
SWEEP_CASES = [(1, 1, 2, 2, 4, 3.0), (2, 5, 16, 16, 8, 3.0), (3, 33, 12, 16, 36, 3.0), (2, 33, 64, 64, 36, 3.0),
               (1, 1, 1, 1, 4, 1.0), (2, 5, 16, 16, 8, 30.0), (2, 3, 5, 7, 4, 1.0)]


def soft_arg_max_norm(maps, hm_size):
    """soft_arg_max(maps) with x / hm_size[1], y / hm_size[0] (function.py:191-193): maps [N,K,H,W] -> [N,K,2]."""
    n, k, h, w = maps.shape
    p = F.softmax(maps.reshape(n, k, -1), dim=2).reshape(n, k, h, w)
    xs = torch.arange(w, dtype=maps.dtype)
    ys = torch.arange(h, dtype=maps.dtype)
    x = (p.sum(dim=2) * xs).sum(dim=2) / hm_size[1]
    y = (p.sum(dim=3) * ys).sum(dim=2) / hm_size[0]
    return torch.stack([x, y], dim=2)


def composite_loss_maps(maps, target, joints_xy, img_size, hm_size, spec=('mse', 'l1', 'None'), weights=(1.0, 0.1, 'None'),
                        apply_cr_loss=False, cr_indices=None, target_cr=4.0 / 3.0, cr_loss_thres=0.15):
    """JointsCompositeLoss.forward(output = maps) (function.py:170-202).  maps [N,K,H,W]; target [n_fs,K,H,W];
    joints_xy [n_fs,K,2] in input pixels; img_size = (width, height); hm_size = [w, h] as the reference's configs hold
    it.  Returns (loss, coords [N', K, 2]) -- N' = n_fs when the heat-map term is on and cut the maps (:184-185)."""
    total = 0
    pred = maps
    if spec[0] != 'None':
        if len(pred) != len(target):
            pred = pred[:len(target)]                     # rebinds heatmaps_pred: everything below sees the prefix
        n, k = pred.shape[:2]
        a, b = pred.reshape(n, k, -1), target.reshape(n, k, -1).to(pred.dtype)
        hm = 0
        for j in range(k):
            hm = hm + 0.5 * _CRIT[spec[0]](a[:, j], b[:, j], reduction='mean')
        total = total + (hm / k) * weights[0]
    coords = None
    if spec[1] != 'None':
        gt = joints_xy[..., :2].clone().to(pred.dtype)
        gt[..., 0] /= img_size[0]
        gt[..., 1] /= img_size[1]
        coords = soft_arg_max_norm(pred, hm_size)
        total = total + _CRIT[spec[1]](coords[:len(gt)], gt, reduction='mean') * weights[1]
    if spec[2] != 'None' and weights[2] != 'None' and apply_cr_loss:
        # (like the reference, L_cr needs the coordinate term to have produced coordinates_pred)
        total = total + cross_ratio_loss(coords, cr_indices, target_cr, cr_loss_thres, spec[2]) * weights[2]
    return total, coords


def to_nhwc(maps, cs, fill=0.0):
    """[N,K,H,W] -> padded NHWC [N,H,W,cs] float32 numpy, pad channels = fill."""
    m = np.asarray(maps, dtype=np.float32)
    n, k, h, w = m.shape
    out = np.full((n, h, w, cs), fill, np.float32)
    out[..., :k] = m.transpose(0, 2, 3, 1)
    return out


def softargmax64(z, K, div_x, div_y):
    """z [N,h,w,cs] -> coords [N,K,2] float64, abs-term sums [N,K,2], and (s [N,h,w,K], ex, ey [N,K])."""
    z = np.asarray(z, np.float64)[..., :K]
    n, h, w, _ = z.shape
    e = np.exp(z - z.max(axis=(1, 2), keepdims=True))
    s = e / e.sum(axis=(1, 2), keepdims=True)
    xs = np.arange(w, dtype=np.float64)[None, None, :, None]
    ys = np.arange(h, dtype=np.float64)[None, :, None, None]
    ex, ey = (s * xs).sum(axis=(1, 2)), (s * ys).sum(axis=(1, 2))
    coords = np.stack([ex / div_x, ey / div_y], axis=2)
    return coords, np.abs(coords), (s, ex, ey)            # every term s_p x_p is >= 0: the sum of |terms| is the value


def softargmax_bwd64(z, K, div_x, div_y, dcoords):
    """d maps [N,h,w,K] float64 for dcoords [N,K,2], and the sum of absolute terms of each element:
    s_p ((x_p + ex) |gx| / div_x + (y_p + ey) |gy| / div_y) -- x_p and ex enter as separate terms."""
    _, _, (s, ex, ey) = softargmax64(z, K, div_x, div_y)
    n, h, w, _ = s.shape
    g = np.asarray(dcoords, np.float64)
    ax, ay = g[:, None, None, :, 0] / div_x, g[:, None, None, :, 1] / div_y
    xs = np.arange(w, dtype=np.float64)[None, None, :, None]
    ys = np.arange(h, dtype=np.float64)[None, :, None, None]
    exb, eyb = ex[:, None, None, :], ey[:, None, None, :]
    dz = s * ((xs - exb) * ax + (ys - eyb) * ay)
    mag = s * ((xs + exb) * np.abs(ax) + (ys + eyb) * np.abs(ay))
    return dz, mag


# ---------------------------------------------------------------------------------------------------------------
# the kernel's order in numpy float32
# ---------------------------------------------------------------------------------------------------------------
def slices(cs):
    return min(64, 1024 // min(cs, 1024))                 # egn_sam_slices


def _tree(part, S, fold):
    """part: list of S arrays; the halving tree of egn_sam_tree_top."""
    p = 1
    while p < S:
        p <<= 1
    off = p >> 1
    while off >= 1:
        for j in range(off):
            if j + off < S:
                part[j] = fold(part[j], part[j + off])
        off >>= 1
    return part[0]


def emulate_fp32(z, K, div_x, div_y, dcoords=None):
    """(coords [N,K,2], dz [N,h,w,K] or None) in float32, summed in the kernel's order."""
    f = np.float32
    z = np.asarray(z, f)
    n, h, w, cs = z.shape
    S, hw = slices(cs), h * w
    zf = z.reshape(n, hw, cs)[..., :K]
    m = zf.max(axis=1)                                    # exact in any order
    e = np.exp((zf - m[:, None, :]).astype(f).astype(np.float64)).astype(f)      # float32 exp, correctly rounded
    px = (np.arange(hw) % w).astype(f)[None, :, None]
    py = (np.arange(hw) // w).astype(f)[None, :, None]
    tx = (e.astype(np.float64) * px)                      # fmaf: the product is exact, one rounding after the add
    ty = (e.astype(np.float64) * py)
    parts = {k: [] for k in ('se', 'sx', 'sy')}
    for j in range(S):
        se, sx, sy = np.zeros((n, K), f), np.zeros((n, K), f), np.zeros((n, K), f)
        for p in range(j, hw, S):
            se = (se + e[:, p]).astype(f)
            sx = (sx.astype(np.float64) + tx[:, p]).astype(f)
            sy = (sy.astype(np.float64) + ty[:, p]).astype(f)
        parts['se'].append(se)
        parts['sx'].append(sx)
        parts['sy'].append(sy)
    tot = {k: _tree(v, S, lambda a, b: (a + b).astype(f)) for k, v in parts.items()}
    ex, ey = (tot['sx'] / tot['se']).astype(f), (tot['sy'] / tot['se']).astype(f)
    coords = np.stack([(ex / f(div_x)).astype(f), (ey / f(div_y)).astype(f)], axis=2)
    if dcoords is None:
        return coords, None
    g = np.asarray(dcoords, f)
    inv = (f(1) / tot['se']).astype(f)
    ax, ay = (g[..., 0] / f(div_x)).astype(f), (g[..., 1] / f(div_y)).astype(f)
    s = (e * inv[:, None, :]).astype(f)
    dx = ((px - ex[:, None, :]).astype(f) * ax[:, None, :]).astype(f)
    dy = (py - ey[:, None, :]).astype(f)
    t = (dy.astype(np.float64) * ay[:, None, :].astype(np.float64) + dx).astype(f)
    return coords, (s * t).astype(f).reshape(n, h, w, K)


def sweep_inputs(case, seed=0):
    n, K, h, w, cs, scale = case
    rng = np.random.RandomState(1000 * seed + n * 131 + K * 17 + h * 5 + w + cs)
    z = np.full((n, h, w, cs), np.nan, np.float32)        # pad channels: NaN, the kernel must not look
    z[..., :K] = (rng.randn(n, h, w, K) * scale).astype(np.float32)
    g = rng.randn(n, K, 2).astype(np.float32)
    return z, g


UNDERFLOW = 2.0 ** -120     # float32's range, not its precision: e_p below e^-87 ~ 2^-125.5 is dropped by definition
                            # (softargmax_math.h) and a product below 2^-126 loses bits; x the geometric factor below


def underflow_floor(z, K, div_x, div_y, g):
    """What float32's RANGE may cost each output, whatever the order: UNDERFLOW x the largest factor a softmax weight
    is multiplied by -- (w - 1) / div_x, (h - 1) / div_y forward; 2 ((w - 1) |gx| / div_x + (h - 1) |gy| / div_y)
    backward."""
    n, h, w, _ = np.asarray(z).shape
    g = np.abs(np.asarray(g, np.float64))
    fc = UNDERFLOW * np.broadcast_to(np.array([(w - 1) / div_x, (h - 1) / div_y]), (n, K, 2))
    fd = UNDERFLOW * 2 * ((w - 1) * g[..., 0] / div_x + (h - 1) * g[..., 1] / div_y)
    return fc, np.broadcast_to(fd[:, None, None, :], (n, h, w, K))


def ratios(got_coords, got_dz, z, K, div_x, div_y, g):
    """Worst (|got - float64| - underflow floor) / (2^-24 x sum of absolute terms), forward and backward."""
    want_c, mag_c, _ = softargmax64(z, K, div_x, div_y)
    want_d, mag_d = softargmax_bwd64(z, K, div_x, div_y, g)
    floor_c, floor_d = underflow_floor(z, K, div_x, div_y, g)

    def worst(got, want, mag, floor):
        err = np.maximum(np.abs(np.asarray(got, np.float64) - want) - floor, 0.0)
        assert not (err[mag == 0] > 0).any(), 'an output with no non-zero term is not exactly zero'
        return float((err[mag > 0] / (EPS * mag[mag > 0])).max()) if (mag > 0).any() else 0.0
    return worst(got_coords, want_c, mag_c, floor_c), worst(got_dz, want_d, mag_d, floor_d)


def measure_ratio():
    """The emulation's worst ratios over SWEEP_CASES (div_x, div_y as the step passes them: h, w)."""
    rf = rb = 0.0
    for case in SWEEP_CASES:
        z, g = sweep_inputs(case)
        n, K, h, w, cs, _ = case
        c, d = emulate_fp32(z, K, float(h), float(w), g)
        a, b = ratios(c, d, z, K, float(h), float(w), g)
        rf, rb = max(rf, a), max(rb, b)
    return {'fwd': rf, 'bwd': rb}
