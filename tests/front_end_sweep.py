"""Cases, references and bounds of the front-end sweep: csrc/crop.hip, csrc/targets.hip, csrc/geometry.hip (pose_math.h)
at the shapes and values where they can go wrong (helper module of tests/test_front_end_sweep_cpu.py and
tests/test_gpu_front_end_sweep.py; imported, not a conftest; needs no GPU).

References
  crops     oracle/crop_oracle.warp_affine_u8, then the float32 (/255 - mean) / std; compared as uint32.
  targets   `targets_ref64`: generate_target (oracle/targets_oracle.py) restated per pixel in float64, with the
            exponent's argument beside the value; held against tests/golden/targets.npz on the CPU.
  geometry  oracle/geometry_oracle.crop_to_screen / six_dof / observation_angle_*, y * std + mean in float64.

Which gap is closed by which test (G = tests/test_gpu_front_end_sweep.py, C = tests/test_front_end_sweep_cpu.py):

  crop.hip   grid-stride wrap of the one-frame entry        G test_crop_wrap_one_frame_entry_and_multi_frame
             one-frame entry, padded rows, odd base         G test_crop_one_frame_padded_rows_odd_base
             out_w < 4, out_h in {1, 15, 17, 33}             G test_crop_multi_frame_output_sizes[WxH]
             vec = 0 for the pointer's alignment            G test_crop_multi_frame_unaligned_out_takes_scalar_stores
             box_frame outside the table reads nothing      G test_crop_box_frame_outside_the_table_reads_nothing
             rotated / sheared / flipped / singular M,      G test_crop_matrix_set_both_entries[imagenet|other]
             box outside, 1x1 frame, x40, /40, mean/std     C test_crop_oracle_vs_scipy_on_rotated_and_sheared,
                                                              test_crop_singular_matrices_give_the_zero_map,
                                                              test_crop_range_condition_holds_for_every_matrix
             no write outside `out`                         every G crop test (guard bands, NaN slack floats)
  targets    beyond the fixtures; truncation points;        G test_targets_edge_cases[sigma1|sigma2|sigma3|sigma1.5|
             the weight rule at the four borders; vis         strides12x20|vis_null|weight_null]
             0 / 0.5 / 0.5+ulp / 1 / NULL; sigma 1.5;       C test_target_cases_hold_every_edge_the_issue_names,
             unequal strides, H != W; weight == NULL          test_target_reference_reproduces_the_fixture,
             the wrap past 8192 x 256                       G test_targets_edge_cases[wrap]
             the bound                                      C test_target_bound_emulation_and_half_precision_mutants
  geometry   egn_unnormalize_f64                            G test_unnormalize[...], test_unnormalize_empty_and_refusals
             keypoints_to_screen: n*K, 192x256, mul,        G test_keypoints_to_screen[...]
             lifter_in NULL, ld_in = 2K + 3, host twin
             pose solve: reflection, gimbal lock, alpha     G test_pose_solve_families[...], test_pose_alpha_next_to_pi,
             wraps, rank-deficient input, host twin           test_pose_rank_deficient_instance_is_alone
                                                            C test_host_pose_families_vs_oracle (g++ build of pose_math.h)
  egonet.py  rotated records through is_cuda=True           G test_get_keypoints_with_rotated_records_on_the_device
"""
import math

import numpy as np

from oracle import crop_oracle, geometry_oracle

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
OTHER_NORM = ((0.1, 0.5, 0.9), (0.3, 1.7, 0.05))           # a mean / std triple that is not ImageNet's

# ---------------------------------------------------------------------------------------------------------------
# 1. crops
# ---------------------------------------------------------------------------------------------------------------
FRAME_HW = (96, 160)
PIXEL_1X1 = (200, 17, 99)                                   # the 1 x 1 frame


def frame(hw=FRAME_HW, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (hw[0], hw[1], 3)).astype(np.uint8)


def affine_about(cx, cy, k, deg, out_wh, shear=(0.0, 0.0), flip=False):
    """Forward 2x3 matrix image -> crop: the point (cx, cy) goes to the crop's centre, scaled by k, rotated by deg,
    sheared by (x from y, y from x) and, with flip, mirrored in x."""
    t = math.radians(deg)
    A = k * np.array([[math.cos(t), math.sin(t)], [-math.sin(t), math.cos(t)]]) @ np.array([[1.0, shear[0]], [shear[1], 1.0]])
    if flip:
        A = A @ np.diag([-1.0, 1.0])
    b = np.array([out_wh[0] * 0.5, out_wh[1] * 0.5]) - A @ np.array([cx, cy])
    return np.hstack([A, b.reshape(2, 1)])


def matrix_set(out_wh, hw=FRAME_HW):
    """[(name, frame index, M)]: frame 0 is `frame()`, frame 1 the 1 x 1 frame."""
    H, W = hw
    cx, cy, k = 0.55 * W, 0.45 * H, out_wh[0] / (0.5 * W)
    c = [('scale+translation', 0, affine_about(cx, cy, k, 0.0, out_wh))]
    for deg in (30.0, 90.0, 180.0, -7.25):
        c.append(('rot%g' % deg, 0, affine_about(cx, cy, k, deg, out_wh)))
    c.append(('shear', 0, affine_about(cx, cy, k, 0.0, out_wh, shear=(0.3, -0.15))))
    c.append(('flip', 0, affine_about(cx, cy, k, 0.0, out_wh, flip=True)))
    c.append(('flip+rot', 0, affine_about(cx, cy, k, 30.0, out_wh, flip=True)))
    c.append(('zeros', 0, np.zeros((2, 3))))
    c.append(('rank1', 0, np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 5.0]])))
    c.append(('outside', 0, affine_about(W + 3.0 * out_wh[0], -2.0 * H, 1.0, 0.0, out_wh)))
    c.append(('x40', 0, affine_about(cx + 0.37, cy - 0.21, 40.0, 0.0, out_wh)))
    c.append(('x40rot', 0, affine_about(1.3, H - 1.4, 41.0, -7.25, out_wh)))
    c.append(('/40', 0, affine_about(0.5 * W, 0.5 * H, 1.0 / 40.0, 0.0, out_wh)))
    c.append(('/40rot', 0, affine_about(0.5 * W, 0.5 * H, 1.0 / 39.0, 30.0, out_wh)))
    c.append(('1x1 frame x8', 1, affine_about(0.0, 0.0, 8.0, 0.0, out_wh)))
    c.append(('1x1 frame rot', 1, affine_about(0.2, -0.3, 5.0, 30.0, out_wh)))
    return c


def inverse_terms(M):
    """(i0 .. i5) of the dst -> src map as both sides compute it: D == 0 gives the zero map."""
    m = np.asarray(M, dtype=np.float64).reshape(2, 3)
    D = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    i0, i1, i3, i4 = m[1, 1] * D, -m[0, 1] * D, -m[1, 0] * D, m[0, 0] * D
    return i0, i1, -i0 * m[0, 2] - i1 * m[1, 2], i3, i4, -i3 * m[0, 2] - i4 * m[1, 2]


def fixed_point_range(M, out_wh):
    """Largest |(a*y + b)*1024| and |a*x*1024| over the crop: below 2^30 the kernel's int32 and the oracle's int64 agree."""
    i0, i1, i2, i3, i4, i5 = inverse_terms(M)
    xs, ys = np.arange(out_wh[0], dtype=np.float64), np.arange(out_wh[1], dtype=np.float64)
    return max(np.abs((i1 * ys + i2) * 1024.0).max(), np.abs((i4 * ys + i5) * 1024.0).max(),
               np.abs(i0 * xs * 1024.0).max(), np.abs(i3 * xs * 1024.0).max())


def assert_range(Ms, out_wh):
    for M in Ms:
        r = fixed_point_range(M, out_wh)
        assert r < 2.0 ** 30, 'fixed-point term %.3g of %s is outside the swept range' % (r, np.asarray(M).ravel())


def normalise(patch, mean, std):
    """[h,w,3] uint8 -> [3,h,w] float32, ToTensor + Normalize in float32."""
    mean = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    std = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    return (patch.transpose(2, 0, 1).astype(np.float32) / np.float32(255) - mean) / std


def ref_crops(frames, box_frame, Ms, out_wh, norm=IMAGENET):
    """[n,3,h,w] float32.  A box whose frame index is outside the table reads nothing: level 0 everywhere."""
    out = []
    for f, M in zip(box_frame, Ms):
        if 0 <= f < len(frames):
            patch = crop_oracle.warp_affine_u8(frames[f], np.asarray(M).reshape(2, 3), out_wh)
        else:
            patch = np.zeros((out_wh[1], out_wh[0], 3), dtype=np.uint8)
        out.append(normalise(patch, *norm))
    return np.stack(out)


def pack_frames(frames, lead=7, pad=lambda i: 5 * (i % 2)):
    """Frames packed into one blob with `lead` bytes in front of each (odd base offsets) and rows of 3 W + pad(i) bytes;
    the gaps hold 0xA5 so that a read of them shows.  -> (blob uint8, table int64 [n][offset, H, W, pitch])"""
    blob, tab, off = [], [], 0
    for i, img in enumerate(frames):
        H, W = img.shape[:2]
        pitch = 3 * W + pad(i)
        rows = np.full((H, pitch), 0xA5, dtype=np.uint8)
        rows[:, :3 * W] = img.reshape(H, 3 * W)
        blob.append(np.full(lead, 0xA5, np.uint8))
        off += lead
        tab.append([off, H, W, pitch])
        blob.append(rows.reshape(-1))
        off += rows.size
    return np.concatenate(blob), np.array(tab, dtype=np.int64)


WRAP_N, WRAP_WH = 2100, (32, 32)            # 2100 * 32 * 32 = 2 150 400 > 8192 * 256 = 2 097 152


def wrap_matrices(n=WRAP_N, out_wh=WRAP_WH, hw=FRAME_HW, seed=5):
    """Many small boxes of one frame: every fourth rotated, some partly outside."""
    rng = np.random.RandomState(seed)
    H, W = hw
    Ms = []
    for i in range(n):
        cx, cy = rng.uniform(-0.1 * W, 1.1 * W), rng.uniform(-0.1 * H, 1.1 * H)
        k = out_wh[0] / rng.uniform(6.0, 0.8 * W)
        Ms.append(affine_about(cx, cy, k, rng.uniform(-180, 180) if i % 4 == 3 else 0.0, out_wh))
    return np.stack(Ms)


# the multi-frame kernel's output sizes: every out_w of {1, 2, 3, 5, 8} and every out_h of {1, 15, 16, 17, 33} at least
# once, and the pair (8, 17)
OUT_SIZES = [(1, 1), (2, 15), (3, 16), (5, 17), (8, 33), (8, 17), (1, 33), (3, 1), (5, 15), (2, 17)]


def size_matrices(out_wh, hw=FRAME_HW):
    """Six boxes for one output size: the plain crop, two rotations, a flip, a shear and a box over the frame's corner."""
    H, W = hw
    k = max(out_wh) / (0.4 * W)
    return np.stack([affine_about(0.5 * W, 0.5 * H, k, 0.0, out_wh), affine_about(0.3 * W, 0.6 * H, k, 30.0, out_wh),
                     affine_about(0.6 * W, 0.4 * H, 2 * k, -7.25, out_wh), affine_about(0.5 * W, 0.5 * H, k, 0.0, out_wh, flip=True),
                     affine_about(0.4 * W, 0.5 * H, k, 0.0, out_wh, shear=(0.3, 0.1)), affine_about(2.0, 1.0, 3 * k, 0.0, out_wh)])


# ---------------------------------------------------------------------------------------------------------------
# 2. Gaussian targets
# ---------------------------------------------------------------------------------------------------------------
C_TARGET = 4.0      # |v - v64| <= C * 2^-24 * (1 + |arg|) * v64; four times the larger measured ratio
VIS_EDGES = (0.0, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1.0))), 1.0)


def _window(joints, stride_x, stride_y, sigma, trunc=np.trunc):
    """mu, ul, br per joint as generate_target computes them: int() truncates toward zero, float64 throughout."""
    tmp = sigma * 3.0
    mu_x = trunc(joints[..., 0] / stride_x + 0.5)
    mu_y = trunc(joints[..., 1] / stride_y + 0.5)
    return (mu_x, mu_y, trunc(mu_x - tmp), trunc(mu_y - tmp), trunc(mu_x + tmp + 1), trunc(mu_y + tmp + 1))


def targets_ref64(joints, vis, H, W, stride_x, stride_y, sigma, trunc=np.trunc):
    """joints [N,K,>=2] f64, vis [N,K] f32 or None -> (value [N,K,H,W] f64, the exponent's argument [N,K,H,W] f64,
    weight [N,K] f32).  The value is exp(-arg) inside the clipped window of a drawn joint and 0 elsewhere.  `trunc` is
    there for the CPU test that shows the case list tells truncation from floor."""
    joints = np.asarray(joints, dtype=np.float64)
    N, K = joints.shape[:2]
    w = np.ones((N, K), dtype=np.float32) if vis is None else np.asarray(vis, dtype=np.float32).reshape(N, K).copy()
    size = 2.0 * sigma * 3.0 + 1.0
    glen = int(math.ceil(size))                            # len(np.arange(0, size, 1))
    c0 = float(size // 2)
    _, _, ulx, uly, brx, bry = _window(joints, stride_x, stride_y, sigma, trunc)
    on = w > np.float32(0.5)
    out = on & ((ulx >= W) | (uly >= H) | (brx < 0) | (bry < 0))
    w[out] = 0
    draw = (on & ~out)[..., None, None]
    px = np.arange(W, dtype=np.float64).reshape(1, 1, 1, W)
    py = np.arange(H, dtype=np.float64).reshape(1, 1, H, 1)
    gx, gy = px - ulx[..., None, None], py - uly[..., None, None]
    win = draw & (gx >= 0) & (gy >= 0) & (gx < glen) & (gy < glen) & \
        (px < np.minimum(brx, W)[..., None, None]) & (py < np.minimum(bry, H)[..., None, None])
    arg = ((gx - c0) ** 2 + (gy - c0) ** 2) / (2.0 * sigma * sigma)
    arg = np.where(win, arg, 0.0)
    return np.where(win, np.exp(-arg), 0.0), arg, w


def targets_emulate32(joints, vis, H, W, stride_x, stride_y, sigma, arg_dtype=np.float32, exp_dtype=np.float32):
    """The kernel's formula in numpy float32: d2 = dx*dx + dy*dy, d2 / (float)(2 sigma^2), exp, each rounded to float32.
    arg_dtype / exp_dtype = float16 round the argument / the exponential to half precision (the wrong variants the bound
    must reject)."""
    v64, _, w = targets_ref64(joints, vis, H, W, stride_x, stride_y, sigma)
    joints = np.asarray(joints, dtype=np.float64)
    _, _, ulx, uly, _, _ = _window(joints, stride_x, stride_y, sigma)
    c0 = np.float32((2.0 * sigma * 3.0 + 1.0) // 2)
    dx = (np.arange(W, dtype=np.float64).reshape(1, 1, 1, W) - ulx[..., None, None]).astype(np.float32) - c0
    dy = (np.arange(H, dtype=np.float64).reshape(1, 1, H, 1) - uly[..., None, None]).astype(np.float32) - c0
    a = ((dx * dx + dy * dy) / np.float32(2.0 * sigma * sigma)).astype(arg_dtype).astype(np.float32)
    with np.errstate(over='ignore', under='ignore'):
        v = np.exp(-a).astype(exp_dtype).astype(np.float32)
    return np.where(v64 != 0, v, np.float32(0)), w


def target_ratio(v, v64, arg):
    """Worst |v - v64| / (2^-24 (1 + |arg|) v64) over the support of v64 (0 where the support is empty)."""
    on = v64 != 0
    if not on.any():
        return 0.0
    return float((np.abs(v.astype(np.float64)[on] - v64[on]) / (2.0 ** -24 * (1.0 + np.abs(arg[on])) * v64[on])).max())


def _coord(t, stride):
    """A joint coordinate whose x / stride + 0.5 is t (exactly, where t - 0.5 has few bits)."""
    return (t - 0.5) * stride


def _edge_ts(size, sigma):
    """Values of x / stride + 0.5 along one axis of `size` cells: the dot's ul at size - 1 and size, its br at 1, 0 and
    -1, the points where truncation and floor part, exact integers and integers - 2^-40."""
    tmp = sigma * 3.0
    ts = []
    for mu in range(-30, size + 30):
        ul, br = math.trunc(mu - tmp), math.trunc(mu + tmp + 1)
        if ul in (size - 1, size) or br in (1, 0, -1):
            ts.append(mu + 0.5 if mu >= 0 else mu - 0.5)
    ts += [-0.7, -0.2, 0.0, 3.0, float(size - 1), 3.0 - 2.0 ** -40, float(size) - 2.0 ** -40, 1.0 - 2.0 ** -40]
    return ts


def _edge_case(name, H, W, stride_x, stride_y, sigma, seed, K=12, vis_null=False, weight_null=False):
    rng = np.random.RandomState(seed)
    mid_x, mid_y = _coord(W // 2 + 0.5, stride_x), _coord(H // 2 + 0.5, stride_y)
    rows = []
    for t in _edge_ts(W, sigma):                          # the edge along x, y inside the map; then along y; then both
        rows.append((_coord(t, stride_x), mid_y, 1.0))
    for t in _edge_ts(H, sigma):
        rows.append((mid_x, _coord(t, stride_y), 1.0))
    for tx, ty in zip(_edge_ts(W, sigma), _edge_ts(H, sigma)):
        rows.append((_coord(tx, stride_x), _coord(ty, stride_y), 1.0))
    for v in VIS_EDGES:
        rows.append((mid_x + stride_x, mid_y - stride_y, v))
        rows.append((_coord(-0.2, stride_x), _coord(float(H - 1), stride_y), v))
    n_fill = (-len(rows)) % K + K                          # random fills around them, some invisible, some far outside
    for _ in range(n_fill):
        rows.append((rng.uniform(-8 * stride_x, (W + 8) * stride_x), rng.uniform(-8 * stride_y, (H + 8) * stride_y),
                     float(rng.choice([0.0, 1.0, 1.0, 1.0]))))
    rows = np.array(rows, dtype=np.float64)[rng.permutation(len(rows))]
    N = len(rows) // K
    joints = np.zeros((N, K, 3))
    joints[..., :2] = rows[:, :2].reshape(N, K, 2)
    joints[..., 2] = rng.uniform(-5, 5, (N, K))            # the third component is ignored
    vis = rows[:, 2].astype(np.float32).reshape(N, K)
    return dict(name=name, joints=joints, vis=None if vis_null else vis, H=H, W=W, stride_x=stride_x, stride_y=stride_y,
                sigma=sigma, weight_null=weight_null)


def _wrap_case():
    """N K H W = 4 * 33 * 128 * 128 = 2 162 688, just above the grid cap of 8192 blocks of 256."""
    rng = np.random.RandomState(11)
    N, K, H, W = 4, 33, 128, 128
    joints = np.zeros((N, K, 3))
    joints[..., 0] = rng.uniform(-30, 4 * W + 30, (N, K))
    joints[..., 1] = rng.uniform(-30, 4 * H + 30, (N, K))
    joints[0, 0, :2] = _coord(-0.2, 4.0), _coord(127.0, 4.0)
    joints[N - 1, K - 1, :2] = _coord(127.0 + 6.0 + 0.5, 4.0), _coord(-0.7, 4.0)     # the last map: ul = W - 1
    vis = (rng.uniform(size=(N, K)) > 0.15).astype(np.float32)
    vis[0, 0] = vis[N - 1, K - 1] = 1
    return dict(name='wrap', joints=joints, vis=vis, H=H, W=W, stride_x=4.0, stride_y=4.0, sigma=2.0, weight_null=False)


def target_cases():
    return [_edge_case('sigma1', 20, 28, 4.0, 4.0, 1.0, 1), _edge_case('sigma2', 20, 28, 4.0, 4.0, 2.0, 2),
            _edge_case('sigma3', 20, 28, 4.0, 4.0, 3.0, 3), _edge_case('sigma1.5', 20, 28, 4.0, 4.0, 1.5, 4),
            _edge_case('strides12x20', 12, 20, 3.0, 2.5, 2.0, 5),
            _edge_case('vis_null', 20, 28, 4.0, 4.0, 2.0, 6, vis_null=True),
            _edge_case('weight_null', 20, 28, 4.0, 4.0, 1.5, 7, weight_null=True), _wrap_case()]


TARGET_CASE_NAMES = ['sigma1', 'sigma2', 'sigma3', 'sigma1.5', 'strides12x20', 'vis_null', 'weight_null', 'wrap']


def check_targets(case, got_t, got_w):
    """-> (worst ratio, [failures]) of a kernel's (or an emulation's) output against the float64 reference."""
    v64, arg, w = targets_ref64(case['joints'], case['vis'], case['H'], case['W'], case['stride_x'], case['stride_y'],
                                case['sigma'])
    fails = []
    if not np.array_equal(got_t != 0, v64 != 0):
        fails.append('support differs at %d pixels' % int(((got_t != 0) != (v64 != 0)).sum()))
    if np.isnan(got_t).any():
        fails.append('%d pixels not written' % int(np.isnan(got_t).sum()))
    if got_w is not None and not np.array_equal(np.asarray(got_w).reshape(w.shape).view(np.uint32), w.view(np.uint32)):
        fails.append('weights differ at %d joints' % int((np.asarray(got_w).reshape(w.shape) != w).sum()))
    both = (got_t != 0) & (v64 != 0)
    ratio = target_ratio(np.where(both, got_t, 0).astype(np.float32), np.where(both, v64, 0.0), arg)
    if not ratio <= C_TARGET:
        fails.append('worst ratio %.2f above C = %g' % (ratio, C_TARGET))
    return ratio, fails


# ---------------------------------------------------------------------------------------------------------------
# 3. geometry
# ---------------------------------------------------------------------------------------------------------------
# (n, K, crop_w, crop_h, mul_x, mul_y, lifter: None or ld_in - 2K)
SCREEN_CASES = [(1, 1, 256, 256, 256.0, 256.0, 0), (5, 51, 256, 256, 64.0, 64.0, 3), (8, 32, 192, 256, 192.0, 256.0, None),
                (1, 257, 192, 256, 48.0, 64.0, 3), (50, 33, 256, 256, 256.0, 256.0, 3), (50, 33, 192, 256, 192.0, 256.0, None),
                (3, 85, 256, 256, 100.0, 90.0, 0)]


def screen_case(n, K, crop_w, crop_h, mul_x, mul_y, seed):
    """-> local [n,K,2] f32, center [n,2], scale [n,2], mean_in [2K], std_in [2K], want screen [n,2K] f64."""
    from egonet_amd import synth
    rng = np.random.RandomState(seed)
    boxes = synth.synth_boxes(n, seed=seed)
    rets = [geometry_oracle.modify_bbox(b, crop_h / crop_w) for b in boxes]
    c, s = np.stack([r['c'] for r in rets]), np.stack([r['s'] for r in rets])
    local = rng.uniform(-0.1, 1.1, (n, K, 2)).astype(np.float32)
    mean_in = rng.uniform(100, 900, 2 * K)
    std_in = rng.uniform(20, 300, 2 * K)
    mul = np.array([mul_x, mul_y]).reshape(1, 2)
    want = np.stack([geometry_oracle.crop_to_screen((local[i] * mul).astype(np.float32), c[i], s[i], (crop_h, crop_w)).reshape(-1)
                     for i in range(n)])
    return local, c, s, mean_in, std_in, want


UNNORM_CASES = [(255, 1, 0), (256, 1, 0), (257, 1, 4), (1, 1, 0), (2, 96, 0), (3, 96, 4), (7, 96, 0), (30, 96, 4)]   # (n, D, ld - D)

POSE_FAMILIES = ('wide', 'mirrored', 'flat', 'noise', 'gimbal')
POSE_N = 65
POSE_K = np.array([[707.0493, 0., 604.0814], [0., 707.0493, 180.5066], [0., 0., 1.]])


def _rot_yxz(a, b, c):
    """R = Rz(c) Rx(b) Ry(a): the matrix whose as_euler('yxz') is (a, b, c), returned by the solve as (b, a, c)."""
    ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
    Ry = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
    Rx = np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
    Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def rot_from_euler_xyz(e):
    """The rotation matrix of one returned (x, y, z) triple."""
    return _rot_yxz(e[1], e[0], e[2])


def _cuboid(l, h, w):
    """The 32 template points [3,32] of a car of size (l, h, w), as geometry_oracle.cuboid_template lays them out."""
    xc = np.array([l, l, l, l, 0, 0, 0, 0], dtype=np.float64) - l / 2
    yc = np.array([0, h, 0, h, 0, h, 0, h], dtype=np.float64) - h
    zc = np.array([w, w, 0, 0, w, w, 0, 0], dtype=np.float64) - w / 2
    corners = np.array([xc, yc, zc])
    par, chi = corners[:, geometry_oracle.EDGE_PARENT - 1], corners[:, geometry_oracle.EDGE_CHILD - 1]
    return np.hstack([corners] + [par + c * (chi - par) for c in (0.332, 0.667)])


def pose_family(name, n=POSE_N):
    """[n,32,3] float64 cuboids, fixed seed per family.
    wide: yaw +-pi, pitch +-1.5, roll +-3, 1 cm noise.  mirrored: the same mirrored in x (the best orthogonal map is a
    reflection).  flat: y scaled by 1e-6.  noise: 32 normal points.  gimbal: pitch exactly +-pi/2, no noise."""
    rng = np.random.RandomState(100 + POSE_FAMILIES.index(name))
    out = np.zeros((n, 32, 3))
    for i in range(n):
        if name == 'noise':
            out[i] = rng.normal(0, 2.0, (32, 3)) + rng.uniform(-10, 10, 3)
            continue
        T = _cuboid(rng.uniform(3, 5), rng.uniform(1.2, 2), rng.uniform(1.4, 2.2))
        a, b, c = rng.uniform(-math.pi, math.pi), rng.uniform(-1.5, 1.5), rng.uniform(-3, 3)
        if name == 'gimbal':
            b = math.pi / 2 if i % 2 else -math.pi / 2
        P = (_rot_yxz(a, b, c) @ T).T + np.array([rng.uniform(-20, 20), rng.uniform(0, 3), rng.uniform(5, 60)])
        if name != 'gimbal':
            P = P + rng.normal(0, 0.01, P.shape)
        if name == 'mirrored':
            P[:, 0] = -P[:, 0]
        if name == 'flat':
            P[:, 1] = P[:, 1] * 1e-6
        out[i] = P
    return out


def pose_kpt_x(name, n=POSE_N):
    return np.random.RandomState(200 + POSE_FAMILIES.index(name)).uniform(0, 1242, n)


def pose_reference(preds, kpt_x, K=POSE_K):
    """-> euler [n,3] (x, y, z), alpha 'proj' [n], alpha 'trans' [n], rotation matrices [n,3,3] of the oracle."""
    euler, trans = geometry_oracle.six_dof(preds)
    R = np.stack([geometry_oracle.rigid_transform(geometry_oracle.cuboid_template(p), p.T)[0] for p in preds])
    return (euler, geometry_oracle.observation_angle_proj(euler, kpt_x, K),
            geometry_oracle.observation_angle_trans(euler, trans), R)


def ang_diff(a, b):
    """|a - b| modulo 2 pi."""
    return np.abs((np.asarray(a) - np.asarray(b) + math.pi) % (2 * math.pi) - math.pi)


def check_pose(name, euler, alpha, ref_euler, ref_alpha, ref_R, tol=1e-9):
    """-> (worst difference, [failures]).  Well-posed families: angle by angle modulo 2 pi.  Gimbal: the matrix
    rebuilt from the three angles against the oracle's, the third angle exactly 0, alpha through the yaw."""
    fails = []
    if name == 'gimbal':
        d = max(float(np.abs(rot_from_euler_xyz(e) - R).max()) for e, R in zip(euler, ref_R))
        if not bool((euler[:, 2] == 0).all()):
            fails.append('gimbal: a third angle is not exactly 0')
        # alpha = yaw - ray angle: hold it against the oracle's ray angle and this solve's own yaw
        d_al = float(ang_diff(alpha - euler[:, 1], ref_alpha - ref_euler[:, 1]).max())
    else:
        d = float(ang_diff(euler, ref_euler).max())
        d_al = float(ang_diff(alpha, ref_alpha).max())
    if not d <= tol:
        fails.append('%s: rotation differs by %.3g' % (name, d))
    if not d_al <= tol:
        fails.append('%s: alpha differs by %.3g' % (name, d_al))
    return max(d, d_al), fails


def near_pi_kpt_x(yaw, delta, K=POSE_K):
    """kpt_x that puts alpha = yaw - atan2(-f, x - cx) - pi/2 at pi + delta (yaw > pi/2) or -pi + delta (yaw < -pi/2)
    before wrapping; None where no pixel column does."""
    f, cx = K[0, 0], K[0, 2]
    raw = (math.pi if yaw > 0 else -math.pi) + delta
    theta = yaw - 0.5 * math.pi - raw                      # atan2(-f, x3) must equal theta in (-pi, 0)
    if not -math.pi + 1e-3 < theta < -1e-3:
        return None
    return cx + f * math.cos(theta) / -math.sin(theta)
