"""The references, case lists and bounds of the front-end sweep (tests/front_end_sweep.py), held without a GPU: the
crop oracle on general matrices against scipy's float bilinear sampler, the fixed-point range every swept matrix stays
in, the zero map of a singular matrix; the float64 target reference against the reference's own fixture, the edges the
case list must contain, the bound against a float32 emulation and against half-precision variants; the crop -> screen
and pose-solve references against the g++ build of csrc/pose_math.h."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

import front_end_sweep as FE
from conftest import golden
from oracle import crop_oracle, geometry_oracle
from test_crop import _image
from test_host_math import harness, _p, _pose     # noqa: F401  (the g++ harness fixture of tests/test_host_math.py)


# ---------------------------------------------------------------------------------------------------------------
# crops
# ---------------------------------------------------------------------------------------------------------------
def test_crop_oracle_vs_scipy_on_rotated_and_sheared():
    """The bound and the image of tests/test_crop.py::test_against_scipy_float_bilinear_on_a_smooth_image, on matrices
    that are not a scale plus translation."""
    img = _image(smooth=True)
    H, W = img.shape[:2]
    wh = (64, 64)
    cases = [('rot%g' % d, FE.affine_about(80.0, 48.0, 1.3, d, wh)) for d in (30.0, 90.0, 180.0, -7.25)]
    cases += [('shear', FE.affine_about(80.0, 48.0, 1.3, 0.0, wh, shear=(0.3, -0.15))),
              ('flip', FE.affine_about(80.0, 48.0, 1.3, 0.0, wh, flip=True)),
              ('flip+rot', FE.affine_about(80.0, 48.0, 1.6, 30.0, wh, flip=True))]
    for name, M in cases:
        got = crop_oracle.warp_affine_u8(img, M, wh).astype(np.float64)
        i0, i1, i2, i3, i4, i5 = FE.inverse_terms(M)
        ys, xs = np.mgrid[0:wh[1], 0:wh[0]]
        src = np.stack([i3 * xs + i4 * ys + i5, i0 * xs + i1 * ys + i2])           # (row, column) in the image
        want = np.stack([ndimage.map_coordinates(img[..., c].astype(np.float64), src, order=1, mode='constant', cval=0.0)
                         for c in range(3)], axis=2)
        inside = (src[0] > 1) & (src[0] < H - 2) & (src[1] > 1) & (src[1] < W - 2)
        assert inside.sum() > 1000, name
        worst = np.abs(got - want)[inside].max()
        print('%-9s worst |oracle - scipy| = %.3f levels over %d pixels' % (name, worst, inside.sum()))
        assert worst < 1.0, name


def test_crop_range_condition_holds_for_every_matrix():
    for wh in [(36, 21), FE.WRAP_WH] + FE.OUT_SIZES:
        FE.assert_range([M for _, _, M in FE.matrix_set(wh)], wh)
        FE.assert_range(FE.size_matrices(wh), wh)
    FE.assert_range(FE.wrap_matrices(), FE.WRAP_WH)
    assert FE.WRAP_N * FE.WRAP_WH[0] * FE.WRAP_WH[1] > 8192 * 256
    with pytest.raises(AssertionError):                    # the condition can fail: a matrix that overflows int32
        FE.assert_range([np.array([[1e-6, 0, 0], [0, 1e-6, 0.0]])], (36, 21))


def test_crop_singular_matrices_give_the_zero_map():
    """D == 0: every inverse term is 0, so X = Y = (0 + 16) >> 5 = 0 in 1/32 pixel: source pixel (0, 0) with weights
    (32, 0, 0, 0), i.e. (1024 p + 512) >> 10 = p.  Every crop pixel is the frame's first pixel."""
    img = FE.frame()
    wh = (36, 21)
    ms = {name: (f, M) for name, f, M in FE.matrix_set(wh)}
    for name in ('zeros', 'rank1'):
        assert FE.inverse_terms(ms[name][1]) == (0, 0, 0, 0, 0, 0)
        out = crop_oracle.warp_affine_u8(img, ms[name][1], wh)
        assert out.shape == (21, 36, 3) and (out == img[0, 0]).all()
    assert not crop_oracle.warp_affine_u8(img, ms['outside'][1], wh).any()
    one = np.array(FE.PIXEL_1X1, dtype=np.uint8).reshape(1, 1, 3)
    out = crop_oracle.warp_affine_u8(one, ms['1x1 frame x8'][1], wh)
    # source (x - 18) / 8, (y - 10.5) / 8: multiples of 1/16 pixel, exact in the 1/32-pixel grid, so the one pixel's
    # bilinear tent is exact too: level = floor(p * max(0, 1 - |sx|) * max(0, 1 - |sy|) + 1/2)
    ys, xs = np.mgrid[0:21, 0:36]
    tent = np.maximum(0, 1 - np.abs(xs - 18) / 8.0) * np.maximum(0, 1 - np.abs(ys - 10.5) / 8.0)
    assert np.array_equal(out, np.floor(one.astype(np.float64) * tent[..., None] + 0.5).astype(np.uint8))
    assert out[10, 18, 0] == 188 and out[10, 18 + 8:].max() == 0 and out[10, 18 + 7].max() > 0
    ref = FE.ref_crops([img, one], [0, 2, -1], [ms['rot30'][1]] * 3, wh)
    lvl0 = FE.normalise(np.zeros((21, 36, 3), np.uint8), *FE.IMAGENET)
    assert np.array_equal(ref[1], lvl0) and np.array_equal(ref[2], lvl0) and not np.array_equal(ref[0], lvl0)


# ---------------------------------------------------------------------------------------------------------------
# targets
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['s1', 's2', 'rect'])
def test_target_reference_reproduces_the_fixture(tag):
    """Support and weight exactly, values within the fixture's 2e-7 (tests/test_gpu_train_ops.py)."""
    g = golden('targets.npz')
    inp, hs = g[tag + '/input_size'], g[tag + '/heatmap_size']
    v64, arg, w = FE.targets_ref64(g[tag + '/joints'], g[tag + '/vis'], int(hs[0]), int(hs[1]), float(inp[0]) / float(hs[0]),
                                   float(inp[1]) / float(hs[1]), float(g[tag + '/sigma']))
    want = g[tag + '/target']
    assert np.array_equal(v64 != 0, want != 0)
    assert np.array_equal(w.reshape(-1), g[tag + '/weight'].reshape(-1))
    assert np.abs(v64 - want).max() <= 2e-7
    ratio = FE.target_ratio(want, v64, arg)
    print('%s: the fixture (numpy float32) against float64: worst ratio %.2f' % (tag, ratio))
    assert ratio <= FE.C_TARGET


def test_target_cases_hold_every_edge_the_issue_names():
    cases = {c['name']: c for c in FE.target_cases()}
    assert list(cases) == FE.TARGET_CASE_NAMES
    assert {cases[n]['sigma'] for n in ('sigma1', 'sigma2', 'sigma3', 'sigma1.5')} == {1.0, 2.0, 3.0, 1.5}
    for name, c in cases.items():
        if name == 'wrap':
            continue
        H, W = c['H'], c['W']
        j = c['joints'].reshape(-1, 3)
        vis = np.ones(len(j), np.float32) if c['vis'] is None else c['vis'].reshape(-1)
        on = vis > 0.5
        mu_x, mu_y, ulx, uly, brx, bry = FE._window(j, c['stride_x'], c['stride_y'], c['sigma'])
        inx, iny = (ulx < W) & (brx >= 0), (uly < H) & (bry >= 0)
        # each border value with the other axis inside the map, so that this comparison alone decides the weight
        assert {W - 1, W} <= set(ulx[on & iny]) and {1, 0, -1} <= set(brx[on & iny]), name
        assert {H - 1, H} <= set(uly[on & inx]) and {1, 0, -1} <= set(bry[on & inx]), name
        tx, ty = j[:, 0] / c['stride_x'] + 0.5, j[:, 1] / c['stride_y'] + 0.5
        for t in (tx[on], ty[on]):
            assert np.isclose(t, -0.7, atol=1e-12).any() and np.isclose(t, -0.2, atol=1e-12).any() and (t == 0.0).any()
            assert (t == 3.0).any() and (t == 3.0 - 2.0 ** -40).any()
        if c['vis'] is not None:
            assert set(FE.VIS_EDGES) <= set(float(v) for v in c['vis'].ravel())
        _, _, w = FE.targets_ref64(c['joints'], c['vis'], H, W, c['stride_x'], c['stride_y'], c['sigma'])
        assert (w == 0).any() and (w == 1).any()
    assert FE.VIS_EDGES[2] > 0.5 and np.float32(FE.VIS_EDGES[2]) == np.nextafter(np.float32(0.5), np.float32(1))
    assert cases['vis_null']['vis'] is None and cases['weight_null']['weight_null']
    c = cases['strides12x20']
    assert (c['H'], c['W']) == (12, 20) and c['stride_x'] != c['stride_y']
    c = cases['wrap']
    assert c['joints'].shape[0] * c['joints'].shape[1] * c['H'] * c['W'] > 8192 * 256
    # truncation and floor part on these lists: a reference that floors has another support
    c = cases['sigma1.5']
    v64, _, w = FE.targets_ref64(c['joints'], c['vis'], c['H'], c['W'], c['stride_x'], c['stride_y'], c['sigma'])
    f64, _, fw = FE.targets_ref64(c['joints'], c['vis'], c['H'], c['W'], c['stride_x'], c['stride_y'], c['sigma'], trunc=np.floor)
    assert not np.array_equal(f64 != 0, v64 != 0) and not np.array_equal(fw, w)


def test_target_bound_emulation_and_half_precision_mutants():
    """C_TARGET is four times the larger of: the worst ratio of the float32 emulation below, the kernel's own on the
    GPU.  An argument or an exponential rounded to half precision misses it by two orders of magnitude."""
    worst, w16a, w16e = 0.0, 0.0, 0.0
    for c in FE.target_cases():
        a = (c['joints'], c['vis'], c['H'], c['W'], c['stride_x'], c['stride_y'], c['sigma'])
        v64, arg, w64 = FE.targets_ref64(*a)
        v32, w32 = FE.targets_emulate32(*a)
        ratio, fails = FE.check_targets(c, v32, w32)
        assert not fails, (c['name'], fails)
        worst = max(worst, ratio)
        w16a = max(w16a, FE.target_ratio(FE.targets_emulate32(*a, arg_dtype=np.float16)[0], v64, arg))
        w16e = max(w16e, FE.target_ratio(FE.targets_emulate32(*a, exp_dtype=np.float16)[0], v64, arg))
    print('float32 emulation: worst ratio %.3f (C = %g); half-precision argument %.0f, half-precision exponential %.0f'
          % (worst, FE.C_TARGET, w16a, w16e))
    assert worst <= FE.C_TARGET / 4 + 1e-9
    assert w16a > 100 * FE.C_TARGET and w16e > 100 * FE.C_TARGET


# ---------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------
def test_screen_cases_vs_host_build(harness):                               # noqa: F811
    assert {n * K for n, K, *_ in FE.SCREEN_CASES} >= {1, 255, 256, 257, 33 * 50}
    assert {(cw, ch) for _, _, cw, ch, *_ in FE.SCREEN_CASES} == {(256, 256), (192, 256)}
    for i, (n, K, cw, ch, mx, my, _) in enumerate(FE.SCREEN_CASES):
        local, c, s, _, _, want = FE.screen_case(n, K, cw, ch, mx, my, seed=i)
        out = np.zeros((n, 2 * K))
        harness.harness_crop_to_screen(_p(local), n, K, C.c_double(mx), C.c_double(my), _p(c), _p(s), cw, ch, _p(out))
        np.testing.assert_allclose(out, want, rtol=0, atol=1e-9)


def test_pose_families_are_what_they_claim():
    for name in FE.POSE_FAMILIES:
        P = FE.pose_family(name)
        assert P.shape == (FE.POSE_N, 32, 3) and FE.POSE_N >= 65
        euler, _, _, R = FE.pose_reference(P, FE.pose_kpt_x(name))
        assert np.allclose(np.linalg.det(R), 1.0)
        if name == 'wide':
            assert np.abs(euler[:, 1]).max() > 3.0 and np.abs(euler[:, 0]).max() > 1.3 and np.abs(euler[:, 2]).max() > 2.5
        if name == 'mirrored':     # without the reflection fix V U^T has determinant -1 for every instance
            for p in P:
                x, y = geometry_oracle.cuboid_template(p), p.T
                u, _, vt = np.linalg.svd((x - x.mean(1, keepdims=True)) @ (y - y.mean(1, keepdims=True)).T)
                assert np.linalg.det(vt.T @ u.T) < 0
        if name == 'gimbal':
            assert np.abs(np.abs(R[:, 2, 1]) - 1).max() < 1e-12
            assert {1.0, -1.0} == set(np.sign(R[:, 2, 1]))


def test_host_pose_families_vs_oracle(harness):                             # noqa: F811
    for name in FE.POSE_FAMILIES:
        P, kx = FE.pose_family(name), FE.pose_kpt_x(name)
        ref_e, ref_proj, ref_trans, ref_R = FE.pose_reference(P, kx)
        for mode, ref_a in ((0, ref_proj), (1, ref_trans)):
            e, a = _pose(harness, P, kx, FE.POSE_K, mode)
            worst, fails = FE.check_pose(name, e, a, ref_e, ref_a, ref_R)
            print('%-8s mode %d: worst difference from the oracle %.3g' % (name, mode, worst))
            assert not fails, fails


def test_host_pose_alpha_next_to_pi(harness):                               # noqa: F811
    P = FE.pose_family('wide')
    ref_e, _, _, _ = FE.pose_reference(P, FE.pose_kpt_x('wide'))
    rows = [(i, d, FE.near_pi_kpt_x(ref_e[i, 1], d)) for i in range(len(P)) for d in (5e-10, -5e-10)]
    rows = [r for r in rows if r[2] is not None]
    assert len(rows) >= 16 and {np.sign(ref_e[i, 1]) for i, _, _ in rows} == {1.0, -1.0}
    idx = np.array([r[0] for r in rows])
    kx = np.array([r[2] for r in rows])
    want = geometry_oracle.observation_angle_proj(ref_e[idx], kx, FE.POSE_K)
    assert (np.abs(np.abs(want) - np.pi) < 1e-9).all()
    assert (want > 0).any() and (want < 0).any()
    e, a = _pose(harness, P[idx], kx, FE.POSE_K, 0)
    assert FE.ang_diff(a, want).max() <= 1e-9 and (np.abs(a) <= np.pi).all()
