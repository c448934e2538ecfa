"""The exact per-instance code of the key-point metric kernel (csrc/kpt_metric_math.h), compiled for the host with
g++: the closed-form inverse crop affine against ``img_proc.get_affine_transform(..., inv=1)``, and the distance /
PCK / visibility code on the reference-generated ``src_coord`` of tests/golden/metric.npz."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import golden, ROOT
from egonet_amd.common import img_proc as lip
from egonet_amd.metric import criterions

BUILD = os.path.join(ROOT, 'tests', '_build')

# Largest difference of a transformed point, closed form against np.linalg.solve, measured over every case of
# test_inverse_affine_matches_get_affine_transform on the CPU (where the header is the very code the kernel runs):
# 2.3e-13 px.  The bound is 10 x that (and stays below the 1e-6 px ceiling).
MEASURED_PX = 2.3e-13
BOUND_PX = min(10 * MEASURED_PX, 1e-6)


@pytest.fixture(scope='module')
def harness():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, 'kpt_metric_math_harness.so')
    src = os.path.join(ROOT, 'tests', 'kpt_metric_math_harness.cpp')
    subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-o', so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _window_points(w, h, seed):
    """float32 points of the crop window: its corners and centre, the heat-map pixel grid's extremes, seeded ones
    inside and a few outside."""
    rng = np.random.RandomState(seed)
    fixed = [[0, 0], [w, 0], [0, h], [w, h], [w / 2, h / 2], [w - 1, h - 1], [0.25, 0.75]]
    inside = rng.rand(40, 2) * [w, h]
    outside = (rng.rand(8, 2) - 0.5) * 3 * [w, h]
    return np.concatenate([fixed, inside, outside]).astype(np.float32)


def _affine_cases():
    g = golden('metric.npz')
    cases = [('fixture%d' % i, g['center'][i], g['scale'][i], float(g['rotation'][i]), (64.0, 64.0)) for i in range(4)]
    rng = np.random.RandomState(11)
    for rot in (0.0, 90.0, -90.0, 180.0, 33.3):
        for size in ((256.0, 256.0), (192.0, 256.0), (288, 384)):           # (w, h); ints like a yaml input_size
            c = rng.rand(2) * [1242.0, 375.0]
            s = 0.2 + rng.rand() * 2.0
            cases.append(('square rot %g %s' % (rot, size), c, np.array([s, s]), rot, size))
            cases.append(('non-square rot %g %s' % (rot, size), c, np.array([s, s * (0.5 + rng.rand())]), rot, size))
    return cases


def test_inverse_affine_matches_get_affine_transform(harness):
    """Transformed window points within BOUND_PX of the three-point solve (measured: 2.3e-13 px at most, over the
    four fixture instances with rotations 0 / 12.5 / -30 / 0, seeded boxes with rotation 0, +-90, 180 and 33.3,
    square and non-square scale, square and non-square image_size)."""
    worst = 0.0
    for seed, (name, c, s, rot, (w, h)) in enumerate(_affine_cases()):
        want_t = lip.get_affine_transform(c, s, rot, (h, w), inv=1)
        pts = _window_points(w, h, seed)
        want = lip.affine_transform_modified(pts, want_t)
        T = np.zeros((2, 3))
        harness.harness_kpt_inv_affine(_p(_f64(c)), _p(_f64(s)), _p(_f64([rot])), 1, C.c_double(w), C.c_double(h),
                                       _p(T))
        got = np.zeros((len(pts), 2))
        harness.harness_kpt_to_source(_p(T), _p(pts), len(pts), _p(got))
        diff = np.abs(got - want).max()
        worst = max(worst, diff)
        assert diff <= BOUND_PX, (name, diff)
    print('largest difference of a transformed point: %.3e px (bound %.1e)' % (worst, BOUND_PX))


@pytest.mark.parametrize('tag,correct', [('hard', [0, 3, 5]), ('soft', [0, 0, 4]), ('coords', [0, 2, 2]),
                                         ('norot', [0, 3, 5])])
def test_distance_pck_visibility_on_the_golden_src_coord(harness, tag, correct):
    """The reference's own src_coord through the per-instance code: cnt == 103, the golden PCK counts exactly, avg to
    rtol 1e-12.  Exact counts are fair: every visible joint is at least 0.73 px from every PCK threshold."""
    g = golden('metric.npz')
    src, gt = _f64(g[tag + '/src_coord']), _f64(g['original_joints'])
    n, K = gt.shape[:2]
    # the margin of this fixture, asserted before the counts: >= 100 x the 5e-3 px coordinate tolerance
    dist = np.sqrt(((gt[:, :, :2] - src) ** 2).sum(axis=2))
    den = (gt[:, :, 1].max(axis=1) - gt[:, :, 1].min(axis=1)) / 3
    margin = np.abs(dist[:, :, None] - criterions.PCK_THRES[None, None] * den[:, None, None])[gt[:, :, 2] != 0].min()
    assert margin >= 100 * 5e-3, margin
    out = np.zeros(5)
    harness.harness_kpt_stats(_p(src), _p(gt), n, K, _p(out))
    assert out[0] == 103
    np.testing.assert_array_equal(out[2:], correct)
    dists, want_correct = [], np.zeros(3)
    for i in range(n):
        dists += criterions.get_distance(gt[i], src[i])
        want_correct += criterions.get_PCK(src[i], gt[i])
    np.testing.assert_array_equal(out[2:], want_correct)
    np.testing.assert_allclose(out[1] / out[0], sum(dists) / len(dists), rtol=1e-12)
    if tag != 'norot':
        assert int(g[tag + '/cnt']) == 103
        np.testing.assert_array_equal(g[tag + '/correct_cnt'], correct)
    np.testing.assert_allclose(out[1] / out[0], float(g[tag + '/avg']), rtol=1e-12)


def test_instance_without_a_visible_joint_and_a_flat_instance(harness):
    """No visible joint: nothing counted.  All annotated joints on one row: denominator 0, no PCK hit, the distances
    still count (get_PCK compares distance < 0)."""
    rng = np.random.RandomState(2)
    gt = np.concatenate([rng.rand(2, 7, 2) * 100, np.ones((2, 7, 1))], axis=2)
    gt[0, :, 2] = 0.0
    gt[1, :, 1] = 40.0
    src = gt[:, :, :2] + rng.rand(2, 7, 2)
    out = np.zeros(5)
    harness.harness_kpt_stats(_p(_f64(src)), _p(_f64(gt)), 2, 7, _p(out))
    assert out[0] == 7 and np.array_equal(out[2:], np.zeros(3))
    np.testing.assert_allclose(out[1], sum(criterions.get_distance(gt[1], src[1])), rtol=1e-12)
