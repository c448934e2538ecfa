"""The exact per-row code of the lifter-metric kernel (csrc/metric_math.h), compiled for the host with g++, against
the float64 restatement of the reference (tests/lifter_metrics_ref.py) on the reference-generated fixture rows, and
against scipy at gimbal lock."""
import ctypes as C
import os
import subprocess
import warnings

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from conftest import golden, ROOT
import lifter_metrics_ref as ref

BUILD = os.path.join(ROOT, 'tests', '_build')


@pytest.fixture(scope='module')
def harness():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, 'metric_math_harness.so')
    src = os.path.join(ROOT, 'tests', 'metric_math_harness.cpp')
    subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-o', so, src])
    return C.CDLL(so)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _rows(h, pred, gt, layout, mean=None, std=None):
    pred, gt = np.ascontiguousarray(pred, dtype=np.float32), np.ascontiguousarray(gt, dtype=np.float32)
    out = np.zeros((len(pred), ref.COLS[layout]))
    if mean is not None:
        mean = np.ascontiguousarray(mean, dtype=np.float32).reshape(-1)
        std = np.ascontiguousarray(std, dtype=np.float32).reshape(-1)
    h.harness_metric_rows(_p(pred), _p(gt), len(pred), int(layout == 'R3d+T'), _p(mean), _p(std), _p(out))
    return out


@pytest.mark.parametrize('layout', ['R3d', 'R3d+T'])
def test_rows_match_the_restatement_on_the_fixture(harness, layout):
    """Distances to 1e-9 m, Euler errors to 1e-9 rad: the bound of the pose solve's Kabsch angles
    (test_host_math.py:40)."""
    g = golden('lifter_metrics.npz')
    p = layout + '/'
    want = ref.rows(g[p + 'pred'], g[p + 'gt'], layout, g[p + 'mean_out'], g[p + 'std_out'])
    got = _rows(harness, g[p + 'pred'], g[p + 'gt'], layout, g[p + 'mean_out'], g[p + 'std_out'])
    assert np.isfinite(got).all()
    np.testing.assert_allclose(np.deg2rad(got[:, 32:35]), np.deg2rad(want[:, 32:35]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.delete(got, [32, 33, 34], axis=1), np.delete(want, [32, 33, 34], axis=1),
                               rtol=0, atol=1e-9)
    assert want[:, 32:35].max() > 5.0 and want[:, 32:35].min() < 1e-3          # several degrees down to almost none
    # without statistics: the rows as they are
    pu = ref.unnormalize_f32(g[p + 'pred'], g[p + 'mean_out'], g[p + 'std_out'])
    gu = ref.unnormalize_f32(g[p + 'gt'], g[p + 'mean_out'], g[p + 'std_out'])
    assert np.array_equal(_rows(harness, pu, gu, layout), got)                # the float32 unnormalise is numpy's


def test_gimbal_lock_rows_follow_scipy(harness):
    """beta = +-90 deg built by hand: scipy sets the third angle to zero, so does the header."""
    mats, want = [], []
    for beta in (90.0, -90.0):
        for alpha in (0.0, 25.0, -140.0):
            R = Rotation.from_euler('xyz', [alpha, beta, 0.0], degrees=True).as_matrix()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', UserWarning)                    # "Gimbal lock detected"
                want.append(np.abs(Rotation.from_matrix(R).as_euler('xyz', degrees=True)))
            mats.append(R)
    for ang in ([10.0, 20.0, 30.0], [-170.0, 89.0, 45.0], [3.0, -60.0, -100.0]):   # and away from it
        R = Rotation.from_euler('xyz', ang, degrees=True).as_matrix()
        mats.append(R)
        want.append(np.abs(Rotation.from_matrix(R).as_euler('xyz', degrees=True)))
    mats = np.ascontiguousarray(np.stack(mats))
    out = np.zeros((len(mats), 3))
    harness.harness_euler_xyz(_p(mats), len(mats), _p(out))
    want = np.stack(want)
    assert np.all(want[:6, 2] == 0.0) and np.all(out[:6, 2] == 0.0)
    np.testing.assert_allclose(np.deg2rad(out), np.deg2rad(want), rtol=0, atol=1e-9)


def test_degenerate_rows_are_finite(harness):
    """H = 0 (every predicted point equal): rotation error (0, 0, 0) like the reference's identity U, V; rank 1:
    finite, unspecified."""
    rng = np.random.RandomState(5)
    gt = rng.randn(3, 96).astype(np.float32)
    pred = gt.copy()
    pred[0] = np.tile(np.array([1.0, 2.0, 3.0], dtype=np.float32), 32)          # H = 0
    line = np.outer(np.linspace(-1, 1, 32), [1.0, 0.5, -2.0]).astype(np.float32)
    pred[1] = line.reshape(-1)                                                   # rank 1: points on a line
    pred[2] = line.reshape(-1)
    gt[2] = (2 * line).reshape(-1)                                               # both on one line
    got = _rows(harness, pred, gt, 'R3d')
    assert np.isfinite(got).all()
    assert np.array_equal(got[0, 32:35], np.zeros(3))
    np.testing.assert_allclose(ref.rotation_errors(pred[:1], gt[:1]), np.zeros((1, 3)), atol=1e-12)
    out = np.zeros(3)
    harness.harness_rotation_error(_p(np.zeros(9)), _p(out))
    assert np.array_equal(out, np.zeros(3))
