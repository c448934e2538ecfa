"""Float64 numpy restatement of the reference's 3-D lifter metrics (libs/metric/criterions.py:223-301 as RError3D /
RTError3D use them, libs/common/transformation.py:99-134, normalization/operations.py:50-52): the checker of the
metric tests.  It imports nothing from the product.

The reference runs the same formulas on the float32 arrays it is given, so its distances, ``H`` and SVD are float32;
here everything after the float32 unnormalise is float64.  ``make_golden_lifter_metrics.py`` measures the gap between
the two on the fixture rows and stores it.
"""
import numpy as np
from scipy.spatial.transform import Rotation

COLS = {'R3d': 35, 'R3d+T': 39}
# result columns of a row, the order of egonet_amd/csrc/metric_math.h
GROUPS = {'R3d': (('_rT', 0, 32), ('_R', 32, 35)),
          'R3d+T': (('_rT', 0, 32), ('_R', 32, 35), ('_T', 35, 36), ('_T_xyz', 36, 39))}


def unnormalize_f32(x, mean, std):
    """operations.py:50-52 on float32 arrays: a float32 product, then a float32 sum."""
    x, mean, std = (np.asarray(v, dtype=np.float32) for v in (x, mean, std))
    return (x * std.reshape(1, -1)).astype(np.float32) + mean.reshape(1, -1)


def rigid_rotation(X, Y):
    """compute_rigid_transform(X, Y)[0], X / Y [3, N] float64."""
    Xm = X - X.mean(axis=1, keepdims=True)
    Ym = Y - Y.mean(axis=1, keepdims=True)
    U, S, Vt = np.linalg.svd(Xm @ Ym.T)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt[-1, :] *= -1
        R = Vt.T @ U.T
    return R


def rotation_errors(pred, gt):
    """[n, 3] |Euler 'xyz'| in degrees of the rotation pred -> gt; pred / gt [n, 96]."""
    n = len(pred)
    p = np.asarray(pred, dtype=np.float64).reshape(n, -1, 3)
    g = np.asarray(gt, dtype=np.float64).reshape(n, -1, 3)
    out = np.zeros((n, 3))
    for i in range(n):
        out[i] = np.abs(Rotation.from_matrix(rigid_rotation(p[i].T, g[i].T)).as_euler('xyz', degrees=True))
    return out


def joint_distances(pred, gt):
    n = len(pred)
    p = np.asarray(pred, dtype=np.float64).reshape(n, -1, 3)
    g = np.asarray(gt, dtype=np.float64).reshape(n, -1, 3)
    return np.sqrt(((g - p) ** 2).sum(axis=2))


def rows(pred, gt, layout, mean=None, std=None):
    """Per-row result columns [n, 35 | 39] float64 of float32 rows (normalised when mean / std are given)."""
    pred, gt = np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    if mean is not None:
        pred, gt = unnormalize_f32(pred, mean, std), unnormalize_f32(gt, mean, std)
    off = 3 if layout == 'R3d+T' else 0
    out = np.zeros((len(pred), COLS[layout]))
    out[:, :32] = joint_distances(pred[:, off:], gt[:, off:])
    out[:, 32:35] = rotation_errors(pred[:, off:], gt[:, off:])
    if off:
        out[:, 35:36] = joint_distances(pred[:, :3], gt[:, :3])
        out[:, 36:39] = np.abs(gt[:, :3].astype(np.float64) - pred[:, :3].astype(np.float64))
    return out


def statistics(per_row, layout):
    """{'count_rT': n, 'mean_rT': ..., 'max_rT': ..., 'min_rT': ..., ...}: update_statistics over all rows (the
    running mean of the reference equals sum / count)."""
    out = {}
    n = len(per_row)
    for name, a, b in GROUPS[layout]:
        x = per_row[:, a:b]
        out['count' + name] = n
        out['mean' + name] = x.sum(axis=0) / n
        out['max' + name] = np.maximum(-np.ones(b - a), x.max(axis=0))
        out['min' + name] = np.minimum(np.ones(b - a) * 1e16, x.min(axis=0))
    return out
