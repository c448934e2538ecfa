"""The reprojection refinement of lifted cuboids on the host: egn_pnp_refine_host_f64 (csrc/pnp_math.h, the code the
device kernel instantiates per wave) through ctypes, against the known truth of noise-free cuboids, against
scipy.optimize.least_squares(method='lm') on noisy ones, and through the reference-shaped API of a CPU model.

Bounds (from a numpy / scipy prototype of the same Levenberg-Marquardt iteration on these distributions, each with
margin): noise-free recovery 1e-6 m (prototype 2e-13), final cost 1e-12 px^2, dims 1e-9 m; noisy cost at most scipy's
times (1 + 1e-9) (prototype excess <= 1e-14); |J^T r| <= 1e-6 |J|_F |r| with a central-difference Jacobian (prototype
1.8e-8, limited by the differencing).  Points are not compared with scipy's: it stops up to 6e-5 m short of the
minimum on the far cases."""
import math

import numpy as np
import pytest

import pnp_cases as pc
from egonet_amd import _lib


@pytest.fixture(scope='module')
def L():
    return _lib.lib()


@pytest.fixture(scope='module')
def clean33():
    return pc.make(64, J=33, seed=11)


def _check_recovered(out, case):
    assert (out['status'] == 1).all(), out['status']
    err = np.abs(out['refined'] - case['pts']).max()
    print('max |refined - truth| = %.3e m, max cost = %.3e px^2, max iters = %d'
          % (err, out['cost'][:, 1].max(), out['iters'].max()))
    assert err <= 1e-6
    assert (out['cost'][:, 1] <= 1e-12).all()
    assert np.abs(out['dims'] - case['dims']).max() <= 1e-9
    assert np.abs(out['refined'][:, 0] - out['rt'][:, 9:]).max() == 0.0


@pytest.mark.parametrize('with_root0', [True, False])
@pytest.mark.parametrize('J', [33, 9])
def test_noise_free_recovery(L, J, with_root0):
    case = pc.make(64, J=J, seed=11 + J)
    rc, out = pc.host_refine(L, case['shape'], case['k'], case['intr'], root0=case['root0'] if with_root0 else None)
    assert rc == 0
    _check_recovered(out, case)
    assert (out['cost'][:, 1] <= out['cost'][:, 0]).all()
    R = out['rt'][:, :9].reshape(-1, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12


def _residuals(x, shape, k, intr):
    """Test-local residual function: x = (rotation vector, T)."""
    R = pc.rodrigues(x[:3])
    pts = np.concatenate([np.zeros((1, 3)), shape]) @ R.T + x[3:]
    u = intr[0] * pts[:, 0] / pts[:, 2] + intr[2]
    v = intr[1] * pts[:, 1] / pts[:, 2] + intr[3]
    return np.stack([u - k[:, 0], v - k[:, 1]], 1).reshape(-1)


def _rotvec(R):
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(R).as_rotvec()


def test_noisy_optimum_against_scipy(L):
    from scipy.optimize import least_squares
    case = pc.make(64, J=33, seed=23, noisy=True)
    rc, out = pc.host_refine(L, case['shape'], case['k'], case['intr'], root0=case['root0'], max_shift=math.inf)
    assert rc == 0
    assert (out['status'] == 1).all()
    assert (out['cost'][:, 1] <= out['cost'][:, 0]).all()
    worst_excess, worst_grad = -np.inf, 0.0
    for i in range(64):
        args = (case['shape'][i], case['k'][i], case['intr'][i])
        x_ours = np.concatenate([_rotvec(out['rt'][i, :9].reshape(3, 3)), out['rt'][i, 9:]])
        r = _residuals(x_ours, *args)
        assert abs(r @ r - out['cost'][i, 1]) <= 1e-9 * out['cost'][i, 1]      # the reported cost is the cost
        x0 = np.concatenate([np.zeros(3), case['root0'][i]])
        ref = least_squares(_residuals, x0, args=args, method='lm', xtol=1e-15, ftol=1e-15, gtol=1e-15)
        c_ref = float(ref.fun @ ref.fun)
        worst_excess = max(worst_excess, out['cost'][i, 1] / c_ref - 1.0)
        assert out['cost'][i, 1] <= c_ref * (1 + 1e-9), (i, out['cost'][i, 1], c_ref)
        Jn = np.empty((r.size, 6))
        for d in range(6):
            h = 1e-6 * max(1.0, abs(x_ours[d]))
            e = np.zeros(6)
            e[d] = h
            Jn[:, d] = (_residuals(x_ours + e, *args) - _residuals(x_ours - e, *args)) / (2 * h)
        g = np.linalg.norm(Jn.T @ r) / (np.linalg.norm(Jn) * np.linalg.norm(r))
        worst_grad = max(worst_grad, g)
        assert g <= 1e-6, (i, g)
    print('max cost / scipy - 1 = %.3e, max |J^T r| / (|J|_F |r|) = %.3e' % (worst_excess, worst_grad))


@pytest.mark.parametrize('with_root0', [True, False])
def test_zero_weights_drop_garbage(L, clean33, with_root0):
    k, w = pc.garbage_weights(clean33)
    rc, out = pc.host_refine(L, clean33['shape'], k, clean33['intr'], weights=w,
                             root0=clean33['root0'] if with_root0 else None)
    assert rc == 0
    _check_recovered(out, clean33)


def test_shift_rule(L, clean33):
    c = clean33
    ray = c['root'] / np.linalg.norm(c['root'], axis=1, keepdims=True)
    root0 = c['root'] + 8.0 * ray
    rc, out = pc.host_refine(L, c['shape'], c['k'], c['intr'], root0=root0)
    assert rc == 0
    assert (out['status'] == 0).all(), out['status']
    want = np.concatenate([root0[:, None], root0[:, None] + c['shape']], 1)
    assert np.array_equal(out['refined'], want)
    assert np.array_equal(out['rt'][:, :9], np.tile(np.eye(3).reshape(-1), (64, 1)))
    assert np.array_equal(out['rt'][:, 9:], root0)
    rc, out = pc.host_refine(L, c['shape'], c['k'], c['intr'], root0=root0, max_shift=math.inf)
    assert rc == 0
    _check_recovered(out, c)


def test_unusable_inputs(L, clean33):
    c = {k: v[:4].copy() for k, v in clean33.items()}
    root0 = c['root0'].copy()
    root0[1, 2] = -1.0
    rc, out = pc.host_refine(L, c['shape'], c['k'], c['intr'], root0=root0)
    assert rc == 0
    assert list(out['status']) == [1, -1, 1, 1]
    assert np.array_equal(out['refined'][1], np.concatenate([root0[1:2], root0[1:2] + c['shape'][1]]))
    for v in out.values():
        assert np.isfinite(v).all()
    # n = 0: nothing is touched, NULL pointers are fine
    assert L.egn_pnp_refine_host_f64(None, None, None, None, None, 0, 33, 5.0, None, None, None, None, None, None) == 0
    for J in (1, 65):
        buf = np.zeros(65 * 3)
        i32 = np.zeros(1, dtype=np.int32)
        p = buf.ctypes.data
        assert L.egn_pnp_refine_host_f64(p, p, p, None, None, 1, J, 5.0, p, p, p, i32.ctypes.data, i32.ctypes.data,
                                         p) == -1
    assert L.egn_pnp_refine_host_f64(None, None, None, None, None, -1, 33, 5.0, None, None, None, None, None,
                                     None) == -1
    assert L.egn_pnp_refine_host_f64(None, None, None, None, None, 0, 33, -1.0, None, None, None, None, None,
                                     None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the reference-shaped API on a CPU model
def _cpu_model():
    from egonet_amd import configs, synth
    from egonet_amd.model.egonet import EgoNet
    cfg = configs.hrnet_config(8, (64, 64), 33, 'coordinates', modules=(1, 1, 1), num_blocks=1, lifter_neurons=128)
    ego = EgoNet(cfg, pre_trained=False)
    ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    return ego.eval()


def _record(case, with_boxes3d):
    n = len(case['k'])
    rec = {'kpts_3d_pred': case['shape'].copy(), 'kpts_2d_pred': [case['k'][i].reshape(1, -1) for i in range(n)],
           'K': pc.KITTI_K.copy()}
    rows = []
    for i in range(n):
        l, h, w = case['dims'][i]
        loc = case['root0'][i] + np.array([0., h / 2, 0.]) if with_boxes3d else np.array([-1000.] * 3)
        rows.append({'class': 'Car', 'truncation': 0., 'occlusion': 0., 'alpha': 0., 'bbox': [0., 0., 1., 1.],
                     'dimensions': [l, h, w], 'locations': list(loc), 'rot_y': 0., 'score': 1.0})
    rec['raw_txt_format'] = rows
    return rec


def _wrap_abs(a):
    return np.abs((a + np.pi) % (2 * np.pi) - np.pi)


@pytest.mark.parametrize('with_boxes3d', [True, False])
def test_gather_lifting_results_refine(with_boxes3d):
    ego = _cpu_model()
    case = pc.make(12, J=33, seed=31, yaw_only_pert=math.radians(10.0))
    plain = ego.gather_lifting_results(_record(case, with_boxes3d), alpha_mode='trans')
    # today's result for the same record, restated: the pose of the lifted shape and "the first point" as translation
    euler0, trans0 = ego.get_6d_rep(case['shape'])
    assert np.array_equal(plain['euler_angles'], euler0) and np.array_equal(plain['translation'], trans0)
    assert np.array_equal(plain['alphas'], ego.get_observation_angle_trans(euler0, trans0))
    assert 'kpts_3d_refined' not in plain and 'refine_status' not in plain
    assert _wrap_abs(plain['euler_angles'][:, 1] - case['yaw']).min() > math.radians(9.0)    # the 10 deg error is there

    rec = ego.gather_lifting_results(_record(case, with_boxes3d), alpha_mode='trans', refine=True)
    assert (rec['refine_status'] == 1).all()
    assert _wrap_abs(rec['euler_angles'][:, 1] - case['yaw']).max() <= 1e-6
    assert np.abs(rec['translation'] - case['root']).max() <= 1e-6
    assert np.abs(rec['kpts_3d_refined'] - case['pts']).max() <= 1e-6
    want_alpha = ego.get_observation_angle_trans(rec['euler_angles'], case['root'])
    assert _wrap_abs(rec['alphas'] - want_alpha).max() <= 1e-6
    # post_process passes the switch on
    recs = ego.post_process({'a.png': _record(case, with_boxes3d)}, alpha_mode='proj', refine=True)
    assert np.abs(recs['a.png']['translation'] - case['root']).max() <= 1e-6


def test_refine_pnp_numpy_and_argument_errors():
    import torch
    ego = _cpu_model()
    case = pc.make(5, J=33, seed=37)
    out = ego.refine_pnp(case['shape'], case['k'].reshape(5, -1), pc.KITTI_K, roots=case['root0'])
    assert set(out) == {'kpts_3d_refined', 'rt', 'cost', 'iters', 'status', 'dims'}
    assert (out['status'] == 1).all() and np.abs(out['kpts_3d_refined'] - case['pts']).max() <= 1e-6
    out2 = ego.refine_pnp(case['shape'], case['k'], np.tile(pc.KITTI_K, (5, 1, 1)))     # [n,3,3], no roots
    assert (out2['status'] == 1).all() and np.abs(out2['kpts_3d_refined'] - case['pts']).max() <= 1e-6
    crops = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match='refine must be'):
        ego.infer_crops(crops, np.zeros((1, 2)), np.ones((1, 2)), K=pc.KITTI_K, refine='bogus')
    with pytest.raises(ValueError, match='needs the intrinsics'):
        ego.infer_crops(crops, np.zeros((1, 2)), np.ones((1, 2)), refine='pnp')
