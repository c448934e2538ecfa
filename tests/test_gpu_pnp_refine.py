"""The reprojection refinement on the device: egn_pnp_refine_f64 (one wave per instance) against its host twin (the same
csrc/pnp_math.h as a plain loop) on the inputs of tests/test_pnp_refine_cpu.py, on a side stream, inside
EgoNet.infer_crops(refine='pnp') and through tools/inference_kitti.py --refine pnp --write-3d.

Device against host: statuses and shift decisions equal; refined to 1e-7 m, rt and dims to 1e-9.  Both sides iterate to
the same minimum with a fast final convergence; what remains is rounding times the depth conditioning (about 2.5 m per
pixel at 60 m), of the order of 1e-10 m, so 1e-7 leaves three decades."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

import pnp_cases as pc
from egonet_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

pytestmark = pytest.mark.gpu

KEYS = ('refined', 'rt', 'cost', 'iters', 'status', 'dims')


def dev_refine(shape, k, intr, weights=None, root0=None, max_shift=5.0, stream=None):
    """egn_pnp_refine_f64 on uploaded copies -> (return code, dict of device tensors)."""
    L = _lib.lib()
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()   # noqa: E731
    n, J = k.shape[0], k.shape[1]
    d_shape, d_k, d_intr, d_w, d_r0 = up(shape), up(k), up(intr), up(weights), up(root0)
    out = {'refined': torch.full((n, J, 3), float('nan'), dtype=torch.float64, device='cuda'),
           'rt': torch.full((n, 12), float('nan'), dtype=torch.float64, device='cuda'),
           'cost': torch.full((n, 2), float('nan'), dtype=torch.float64, device='cuda'),
           'iters': torch.full((n,), -7, dtype=torch.int32, device='cuda'),
           'status': torch.full((n,), -7, dtype=torch.int32, device='cuda'),
           'dims': torch.full((n, 3), float('nan'), dtype=torch.float64, device='cuda')}
    torch.cuda.synchronize()
    s = _lib.current_stream() if stream is None else C.c_void_p(stream.cuda_stream)
    rc = L.egn_pnp_refine_f64(_lib.ptr(d_shape), _lib.ptr(d_k), _lib.ptr(d_intr), _lib.ptr(d_w), _lib.ptr(d_r0), n, J,
                              float(max_shift), *[_lib.ptr(out[key]) for key in KEYS], s)
    out['_keep'] = (d_shape, d_k, d_intr, d_w, d_r0)
    return rc, out


def variants(n, J):
    """The inputs of the CPU tests at this size: name -> keyword arguments of the two refine helpers."""
    clean = pc.make(n, J=J, seed=100 + n + J)
    noisy = pc.make(n, J=J, seed=200 + n + J, noisy=True)
    gk, gw = pc.garbage_weights(clean, n_bad=10 if J == 33 else 3)
    ray = clean['root'] / np.linalg.norm(clean['root'], axis=1, keepdims=True)
    far = clean['root'] + 8.0 * ray
    behind = clean['root0'].copy()
    behind[n // 2, 2] = -1.0
    base = dict(shape=clean['shape'], k=clean['k'], intr=clean['intr'])
    return {
        'clean_root0': dict(base, root0=clean['root0']),
        'clean_weak_perspective': dict(base),
        'noisy': dict(shape=noisy['shape'], k=noisy['k'], intr=noisy['intr'], root0=noisy['root0'], max_shift=math.inf),
        'weights_root0': dict(base, k=gk, weights=gw, root0=clean['root0']),
        'weights_weak_perspective': dict(base, k=gk, weights=gw),
        'shift_discarded': dict(base, root0=far),
        'shift_unbounded': dict(base, root0=far, max_shift=math.inf),
        'behind_camera': dict(base, root0=behind),
    }


@pytest.mark.parametrize('J', [33, 9])
@pytest.mark.parametrize('n', [1, 5, 64, 257])
def test_device_matches_host_twin(hip_lib, n, J):
    for name, kw in variants(n, J).items():
        rc_h, host = pc.host_refine(hip_lib, **kw)
        rc_d, dev = dev_refine(**kw)
        rc_d2, dev2 = dev_refine(**kw)
        torch.cuda.synchronize()
        assert rc_h == 0 and rc_d == 0 and rc_d2 == 0
        for key in KEYS:
            assert torch.equal(dev[key], dev2[key]), (name, key)          # bit-reproducible from run to run
        got = {key: dev[key].cpu().numpy() for key in KEYS}
        d_ref = np.abs(got['refined'] - host['refined']).max()
        d_rt = np.abs(got['rt'] - host['rt']).max()
        d_dims = np.abs(got['dims'] - host['dims']).max()
        print('%-26s n=%3d J=%2d  |d refined| %.2e  |d rt| %.2e  |d dims| %.2e  statuses %s  iters <= %d'
              % (name, n, J, d_ref, d_rt, d_dims, sorted(set(got['status'].tolist())), got['iters'].max()))
        assert np.array_equal(got['status'], host['status']), name
        assert d_ref <= 1e-7 and d_rt <= 1e-9 and d_dims <= 1e-9, name
        assert np.isfinite(got['refined']).all() and np.isfinite(got['cost']).all()
        if name == 'shift_discarded':
            assert (got['status'] == 0).all()
            far = kw['root0']
            assert np.array_equal(got['refined'], np.concatenate([far[:, None], far[:, None] + kw['shape']], 1))
        elif name == 'behind_camera':
            assert got['status'][n // 2] == -1 and (np.delete(got['status'], n // 2) == 1).all()
        else:
            assert (got['status'] == 1).all(), name


def test_device_argument_rules(hip_lib):
    L = hip_lib
    before = L.egn_launch_count()
    assert L.egn_pnp_refine_f64(None, None, None, None, None, 0, 33, 5.0, None, None, None, None, None, None, None) == 0
    assert L.egn_launch_count() == before                                     # n = 0: no launch
    buf = torch.zeros(65 * 3, dtype=torch.float64, device='cuda')
    i32 = torch.zeros(1, dtype=torch.int32, device='cuda')
    p, q = _lib.ptr(buf), _lib.ptr(i32)
    for J in (1, 65):
        assert L.egn_pnp_refine_f64(p, p, p, None, None, 1, J, 5.0, p, p, p, q, q, p, None) == -1
    assert L.egn_pnp_refine_f64(p, p, p, None, None, -1, 33, 5.0, p, p, p, q, q, p, None) == -1
    assert L.egn_pnp_refine_f64(p, p, p, None, None, 1, 33, -1.0, p, p, p, q, q, p, None) == -1
    assert L.egn_pnp_refine_f64(p, p, p, None, None, 1, 33, 5.0, None, p, p, q, q, p, None) == -1
    assert L.egn_launch_count() == before
    case = pc.make(3, J=33, seed=5)
    rc, _ = dev_refine(case['shape'], case['k'], case['intr'])
    torch.cuda.synchronize()
    assert rc == 0 and L.egn_launch_count() == before + 1


def test_side_stream():
    case = pc.make(64, J=33, seed=77, noisy=True)
    kw = dict(shape=case['shape'], k=case['k'], intr=case['intr'], root0=case['root0'])
    rc, want = dev_refine(**kw)
    torch.cuda.synchronize()
    assert rc == 0
    side, busy = torch.cuda.Stream(), torch.cuda.Stream()
    a = torch.randn(2048, 2048, device='cuda')
    torch.cuda.synchronize()
    with torch.cuda.stream(busy):
        for _ in range(8):
            a = torch.tanh(a @ a * 1e-3)
    rc, got = dev_refine(stream=side, **kw)
    torch.cuda.synchronize()
    assert rc == 0
    for key in KEYS:
        assert torch.equal(got[key], want[key]), key


def _tiny_model():
    from egonet_amd import configs, synth
    from egonet_amd.model.egonet import EgoNet
    cfg = configs.hrnet_config(8, (64, 64), 33, 'coordinates', modules=(1, 1, 1), num_blocks=1, lifter_neurons=128)
    ego = EgoNet(cfg, pre_trained=False)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=6))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=7))
    ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    return ego.eval().cuda()


def test_infer_crops_refine(hip_lib, monkeypatch):
    from egonet_amd import synth
    from egonet_amd.common.img_proc import modify_bbox
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    L = hip_lib
    ego = _tiny_model()
    n = 5
    crops = synth.synth_crops(n, 3, 64, 64, seed=8).cuda()
    rets = [modify_bbox(b, 1.0) for b in synth.synth_boxes(n, seed=2)]
    centers, scales = np.stack([r['c'] for r in rets]), np.stack([r['s'] for r in rets])
    K = pc.KITTI_K
    ego.infer_crops(crops, centers, scales, K=K, to_host=False)              # first use: packing, plans
    torch.cuda.synchronize()
    c0 = L.egn_launch_count()
    plain = ego.infer_crops(crops, centers, scales, K=K, to_host=False)
    torch.cuda.synchronize()
    c1 = L.egn_launch_count()
    same = ego.infer_crops(crops, centers, scales, K=K, to_host=False, refine=None, roots=None, max_shift=5.0)
    torch.cuda.synchronize()
    c2 = L.egn_launch_count()
    ref = ego.infer_crops(crops, centers, scales, K=K, to_host=False, refine='pnp', alpha_mode='trans')
    torch.cuda.synchronize()
    c3 = L.egn_launch_count()
    assert c2 - c1 == c1 - c0 and c3 - c2 == c1 - c0 + 1
    assert set(same) == set(plain) and all(torch.equal(same[k], plain[k]) for k in plain)
    for k in ('local', 'kpts_2d', 'kpts_3d'):
        assert torch.equal(ref[k], plain[k])
    assert set(ref) == set(plain) | {'kpts_3d_refined', 'refine_status', 'dims'}

    k2d = plain['kpts_2d'].cpu().numpy().reshape(n, 33, 2)
    k3d = plain['kpts_3d'].cpu().numpy()
    intr = np.tile([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], (n, 1))
    rc, host = pc.host_refine(L, k3d, k2d, intr)
    assert rc == 0
    refined = ref['kpts_3d_refined'].cpu().numpy()
    status = ref['refine_status'].cpu().numpy()
    print('statuses', status.tolist(), ' |d refined| %.2e' % np.abs(refined - host['refined']).max())
    assert np.array_equal(status, host['status'])
    assert np.abs(refined - host['refined']).max() <= 1e-7
    assert np.abs(ref['dims'].cpu().numpy() - host['dims']).max() <= 1e-9
    assert torch.equal(ref['translation'], ref['kpts_3d_refined'][:, 0])
    rel = np.ascontiguousarray((refined[:, 1:] - refined[:, :1]).reshape(n, -1))
    euler, alpha = np.empty((n, 3)), np.empty(n)
    assert L.egn_pose_solve_host_f64(rel.ctypes.data, n, None, 1.0, 0.0, 1, euler.ctypes.data, alpha.ctypes.data) == 0
    got = ref['euler'].cpu().numpy()
    assert np.abs(np.cos(got) - np.cos(euler)).max() <= 1e-8 and np.abs(np.sin(got) - np.sin(euler)).max() <= 1e-8
    want_alpha = ego.get_observation_angle_trans(euler, refined[:, 0])
    d = ref['alpha'].cpu().numpy() - want_alpha
    assert np.abs((d + np.pi) % (2 * np.pi) - np.pi).max() <= 1e-8
    # EgoNet.refine_pnp on device tensors is the same launch
    again = ego.refine_pnp(plain['kpts_3d'], plain['kpts_2d'], torch.as_tensor(K).cuda())
    assert torch.equal(again['kpts_3d_refined'], ref['kpts_3d_refined']) and again['status'].is_cuda


def _label(cls, alpha, box, loc=(1.00, 1.50, 20.00), dims=(1.50, 1.60, 3.90), occ=0):
    return '%s 0.00 %d %.4f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.4f' % (
        (cls, occ, alpha) + box + dims + loc + (alpha + 0.05,))


def test_tool_refine_write_3d(tmp_path, monkeypatch):
    from PIL import Image
    import inference_kitti
    from egonet_amd.common import format as kfmt
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    img_dir, lab_dir, det_dir, out_dir = (tmp_path / n for n in ('image_2', 'label_2', 'det', 'out'))
    for d in (img_dir, lab_dir, det_dir):
        d.mkdir()
    rng = np.random.RandomState(0)
    boxes = {0: [(100.0, 150.0, 260.0, 250.0), (600.0, 160.0, 700.0, 230.0)], 1: [],
             2: [(900.0, 170.0, 1100.0, 300.0)]}
    locs = {0: [(-8.0, 1.6, 18.0), (1.5, 1.7, 30.0)], 2: [(9.0, 1.8, 14.0)]}
    for idx, bs in boxes.items():
        Image.fromarray(rng.randint(0, 256, (375, 1242, 3)).astype(np.uint8)).save(str(img_dir / ('%06d.png' % idx)))
        gt = [_label('Car', 0.3 * (j + 1), b, loc=locs[idx][j]) for j, b in enumerate(bs)]
        # frame 0: a 3-D detector's boxes (the fit starts at them); frame 2: a 2-D detector's (no 3-D fields)
        det = gt if idx == 0 else [_label('Car', -10.0, b, loc=(-1000.0,) * 3, dims=(-1.0,) * 3) for b in bs]
        (lab_dir / ('%06d.txt' % idx)).write_text('\n'.join(gt) + ('\n' if gt else ''))
        (det_dir / ('%06d.txt' % idx)).write_text('\n'.join(det) + ('\n' if det else ''))
    with pytest.raises(SystemExit):
        inference_kitti.main(['--images', str(img_dir), '--boxes', str(det_dir), '--out', str(out_dir), '--synthetic',
                              '--tiny', '--write-3d'])
    out = inference_kitti.main(['--images', str(img_dir), '--boxes', str(det_dir), '--out', str(out_dir),
                                '--synthetic', '--tiny', '--gt', str(lab_dir), '--frames-per-step', '2',
                                '--refine', 'pnp', '--refine-max-shift', '50', '--write-3d'])
    assert out['frames'] == 3 and out['instances'] == 3 and out['refine'] == 'pnp'
    assert sorted(os.listdir(str(out_dir / 'data'))) == ['000000.txt', '000001.txt', '000002.txt']
    assert (out_dir / 'data' / '000001.txt').read_text() == ''
    changed = 0
    for idx in (0, 2):
        got = [kfmt.parse_label_line(l) for l in (out_dir / 'data' / ('%06d.txt' % idx)).read_text().split('\n')]
        src = [kfmt.parse_label_line(l) for l in (det_dir / ('%06d.txt' % idx)).read_text().split('\n') if l.strip()]
        assert len(got) == len(src)
        for g, s in zip(got, src):
            assert g['class'] == 'Car' and g['bbox'] == s['bbox']
            assert -math.pi <= g['alpha'] <= math.pi and math.isfinite(g['rot_y'])
            if g['locations'] != s['locations']:            # status 1: the fit's own box
                changed += 1
                assert all(math.isfinite(v) for v in g['locations'] + g['dimensions'])
                assert g['locations'][2] > 0 and min(g['dimensions']) > 0
            else:
                assert g['dimensions'] == s['dimensions']
    print('refined 3-D boxes written: %d of 3' % changed)
    assert changed == out['refined_3d']
    ev = out['eval']['car']
    assert all(math.isfinite(v) for v in ev['AP']) and 'AP_bev' in ev and 'AP_3d' in ev
