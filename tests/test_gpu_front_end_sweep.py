"""csrc/crop.hip, csrc/targets.hip and csrc/geometry.hip at their edge shapes, through the C ABI, against the references
of tests/front_end_sweep.py (its docstring maps every gap to a test here).  Per launch:
  1. every output sits NaN-filled between two guard bands (sweep_guards), with NaN slack floats next to it where the
     output's alignment is chosen; bands and slack are checked, so is every element (no sampling);
  2. crops: the same bits as the oracle's warp + float32 normalisation, and as the other entry point;
  3. targets: the float64 reference's support and weights exactly, |v - v64| <= C_TARGET 2^-24 (1 + |arg|) v64;
  4. geometry: the oracle at the project's 1e-9 (1e-6 for the float32 lifter input, one float64 rounding for the
     un-normalisation), the host twins at 1e-12 (pose) and 1e-11 (screen);
  5. each test prints its worst measured figure."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import front_end_sweep as FE
from conftest import golden
from egonet_amd import _lib, configs
from oracle import geometry_oracle
from sweep_guards import _guarded, _guards_intact

pytestmark = pytest.mark.gpu
NAN = float('nan')


def _st():
    return _lib.current_stream()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _out(numel, dtype=torch.float32, off=0):
    """(whole, slack, body): numel NaN elements `off` elements past a 16-byte boundary, NaN slack around them, a guard
    band on each side."""
    whole, slack = _guarded(numel + 4, dtype, NAN)
    body = slack[off:off + numel]
    assert slack.data_ptr() % 16 == 0
    return whole, slack, body


def _clean(whole, slack, off, numel):
    """Nothing written outside the body."""
    return _guards_intact(whole) and bool(torch.isnan(slack[:off]).all()) and bool(torch.isnan(slack[off + numel:]).all())


# ---------------------------------------------------------------------------------------------------------------
# crops
# ---------------------------------------------------------------------------------------------------------------
def _norm_dev(norm):
    return torch.tensor(norm[0], dtype=torch.float32, device='cuda'), torch.tensor(norm[1], dtype=torch.float32, device='cuda')


def _crop_multi(frames, box_frame, Ms, out_wh, norm=FE.IMAGENET, out_off=0, n_frames=None):
    """One launch of the multi-frame entry over frames packed with odd base offsets and padded rows."""
    w, h = out_wh
    blob, tab = FE.pack_frames(frames)
    data, tab_d = _dev(blob), _dev(tab)
    bf = _dev(np.asarray(box_frame), np.int32)
    M_d = _dev(np.asarray(Ms).reshape(-1, 6), np.float64)
    n = M_d.shape[0]
    mean_t, std_t = _norm_dev(norm)
    whole, slack, body = _out(n * 3 * h * w, off=out_off)
    keep = data.clone()
    rc = _lib.lib().egn_crop_frames_warp_normalize_u8(
        _lib.ptr(data), _lib.ptr(tab_d), len(frames) if n_frames is None else n_frames, _lib.ptr(bf), _lib.ptr(M_d), n, h, w,
        _lib.ptr(mean_t), _lib.ptr(std_t), _lib.ptr(body), _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert _clean(whole, slack, out_off, n * 3 * h * w), 'write outside the crops'
    assert torch.equal(data, keep)
    return body.cpu().numpy().reshape(n, 3, h, w)


def _crop_one(img, Ms, out_wh, norm=FE.IMAGENET, pad=0, base=0, out_off=0):
    """One launch of the one-frame entry; the frame starts `base` bytes into its allocation, rows of 3 W + pad bytes."""
    w, h = out_wh
    H, W = img.shape[:2]
    blob, tab = FE.pack_frames([img], lead=base, pad=lambda i: pad)
    data = _dev(blob)
    M_d = _dev(np.asarray(Ms).reshape(-1, 6), np.float64)
    n = M_d.shape[0]
    mean_t, std_t = _norm_dev(norm)
    whole, slack, body = _out(n * 3 * h * w, off=out_off)
    rc = _lib.lib().egn_crop_warp_normalize_u8(
        C.c_void_p(data.data_ptr() + int(tab[0, 0])), H, W, int(tab[0, 3]), _lib.ptr(M_d), n, h, w, _lib.ptr(mean_t),
        _lib.ptr(std_t), _lib.ptr(body), _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert _clean(whole, slack, out_off, n * 3 * h * w), 'write outside the crops'
    return body.cpu().numpy().reshape(n, 3, h, w)


def _differ(got, want, names=None):
    """Per crop, the number of elements whose bits differ -> (total, text)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    bad = (got.view(np.uint32) != want.view(np.uint32)).reshape(len(got), -1).sum(axis=1)
    txt = ', '.join('%s: %d' % (names[i] if names else i, b) for i, b in enumerate(bad) if b)
    return int(bad.sum()), txt


@pytest.fixture(scope='module')
def wrap_ref():
    t = time.time()
    Ms = FE.wrap_matrices()
    FE.assert_range(Ms, FE.WRAP_WH)
    img = FE.frame()
    ref = FE.ref_crops([img], [0] * len(Ms), Ms, FE.WRAP_WH)
    print('\nthe oracle over %d crops of %dx%d: %.1f s' % (len(Ms), FE.WRAP_WH[0], FE.WRAP_WH[1], time.time() - t))
    return img, Ms, ref


def test_crop_wrap_one_frame_entry_and_multi_frame(wrap_ref):
    """n * out_h * out_w = 2 150 400 > 8192 * 256: the one-frame entry's stride loop takes a second trip."""
    img, Ms, ref = wrap_ref
    one = _crop_one(img, Ms, FE.WRAP_WH)
    multi = _crop_multi([img], [0] * len(Ms), Ms, FE.WRAP_WH)
    d1, t1 = _differ(one, ref)
    d2, t2 = _differ(multi, ref)
    d3, _ = _differ(one, multi)
    print('\nwrap: %d elements; differing from the oracle: one-frame %d, multi-frame %d; between the entries %d'
          % (ref.size, d1, d2, d3))
    assert d1 == 0 and d2 == 0 and d3 == 0, (t1[:400], t2[:400])


def test_crop_one_frame_padded_rows_odd_base(wrap_ref):
    img, Ms, ref = wrap_ref
    sel = np.r_[0:40, 1000:1040]
    got = _crop_one(img, Ms[sel], FE.WRAP_WH, pad=5, base=7)
    d, t = _differ(got, ref[sel])
    wh = (36, 21)
    ms = [M for _, f, M in FE.matrix_set(wh) if f == 0]
    got2 = _crop_one(img, ms, wh, pad=5, base=13)
    d2, t2 = _differ(got2, FE.ref_crops([img], [0] * len(ms), ms, wh))
    print('\npitch 3 W + 5, odd base: %d + %d elements differ' % (d, d2))
    assert d == 0 and d2 == 0, (t, t2)


@pytest.mark.parametrize('wh', FE.OUT_SIZES, ids=['%dx%d' % s for s in FE.OUT_SIZES])
def test_crop_multi_frame_output_sizes(wh):
    """A single ragged quad (out_w < 4), a quad and a ragged one (5), two quads (8); the row-tail block of 16 rows alone
    (1, 15), none (16), next to full ones (17, 33)."""
    frames = [FE.frame(), FE.frame((37, 53), seed=2)]
    Ms = FE.size_matrices(wh)
    FE.assert_range(Ms, wh)
    box_frame = [0] * len(Ms) + [1] * len(Ms)
    Ms2 = np.concatenate([Ms, Ms])
    ref = FE.ref_crops(frames, box_frame, Ms2, wh)
    got = _crop_multi(frames, box_frame, Ms2, wh)
    one = _crop_one(frames[0], Ms, wh)
    d, t = _differ(got, ref)
    d1, t1 = _differ(one, ref[:len(Ms)])
    print('\n%dx%d: %d elements, %d (multi-frame) and %d (one-frame) differ' % (wh[0], wh[1], ref.size, d, d1))
    assert len({tuple(r.ravel()) for r in ref}) > len(Ms), 'the crops are not distinct'
    assert d == 0 and d1 == 0, (t, t1)


def test_crop_multi_frame_unaligned_out_takes_scalar_stores():
    """out_w % 4 == 0 with `out` one, two, three floats past a 16-byte boundary: vec = 0 for the pointer alone."""
    wh = (8, 17)
    frames = [FE.frame()]
    Ms = FE.size_matrices(wh)
    ref = FE.ref_crops(frames, [0] * len(Ms), Ms, wh)
    aligned = _crop_multi(frames, [0] * len(Ms), Ms, wh)
    assert _differ(aligned, ref)[0] == 0
    for off in (1, 2, 3):
        got = _crop_multi(frames, [0] * len(Ms), Ms, wh, out_off=off)
        d, t = _differ(got, aligned)
        print('out %d floats past the boundary: %d elements differ from the aligned run' % (off, d))
        assert d == 0, t


def test_crop_box_frame_outside_the_table_reads_nothing():
    """box_frame of -1, n_frames and beyond: the normalised level 0 everywhere; the boxes next to them as without."""
    wh = (12, 17)
    frames = [FE.frame(), FE.frame((37, 53), seed=2)]
    Ms = FE.size_matrices(wh)
    box_frame = [-1, 0, 2, 1, 7, -2 ** 31]
    ref = FE.ref_crops(frames, box_frame, Ms, wh)
    lvl0 = FE.normalise(np.zeros((wh[1], wh[0], 3), np.uint8), *FE.IMAGENET)
    for i in (0, 2, 4, 5):
        assert np.array_equal(ref[i], lvl0)
    got = _crop_multi(frames, box_frame, Ms, wh)
    d, t = _differ(got, ref)
    print('\nbox_frame %s: %d elements differ' % (box_frame, d))
    assert d == 0, t


@pytest.mark.parametrize('norm', [FE.IMAGENET, FE.OTHER_NORM], ids=['imagenet', 'other'])
def test_crop_matrix_set_both_entries(norm):
    wh = (36, 21)
    frames = [FE.frame(), np.array(FE.PIXEL_1X1, dtype=np.uint8).reshape(1, 1, 3)]
    cases = FE.matrix_set(wh)
    names, box_frame, Ms = [c[0] for c in cases], [c[1] for c in cases], np.stack([c[2] for c in cases])
    FE.assert_range(Ms, wh)
    ref = FE.ref_crops(frames, box_frame, Ms, wh, norm)
    multi = _crop_multi(frames, box_frame, Ms, wh, norm)
    one = np.full_like(ref, np.nan)
    for f in (0, 1):
        idx = [i for i, b in enumerate(box_frame) if b == f]
        one[idx] = _crop_one(frames[f], Ms[idx], wh, norm, pad=3 * f, base=f)
    d, t = _differ(multi, ref, names)
    d1, t1 = _differ(one, ref, names)
    print('\n%d matrices, %d elements: %d (multi-frame) and %d (one-frame) differ from the oracle' % (len(Ms), ref.size, d, d1))
    assert d == 0 and d1 == 0, (t, t1)


# ---------------------------------------------------------------------------------------------------------------
# targets
# ---------------------------------------------------------------------------------------------------------------
_TARGET_CASES = {}


def _target_case(name):
    if not _TARGET_CASES:
        _TARGET_CASES.update({c['name']: c for c in FE.target_cases()})
    return _TARGET_CASES[name]


@pytest.mark.parametrize('name', FE.TARGET_CASE_NAMES)
def test_targets_edge_cases(name):
    c = _target_case(name)
    N, K = c['joints'].shape[:2]
    H, W = c['H'], c['W']
    j_d = _dev(c['joints'], np.float64)
    v_d = None if c['vis'] is None else _dev(c['vis'], np.float32)
    wt, st, tgt = _out(N * K * H * W)
    ww, sw, wgt = _out(N * K)
    keep_j = j_d.clone()
    rc = _lib.lib().egn_gaussian_targets_f32(_lib.ptr(j_d), _lib.ptr(v_d), N, K, H, W, c['stride_x'], c['stride_y'], c['sigma'],
                                             _lib.ptr(tgt), None if c['weight_null'] else _lib.ptr(wgt), _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert _clean(wt, st, 0, N * K * H * W) and _clean(ww, sw, 0, N * K), 'write outside the outputs'
    assert torch.equal(j_d, keep_j)
    if c['weight_null']:
        assert bool(torch.isnan(wgt).all())
    got_w = None if c['weight_null'] else wgt.cpu().numpy()
    ratio, fails = FE.check_targets(c, tgt.cpu().numpy().reshape(N, K, H, W), got_w)
    print('\n%-13s %d x %d maps of %d x %d, sigma %g: worst ratio %.3f (C %g)' % (name, N, K, H, W, c['sigma'], ratio, FE.C_TARGET))
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(len(FE.SCREEN_CASES)),
                         ids=['%dx%d_%dx%d_%s' % (c[0], c[1], c[2], c[3], 'nolift' if c[6] is None else 'ld+%d' % c[6])
                              for c in FE.SCREEN_CASES])
def test_keypoints_to_screen(case):
    n, K, cw, ch, mx, my, lift = FE.SCREEN_CASES[case]
    local, c, s, mean_in, std_in, want = FE.screen_case(n, K, cw, ch, mx, my, seed=case)
    L = _lib.lib()
    ws, ss, scr = _out(n * 2 * K, torch.float64)
    ld = 0 if lift is None else 2 * K + lift
    wl, sl, lin = _out(max(1, n * ld))
    l_d, c_d, s_d, m_d, d_d = _dev(local), _dev(c), _dev(s), _dev(mean_in), _dev(std_in)
    rc = L.egn_keypoints_to_screen_f64(_lib.ptr(l_d), n, K, mx, my, _lib.ptr(c_d), _lib.ptr(s_d), cw, ch, _lib.ptr(scr),
                                       None if lift is None else _lib.ptr(m_d), None if lift is None else _lib.ptr(d_d),
                                       None if lift is None else _lib.ptr(lin), ld, _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert _clean(ws, ss, 0, n * 2 * K) and _guards_intact(wl), 'write outside the outputs'
    got = scr.cpu().numpy().reshape(n, 2 * K)
    assert not np.isnan(got).any()                                   # screen is written with and without lifter_in
    worst = np.abs(got - want).max()
    assert worst <= 1e-9
    worst_in = 0.0
    if lift is None:
        assert bool(torch.isnan(sl).all())
    else:
        got_in = lin.cpu().numpy().reshape(n, ld)
        assert bool(torch.isnan(sl[n * ld:]).all()) and np.isnan(got_in[:, 2 * K:]).all(), 'a pad column was written'
        want_in = ((want - mean_in) / std_in).astype(np.float32)
        worst_in = np.abs(got_in[:, :2 * K] - want_in).max()
        assert worst_in <= 1e-6
    host = np.full((n, 2 * K), np.nan)
    assert L.egn_keypoints_to_screen_host_f64(local.ctypes.data, n, K, mx, my, c.ctypes.data, s.ctypes.data, cw, ch,
                                              host.ctypes.data) == 0
    twin = np.abs(got - host).max()
    print('\nn K = %d: |screen - oracle| %.2e, |lifter_in - oracle| %.2e, |device - host twin| %.2e' % (n * K, worst, worst_in, twin))
    # the same few float64 operations on |X| < 2^13 px; a fused multiply-add may round 4 of them differently: 4 ulp
    assert twin <= 1e-11


@pytest.mark.parametrize('n,D,extra', FE.UNNORM_CASES)
def test_unnormalize(n, D, extra):
    rng = np.random.RandomState(n * 131 + D)
    ld = D + extra
    y = np.full((n, ld), np.nan, dtype=np.float32)                   # the kernel must not look at the pad columns
    y[:, :D] = rng.normal(0, 1.5, (n, D)).astype(np.float32)
    mean, std = rng.normal(0, 20, D), rng.uniform(0.01, 5, D)
    w, s, out = _out(n * D, torch.float64)
    y_d, m_d, s_d = _dev(y), _dev(mean), _dev(std)
    rc = _lib.lib().egn_unnormalize_f64(_lib.ptr(y_d), n, D, ld, _lib.ptr(m_d), _lib.ptr(s_d), _lib.ptr(out), _st())
    torch.cuda.synchronize()
    assert rc == 0 and _clean(w, s, 0, n * D)
    got = out.cpu().numpy().reshape(n, D)
    y64 = y[:, :D].astype(np.float64)
    want = y64 * std + mean
    slack = 2.0 ** -53 * (np.abs(y64 * std) + np.abs(mean))
    assert not np.isnan(got).any()
    ratio = (np.abs(got - want) / slack).max()
    print('\nn D ld = %d %d %d: worst |got - want| / slack = %.3f, %d of %d elements differ' % (n, D, ld, ratio, (got != want).sum(), got.size))
    assert ratio <= 1.0


def test_unnormalize_empty_and_refusals():
    L = _lib.lib()
    assert L.egn_unnormalize_f64(None, 0, 96, 96, None, None, None, _st()) == 0          # n == 0: no launch
    w, s, out = _out(96 * 4, torch.float64)
    y = torch.randn(4, 96, device='cuda')
    m = torch.zeros(96, dtype=torch.float64, device='cuda')
    for n, D, ld in ((4, 96, 95), (4, 0, 96), (4, -1, 96), (-1, 96, 96)):
        assert L.egn_unnormalize_f64(_lib.ptr(y), n, D, ld, _lib.ptr(m), _lib.ptr(m), _lib.ptr(out), _st()) == -1, (n, D, ld)
    torch.cuda.synchronize()
    assert bool(torch.isnan(s).all()) and _guards_intact(w)


def _pose_dev(P, kx, mode, K=FE.POSE_K):
    n = len(P)
    p_d = _dev(P.reshape(n, -1), np.float64)
    k_d = None if kx is None else _dev(kx, np.float64)
    we, se, eu = _out(3 * n, torch.float64)
    wa, sa, al = _out(n, torch.float64)
    rc = _lib.lib().egn_pose_solve_f64(_lib.ptr(p_d), n, _lib.ptr(k_d), float(K[0, 0]), float(K[0, 2]), mode, _lib.ptr(eu),
                                       _lib.ptr(al), _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert _clean(we, se, 0, 3 * n) and _clean(wa, sa, 0, n), 'write outside euler / alpha'
    return eu.cpu().numpy().reshape(n, 3), al.cpu().numpy()


def _pose_host(P, kx, mode, K=FE.POSE_K):
    n = len(P)
    p = np.ascontiguousarray(P.reshape(n, -1), dtype=np.float64)
    kx = np.ascontiguousarray(kx, dtype=np.float64)
    e, a = np.full((n, 3), np.nan), np.full(n, np.nan)
    assert _lib.lib().egn_pose_solve_host_f64(p.ctypes.data, n, kx.ctypes.data, float(K[0, 0]), float(K[0, 2]), mode,
                                              e.ctypes.data, a.ctypes.data) == 0
    return e, a


@pytest.mark.parametrize('name', FE.POSE_FAMILIES)
def test_pose_solve_families(name):
    """n = 1, 63, 64, 65 (one wave per block), both alpha modes."""
    import warnings
    P, kx = FE.pose_family(name), FE.pose_kpt_x(name)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                  # scipy announces the gimbal lock it resolves like the solve does
        ref_e, ref_proj, ref_trans, ref_R = FE.pose_reference(P, kx)
    worst, twin, fails = 0.0, 0.0, []
    for n in (1, 63, 64, 65):
        for mode, ref_a in ((0, ref_proj), (1, ref_trans)):
            e, a = _pose_dev(P[:n], kx[:n], mode)
            assert not np.isnan(e).any() and not np.isnan(a).any()
            w, f = FE.check_pose(name, e, a, ref_e[:n], ref_a[:n], ref_R[:n])
            worst = max(worst, w)
            fails += ['n %d mode %d: %s' % (n, mode, m) for m in f]
            he, ha = _pose_host(P[:n], kx[:n], mode)
            twin = max(twin, float(FE.ang_diff(e, he).max()), float(FE.ang_diff(a, ha).max()))
    print('\n%-8s worst difference from the oracle %.3g, from the host twin %.3g' % (name, worst, twin))
    assert not fails, fails
    assert twin <= 1e-12


def test_pose_alpha_next_to_pi():
    """kpt_x chosen so that alpha lands 5e-10 on either side of +pi and of -pi before the two `while` wraps."""
    P = FE.pose_family('wide')
    ref_e, _, _, _ = FE.pose_reference(P, FE.pose_kpt_x('wide'))
    rows = [(i, d, FE.near_pi_kpt_x(ref_e[i, 1], d)) for i in range(len(P)) for d in (5e-10, -5e-10)]
    rows = [r for r in rows if r[2] is not None]
    idx, kx = np.array([r[0] for r in rows]), np.array([r[2] for r in rows])
    want = geometry_oracle.observation_angle_proj(ref_e[idx], kx, FE.POSE_K)
    assert len(rows) >= 16 and (np.abs(np.abs(want) - np.pi) < 1e-9).all() and (want > 0).any() and (want < 0).any()
    e, a = _pose_dev(P[idx], kx, 0)
    he, ha = _pose_host(P[idx], kx, 0)
    d, twin = float(FE.ang_diff(a, want).max()), float(FE.ang_diff(a, ha).max())
    print('\n%d alphas within 1e-9 of +-pi: worst difference from the oracle %.3g, from the host twin %.3g' % (len(rows), d, twin))
    assert d <= 1e-9 and twin <= 1e-12 and (np.abs(a) <= np.pi).all()


def test_pose_rank_deficient_instance_is_alone():
    """All 32 points equal: the template is a point, H = 0, and NaN comes back in the pitch, the yaw and alpha (the
    third angle is the gimbal branch's 0); the instances around it, in the same wave and the next, keep their bits."""
    P, kx = FE.pose_family('wide').copy(), FE.pose_kpt_x('wide')
    e0, a0 = _pose_dev(P, kx, 0)
    bad = [0, 31, 64]
    for i in bad:
        P[i] = P[i, 0]
    for mode in (0, 1):
        e, a = _pose_dev(P, kx, mode)
        assert np.isnan(e[bad, :2]).all() and np.isnan(a[bad]).all()
        he, ha = _pose_host(P, kx, mode)
        assert np.isnan(he[bad, :2]).all() and np.isnan(ha[bad]).all()
        good = np.setdiff1d(np.arange(len(P)), bad)
        assert np.array_equal(e[good], e0[good])
        if mode == 0:
            assert np.array_equal(a[good], a0[good])
        assert not np.isnan(a[good]).any()


# ---------------------------------------------------------------------------------------------------------------
# EgoNet.get_keypoints on the device with rotated records
# ---------------------------------------------------------------------------------------------------------------
def test_get_keypoints_with_rotated_records_on_the_device():
    """The GPU twin of tests/test_egonet_cpu.py::test_get_keypoints_with_rotated_records_vs_reference: the rot = 0 rows
    come from the device kernel, the others from the host override (libs/model/egonet.py:442-452)."""
    from egonet_amd.model.egonet import EgoNet
    g = golden('kpts_rotated.npz')
    ego = EgoNet(configs.tiny_config('coordinates'), pre_trained=False).eval()
    ego.resolution = [int(v) for v in g['resolution']]
    local = torch.from_numpy(g['local']).cuda()
    n = local.shape[0]

    class _Stub(torch.nn.Module):
        def forward(self, x):
            assert x.is_cuda
            return None, local
    ego.HC = _Stub()
    records = [dict(path='img%d.png' % (i // 4), center=g['centers'][i], scale=g['scales'][i], rotation=float(g['rots'][i]),
                    bbox_resize=[0, 0, 1, 1], label='Car', score=1.0) for i in range(n)]
    assert 0.0 in [r['rotation'] for r in records] and any(r['rotation'] != 0 for r in records)
    rec = ego.get_keypoints(torch.zeros(n, 3, 8, 8), records, is_cuda=True)
    got = np.concatenate([np.concatenate(rec[p]['kpts_2d_pred']) for p in rec]).reshape(n, -1, 2)
    worst = np.abs(got - g['screen']).max(axis=(1, 2))
    print('\nrotations %s: worst |screen - reference| per record %s' % (list(g['rots']), ['%.1e' % w for w in worst]))
    np.testing.assert_allclose(got, g['screen'], rtol=0, atol=1e-6)
    assert [r for p in rec for r in rec[p]['rotation']] == [float(v) for v in g['rots']]
