"""KITTI bird's-eye-view and 3D AP on the host path (csrc/kitti_eval.cpp over csrc/kitti_overlap_math.h, no GPU):
the overlap routine against closed forms and against scipy's half-plane intersection, the whole evaluator against the
independent restatement tests/kitti_eval3d_ref.py, hand-computed cases, and the image part against evaluate_aos.
The reference's own evaluator needs Boost and cannot be built here: parity with its binary is unpinned."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import kitti_eval3d_ref as ref
from egonet_amd import _lib, evaluate

BOUND = 1e-9        # the project's bound for float64 geometry (tests/golden/pose_solve.npz)


def box(h=1.5, w=1.6, l=3.9, t1=1.0, t2=1.5, t3=20.0, ry=0.0, x1=100.0, y1=100.0, x2=200.0, y2=180.0, alpha=0.0):
    return dict(x1=x1, y1=y1, x2=x2, y2=y2, alpha=alpha, h=h, w=w, l=l, t1=t1, t2=t2, t3=t3, ry=ry)


def host_overlaps(dets, gts, criterion=-1):
    """[n][4]: image, ground, 3D overlap and bird's-eye-view intersection through the host ABI entry."""
    d = np.array([ref.box12(b) for b in dets], dtype=np.float64).reshape(-1, 12)
    g = np.array([ref.box12(b) for b in gts], dtype=np.float64).reshape(-1, 12)
    out = np.full((len(d), 4), np.nan)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    assert _lib.lib().egn_kitti_overlap_host_f64(vp(d), vp(g), len(d), criterion, vp(out)) == 0
    return out


def one(d, g, criterion=-1):
    return host_overlaps([d], [g], criterion)[0]


DONTCARE = box(h=-1, w=-1, l=-1, t1=-1000, t2=-1000, t3=-1000, ry=-10, alpha=-10, x1=700, y1=100, x2=900, y2=250)


def jittered_pairs(seed, n):
    """Pairs as the evaluator meets them: a car-sized box and a copy moved by up to a box length, turned and resized."""
    rng = np.random.RandomState(seed)
    dets, gts = [], []
    for _ in range(n):
        g = box(h=rng.uniform(1.2, 2.0), w=rng.uniform(0.5, 2.2), l=rng.uniform(0.8, 5.0), t1=rng.uniform(-30, 30),
                t2=rng.uniform(1.0, 2.0), t3=rng.uniform(3, 70), ry=rng.uniform(-3.2, 3.2))
        s = rng.choice([0.05, 0.5, 2.0])
        d = box(h=g['h'] * rng.uniform(0.8, 1.2), w=g['w'] * rng.uniform(0.8, 1.2), l=g['l'] * rng.uniform(0.8, 1.2),
                t1=g['t1'] + rng.normal(0, s), t2=g['t2'] + rng.normal(0, 0.2), t3=g['t3'] + rng.normal(0, s),
                ry=g['ry'] + rng.choice([0.0, math.pi / 2, math.pi]) + rng.normal(0, 0.3))
        dets.append(d)
        gts.append(g)
    return dets, gts


def test_identical_boxes_overlap_exactly_one():
    for b in (box(), box(ry=0.7, t1=-13.25, t3=41.5), box(h=1.75, w=0.5, l=0.75, ry=-2.9, t2=1.75)):
        o = one(b, dict(b))
        assert o[1] == 1.0 and o[2] == 1.0 and o[0] == 1.0, o
        assert o[3] == b['l'] * b['w']


@pytest.mark.parametrize('dx,dz', [(1.0, 0.0), (0.0, 0.4), (2.5, 1.0), (-3.0, -0.6)])
def test_axis_aligned_offsets_equal_the_rectangle_formula(dx, dz):
    g, d = box(), box(t1=1.0 + dx, t3=20.0 + dz)
    inter = max(0.0, 3.9 - abs(dx)) * max(0.0, 1.6 - abs(dz))
    o = one(d, g)
    assert abs(o[3] - inter) < BOUND
    assert abs(o[1] - inter / (2 * 3.9 * 1.6 - inter)) < BOUND
    assert abs(o[2] - inter * 1.5 / (2 * 3.9 * 1.6 * 1.5 - inter * 1.5)) < BOUND


def test_rotated_closed_forms():
    sq = box(l=1.0, w=1.0)
    o = one(box(l=1.0, w=1.0, ry=math.pi / 4), sq)
    assert abs(o[3] - 2 * (math.sqrt(2) - 1)) < BOUND             # the regular octagon
    o = one(box(ry=math.pi / 2), box())
    assert abs(o[3] - 1.6 ** 2) < BOUND
    assert abs(o[1] - 1.6 ** 2 / (2 * 3.9 * 1.6 - 1.6 ** 2)) < BOUND and abs(o[1] - 0.25806451612903225) < BOUND
    # either corner orientation: negative extents describe the same rectangle
    o2 = one(box(l=-3.9, w=-1.6, ry=math.pi / 2), box())
    assert abs(o2[3] - 1.6 ** 2) < BOUND


def test_disjoint_touching_contained():
    g = box()
    assert one(box(t1=30.0), g)[1:].tolist() == [0.0, 0.0, 0.0]                     # disjoint
    o = one(box(t1=1.0 + 3.9), g)                                                   # sharing an edge
    assert o[3] == 0.0 and o[1] == 0.0 and o[2] == 0.0
    small = box(l=1.0, w=0.5, ry=0.3, t1=1.2, t3=20.1)
    o = one(small, g)
    assert abs(o[3] - 0.5) < BOUND and abs(o[1] - 0.5 / (3.9 * 1.6)) < BOUND         # contained: ratio of the areas


def test_height_only_difference():
    g = box()
    for dy in (0.0, 0.5, -0.25, 1.5, 4.0):
        o = one(box(t2=1.5 + dy), g)
        hov = max(0.0, 1.5 - abs(dy))
        assert abs(o[1] - 1.0) < BOUND
        assert abs(o[2] - hov / (3.0 - hov)) < BOUND


def test_criteria_divide_by_the_detection_or_the_ground_truth():
    d, g = box(h=1.2, t1=2.0, t3=20.3, x1=120, y1=110, x2=220, y2=200), box()
    inter = (3.9 - 1.0) * (1.6 - 0.3)
    ymin, ymax = max(1.5 - 1.2, 0.0), 1.5
    vol = inter * (ymax - ymin)
    o0, o1 = one(d, g, 0), one(d, g, 1)
    assert abs(o0[1] - inter / (3.9 * 1.6)) < BOUND and abs(o1[1] - inter / (3.9 * 1.6)) < BOUND
    assert abs(o0[2] - vol / (1.2 * 3.9 * 1.6)) < BOUND and abs(o1[2] - vol / (1.5 * 3.9 * 1.6)) < BOUND
    img = 80.0 * 70.0
    assert abs(o0[0] - img / (100 * 90.0)) < BOUND and abs(o1[0] - img / (100 * 80.0)) < BOUND


def test_dontcare_row_against_real_detections_is_zero():
    dets, _ = jittered_pairs(5, 20)
    for crit in (-1, 0):
        o = host_overlaps(dets, [DONTCARE] * len(dets), crit)
        assert not o[:, 1:].any() and np.isfinite(o).all()


@functools.lru_cache(maxsize=None)
def scipy_overlaps(seed=11, n=480):
    """(detections, ground truths, [n][3] ground overlap, 3D overlap, intersection by scipy), computed once."""
    dets, gts = jittered_pairs(seed, n)
    want = np.array([[ref.ground_overlap(d, g), ref.box3d_overlap(d, g), ref.bev_intersection(d, g)]
                     for d, g in zip(dets, gts)])
    want.setflags(write=False)
    return dets, gts, want


def test_overlaps_against_half_plane_intersection():
    """480 seeded pairs of jittered boxes against scipy (HalfspaceIntersection around a linprog Chebyshev centre,
    ConvexHull.volume), bound 1e-9 absolute.  Measured on the host path: max |intersection - scipy| = 4.4e-14,
    max |ground overlap - scipy| = 1.7e-14, max |3D overlap - scipy| = 1.6e-14; symmetry in the two boxes 3.6e-15;
    a common rotation and translation of both boxes 3.5e-14."""
    dets, gts, want = scipy_overlaps()
    got = host_overlaps(dets, gts)
    assert (want[:, 2] > 0.05).sum() > 150 and (want[:, 2] == 0).sum() > 20        # both kinds of pair are there
    err = np.abs(got[:, 1:] - want).max(axis=0)
    print('host - scipy: ground %.3g, 3D %.3g, intersection %.3g' % tuple(err))
    assert err.max() < BOUND
    swapped = host_overlaps(gts, dets)
    sym = np.abs(swapped[:, 1:] - got[:, 1:]).max()
    rng = np.random.RandomState(3)
    moved_d, moved_g = [], []
    for d, g in zip(dets, gts):
        th, sx, sz = rng.uniform(-3, 3), rng.uniform(-40, 40), rng.uniform(-40, 40)
        c, s = math.cos(th), math.sin(th)

        def move(b):
            # toPolygon turns by -ry: turning the scene by th about the origin adds -th to ry
            return dict(b, t1=c * b['t1'] - s * b['t3'] + sx, t3=s * b['t1'] + c * b['t3'] + sz, ry=b['ry'] - th)
        moved_d.append(move(d))
        moved_g.append(move(g))
    rigid = np.abs(host_overlaps(moved_d, moved_g)[:, 1:] - got[:, 1:]).max()
    print('symmetry %.3g, rigid motion %.3g' % (sym, rigid))
    assert sym < BOUND and rigid < BOUND


SEEDS = (0, 1, 2)


def _frames_as_arrays(frames):
    keys = sorted(frames)
    return [ref.to_arrays(frames[k][0], False) for k in keys], [ref.to_arrays(frames[k][1], True) for k in keys]


@pytest.mark.parametrize('seed', SEEDS)
def test_evaluator_equals_python_restatement(seed):
    frames, parsed, tables, want = ref.reference(seed)
    # no overlap of any pair, in any metric, within 1e-6 of a class threshold: a last-place difference between the
    # clip and scipy cannot change a match
    n_pairs = 0
    for tab in tables:
        for metric in ref.METRICS:
            for row in tab[metric]:
                for o in row:
                    assert abs(o - 0.5) > 1e-6 and abs(o - 0.7) > 1e-6, (metric, o)
                    n_pairs += 1
    assert n_pairs > 300
    gt_frames, det_frames = _frames_as_arrays(frames)
    got = evaluate.evaluate_frames(gt_frames, det_frames, device='cpu')
    assert got['n_frames'] == len(frames)
    assert set(k for k in got if k in evaluate.CLASSES) == set(want)
    key = {'image': 'precision', 'ground': 'precision_ground', '3d': 'precision_3d'}
    for name, per_metric in want.items():
        assert set(m for m in ref.METRICS if key[m] in got[name]) == set(per_metric)
        for metric, (prec, counts) in per_metric.items():
            np.testing.assert_array_equal(got[name][key[metric]], np.array(prec))     # same doubles, NaN == NaN
            for lv in range(3):
                n = int(got[name]['n_thresholds'][metric][lv])
                assert n == len(counts[lv])
                np.testing.assert_array_equal(got[name]['counts'][metric][lv][:n], np.array(counts[lv]).reshape(n, 3))
    assert np.count_nonzero(got['car']['precision_ground'][2]) >= 3                  # real curves, not trivial ones
    assert np.count_nonzero(got['car']['precision_3d'][2]) >= 2


def _write(tmp, frames):
    gt_dir, res_dir = tmp / 'label_2', tmp / 'result'
    (res_dir / 'data').mkdir(parents=True)
    gt_dir.mkdir()
    for idx, (gts, dets) in frames.items():
        (gt_dir / ('%06d.txt' % idx)).write_text('\n'.join(gts) + ('\n' if gts else ''))
        (res_dir / 'data' / ('%06d.txt' % idx)).write_text('\n'.join(dets) + ('\n' if dets else ''))
    return str(gt_dir), str(res_dir)


def test_directories_and_arrays_agree_and_the_image_part_equals_evaluate_aos(tmp_path):
    frames = ref.reference(0)[0]
    gt_dir, res_dir = _write(tmp_path, frames)
    got = evaluate.evaluate_kitti(gt_dir, res_dir, device='cpu')
    old = evaluate.evaluate_aos(gt_dir, res_dir)
    assert got['n_frames'] == old['n_frames'] and got['aos_valid'] == old['aos_valid'] is True
    assert set(old) <= set(got)
    for name in evaluate.CLASSES:
        if name in old:
            np.testing.assert_array_equal(got[name]['precision'], old[name]['precision'])
            np.testing.assert_array_equal(got[name]['aos'], old[name]['aos'])
            assert got[name]['AP'] == old[name]['AP'] and got[name]['AOS'] == old[name]['AOS']
    arrays = evaluate.evaluate_frames(*_frames_as_arrays(frames), device='cpu')
    for name in evaluate.CLASSES:
        if name in got:
            for k in ('precision', 'aos', 'precision_ground', 'precision_3d'):
                np.testing.assert_array_equal(arrays[name][k], got[name][k])
    only = evaluate.evaluate_kitti(gt_dir, res_dir, metrics=('3d',), device='cpu')
    assert 'precision' not in only['car'] and 'AP_bev' not in only['car']
    np.testing.assert_array_equal(only['car']['precision_3d'], got['car']['precision_3d'])
    with pytest.raises(ValueError):
        evaluate.evaluate_kitti(gt_dir, res_dir, metrics=('bev',), device='cpu')
    with pytest.raises(FileNotFoundError):
        evaluate.evaluate_kitti(gt_dir, str(tmp_path / 'nowhere'), device='cpu')


def _perfect_frames(shift_t2=0.0, no_t1=False):
    """80 easy cars, 2 per frame, detected with distinct scores; the detection's 3D box is the label's, moved by
    shift_t2 along y (or carrying t1 = -1000)."""
    frames = {}
    for f in range(40):
        gts, dets = [], []
        for k in range(2):
            b2 = (100.0 + 300 * k, 150.0, 200.0 + 300 * k, 230.0)
            dims, loc, ry = (1.5, 1.6, 3.9), (-4.0 + 8 * k, 1.5, 12.0 + f), 0.1 * f - 1.0
            gts.append(ref.gt_line('Car', 0.0, 0, 0.2 * k, b2, dims, loc, ry))
            dloc = (-1000 if no_t1 else loc[0], loc[1] + shift_t2, loc[2])
            dets.append(ref.det_line('Car', 0.2 * k, b2, dims, dloc, ry, 0.99 - 0.01 * (2 * f + k)))
        frames[f] = (gts, dets)
    return frames


def test_perfect_boxes_score_100_in_every_metric():
    res = evaluate.evaluate_frames(*_frames_as_arrays(_perfect_frames()), device='cpu')
    for k in ('AP', 'AP_bev', 'AP_3d', 'AOS'):
        assert res['car'][k] == [100.0, 100.0, 100.0], k
    for m in ref.METRICS:
        assert res['car']['n_thresholds'][m].tolist() == [41, 41, 41]


def test_detections_shifted_by_their_height_keep_bev_and_lose_3d():
    """Every detection moved by h = 1.5 in t2: the height intervals only touch, every 3D overlap is 0.  The recall pass
    finds no true positive, so there is no score threshold: n_thresholds = 0, the curve is all zero, AP_3d = 0 --
    80 false negatives and 80 false positives that never enter a curve.  BEV and IMAGE do not see t2."""
    res = evaluate.evaluate_frames(*_frames_as_arrays(_perfect_frames(shift_t2=1.5)), device='cpu')
    assert res['car']['AP_bev'] == [100.0, 100.0, 100.0] and res['car']['AP'] == [100.0, 100.0, 100.0]
    assert res['car']['AP_3d'] == [0.0, 0.0, 0.0]
    assert res['car']['n_thresholds']['3d'].tolist() == [0, 0, 0] and not res['car']['precision_3d'].any()
    # half the height: IoU = (h/2) / (3h/2) = 1/3 < 0.7 as well; a tenth: 0.9 / 1.1 = 0.818 > 0.7 and all is found
    res = evaluate.evaluate_frames(*_frames_as_arrays(_perfect_frames(shift_t2=0.15)), device='cpu')
    assert res['car']['AP_3d'] == [100.0, 100.0, 100.0]
    # at the last threshold (the lowest score) all 80 are matched: tp 80, fp 0, fn 0
    assert res['car']['counts']['3d'][0][40].tolist() == [80, 0, 0]
    assert res['car']['counts']['3d'][0][0].tolist() == [1, 0, 79]


def test_mixed_3d_misses_give_the_counted_curve():
    """The perfect set with the second car of every frame moved by h in t2: in 3D 40 cars are found and 40 are not.
    The 40 true positives give thresholds at recall steps of 1/80 up to 0.5 -> 21 samples (0, 0.025 .. 0.5); at the
    k-th threshold the found cars above it are true, the shifted detections above it false positives."""
    frames = _perfect_frames()
    shifted = _perfect_frames(shift_t2=1.5)
    mixed = {f: (frames[f][0], [frames[f][1][0], shifted[f][1][1]]) for f in frames}
    res = evaluate.evaluate_frames(*_frames_as_arrays(mixed), device='cpu')
    assert res['car']['AP_bev'] == [100.0, 100.0, 100.0]
    n = int(res['car']['n_thresholds']['3d'][0])
    assert n == 21
    counts = res['car']['counts']['3d'][0][:n]
    # scores: frame f holds 0.99 - 0.02 f (found) and 0.98 - 0.02 f (shifted).  The i-th sample's threshold is the
    # score of the (2 i)-th found car (the first for i = 0): 2 i found cars and 2 i - 1 shifted ones lie at or above it
    tp = np.array([1] + [2 * i for i in range(1, 21)])
    assert counts[:, 0].tolist() == tp.tolist()
    assert counts[:, 1].tolist() == (tp - 1).tolist()
    assert counts[:, 2].tolist() == (80 - tp).tolist()
    prec = tp / (2.0 * tp - 1)
    want = np.zeros(41)
    want[:21] = [prec[i:].max() for i in range(21)]
    np.testing.assert_allclose(res['car']['precision_3d'][0], want, rtol=1e-15)
    assert abs(res['car']['AP_3d'][0] - 100 * want[::4].sum() / 11) < 1e-12


def test_class_without_ground_boxes_has_no_ground_key():
    res = evaluate.evaluate_frames(*_frames_as_arrays(_perfect_frames(no_t1=True)), device='cpu')
    assert 'precision_ground' not in res['car'] and 'AP_bev' not in res['car']
    assert res['car']['AP'] == [100.0, 100.0, 100.0]
    assert 'precision_3d' in res['car'] and res['car']['AP_3d'] == [0.0, 0.0, 0.0]     # t2 is there, the boxes are not


def test_bad_packed_input_is_refused():
    gt, det = _frames_as_arrays(_perfect_frames())
    with pytest.raises(ValueError):
        evaluate.evaluate_frames(gt, det[:-1], device='cpu')
    L = _lib.lib()
    off = np.array([0, 2, 1], dtype=np.int32)
    z = np.zeros(64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    ev, prec = np.zeros(9, np.int32), np.zeros(27 * 41)
    valid = C.c_int(0)
    rc = L.egn_kitti_eval_packed_host(2, vp(off), vp(off), vp(z), vp(z), vp(z), vp(z), vp(z), vp(z), vp(z), 7,
                                      ev.ctypes.data_as(C.POINTER(C.c_int)), C.byref(valid),
                                      prec.ctypes.data_as(C.POINTER(C.c_double)),
                                      prec.ctypes.data_as(C.POINTER(C.c_double)), None, None)
    assert rc == -1
