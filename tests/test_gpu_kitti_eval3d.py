"""The KITTI evaluator on the GPU (csrc/kitti_eval.hip): device overlaps against the host entry and scipy, the device
evaluator against the host path of the same tree (integer counts and curves bit for bit), the smallest frame sets that
can go wrong, reproducibility and the launch count."""
import numpy as np
import pytest
import torch

import kitti_eval3d_ref as ref
import test_kitti_eval3d_cpu as cpu
from egonet_amd import _lib, evaluate

pytestmark = pytest.mark.gpu

CURVES = ('precision', 'aos', 'precision_ground', 'precision_3d')


def assert_same(got, want):
    """Two results of evaluate_frames / evaluate_kitti: same keys, integer counts and curves bit for bit."""
    assert got['n_frames'] == want['n_frames'] and got['aos_valid'] == want['aos_valid']
    assert set(got) == set(want)
    for name in evaluate.CLASSES:
        if name not in want:
            continue
        assert set(got[name]) == set(want[name])
        for metric in want[name]['counts']:
            np.testing.assert_array_equal(got[name]['n_thresholds'][metric], want[name]['n_thresholds'][metric])
            np.testing.assert_array_equal(got[name]['counts'][metric], want[name]['counts'][metric])
        for k in CURVES:
            if k in want[name] and want[name][k] is not None:
                np.testing.assert_array_equal(got[name][k], want[name][k])              # same doubles, NaN == NaN
        for k in ('AP', 'AOS', 'AP_bev', 'AP_3d'):
            if k in want[name]:
                assert repr(got[name][k]) == repr(want[name][k])


def both(gt_frames, det_frames):
    dev = evaluate.evaluate_frames(gt_frames, det_frames, device='cuda')
    host = evaluate.evaluate_frames(gt_frames, det_frames, device='cpu')
    assert_same(dev, host)
    return dev


def test_device_overlaps_against_host_and_scipy():
    """The 480 pairs of the host test.  Bound 1e-9 against scipy and against the host entry (the device's sin / cos
    may differ from the host's in the last place; the image overlap has neither and must be equal).  The test prints
    the measured differences.  The host-device difference has not been
    recorded here yet: this file was written without a run on a GPU."""
    dets, gts, want = cpu.scipy_overlaps()
    host = cpu.host_overlaps(dets, gts)
    d = torch.tensor([ref.box12(b) for b in dets], dtype=torch.float64, device='cuda')
    g = torch.tensor([ref.box12(b) for b in gts], dtype=torch.float64, device='cuda')
    for crit in (-1, 0, 1):
        out = torch.full((len(dets), 4), float('nan'), dtype=torch.float64, device='cuda')
        _lib.check(_lib.lib().egn_kitti_overlap_dev_f64(_lib.ptr(d), _lib.ptr(g), len(dets), crit, _lib.ptr(out),
                                                        _lib.current_stream()), 'egn_kitti_overlap_dev_f64')
        got = out.cpu().numpy()
        to_host = np.abs(got - cpu.host_overlaps(dets, gts, crit)).max()
        print('criterion %d: device - host %.3g' % (crit, to_host))
        assert to_host < cpu.BOUND
        if crit == -1:
            to_scipy = np.abs(got[:, 1:] - want).max()
            print('device - scipy %.3g' % to_scipy)
            assert to_scipy < cpu.BOUND
            np.testing.assert_array_equal(got[:, 0], host[:, 0])        # the image overlap has no sin / cos in it
    same = torch.tensor([ref.box12(cpu.box(ry=0.7, t1=-13.25))], dtype=torch.float64, device='cuda')
    out = torch.zeros((1, 4), dtype=torch.float64, device='cuda')
    _lib.check(_lib.lib().egn_kitti_overlap_dev_f64(_lib.ptr(same), _lib.ptr(same), 1, -1, _lib.ptr(out),
                                                    _lib.current_stream()))
    assert out.cpu().numpy()[0, :3].tolist() == [1.0, 1.0, 1.0]


@pytest.mark.parametrize('seed', cpu.SEEDS)
def test_device_evaluator_equals_host_path(seed):
    """The frame sets whose overlaps the host test asserts to stay 1e-6 away from every class threshold."""
    frames = ref.random_frames(seed)
    res = both(*cpu._frames_as_arrays(frames))
    assert np.count_nonzero(res['car']['precision_3d'][2]) >= 2 and res['aos_valid']


def test_directories_on_the_device(tmp_path):
    gt_dir, res_dir = cpu._write(tmp_path, ref.random_frames(1))
    assert_same(evaluate.evaluate_kitti(gt_dir, res_dir, device='cuda'), evaluate.evaluate_kitti(gt_dir, res_dir, device='cpu'))
    assert_same(evaluate.evaluate_kitti(gt_dir, res_dir), evaluate.evaluate_kitti(gt_dir, res_dir, device='cpu'))
    only = evaluate.evaluate_kitti(gt_dir, res_dir, metrics=('ground',), device='cuda')
    assert_same(only, evaluate.evaluate_kitti(gt_dir, res_dir, metrics=('ground',), device='cpu'))


def _car(k, score=None, shift=0.0):
    b2 = (20.0 + 40 * (k % 30), 100.0 + 5 * (k // 30), 50.0 + 40 * (k % 30), 160.0 + 5 * (k // 30))
    dims, loc, ry = (1.5, 1.6, 3.9), (-40.0 + 6 * (k % 30) + shift, 1.5, 10.0 + 7 * (k // 30)), 0.05 * k
    if score is None:
        return ref.gt_line('Car', 0.0, 0, 0.1 * k, b2, dims, loc, ry)
    return ref.det_line('Car', 0.1 * k + 0.2, b2, dims, loc, ry, score)


def _arrays(gts, dets):
    return [ref.to_arrays(g, False) for g in gts], [ref.to_arrays(d, True) for d in dets]


def test_smallest_frame_sets():
    res = both(*_arrays([[], []], [[], []]))                                    # frames, no boxes at all
    assert set(res) == {'n_frames', 'aos_valid'} and res['n_frames'] == 2
    res = both(*_arrays([[_car(0), _car(1)]], [[]]))                            # ground truth, no detections
    assert set(res) == {'n_frames', 'aos_valid'}
    res = both(*_arrays([[]], [[_car(0, 0.9)]]))                                # detections, no ground truth
    assert res['car']['n_thresholds']['3d'].tolist() == [0, 0, 0]
    res = both(*_arrays([[_car(0)]], [[_car(0, 0.9)]]))                         # a single pair
    assert res['car']['counts']['3d'][0][0].tolist() == [1, 0, 0] and res['car']['precision_3d'][0][0] == 1.0
    assert evaluate.evaluate_frames([], [], device='cuda') == {'n_frames': 0, 'aos_valid': True}


def test_more_detections_than_a_wave_and_more_than_one_mask_word():
    """One frame, 30 ground truths and 70 detections: 30 exact ones (the last 6 of them beyond bit 64 of the
    assigned set), 40 moved by 1.2 m, which overlap their car by less than 0.7 in BEV and 3D and fully in the image."""
    gts = [_car(k) for k in range(30)]
    dets = [_car(k, 0.91 + 0.001 * k, shift=1.2) for k in range(30)] + [_car(k, 0.95 + 0.001 * k, shift=1.2) for k in range(10)]
    dets = dets[:34] + [_car(k, 0.9 - 0.01 * k) for k in range(24)] + dets[34:] + [_car(k, 0.9 - 0.01 * k) for k in range(24, 30)]
    assert len(dets) == 70
    res = both(*_arrays([gts, [_car(3)]], [dets, [_car(3, 0.95)]]))
    last = int(res['car']['n_thresholds']['3d'][0]) - 1
    assert res['car']['counts']['3d'][0][last].tolist() == [31, 40, 0]
    assert res['car']['counts']['image'][0][int(res['car']['n_thresholds']['image'][0]) - 1][0] == 31


def test_all_41_recall_samples_and_fewer():
    full = cpu._perfect_frames()
    res = both(*cpu._frames_as_arrays(full))
    assert res['car']['n_thresholds']['3d'].tolist() == [41, 41, 41] and res['car']['AP_3d'] == [100.0] * 3
    shifted = cpu._perfect_frames(shift_t2=1.5)
    mixed = {f: (full[f][0], [full[f][1][0], shifted[f][1][1]]) for f in full}
    res = both(*cpu._frames_as_arrays(mixed))
    assert res['car']['n_thresholds']['3d'].tolist() == [21, 21, 21]
    assert res['car']['n_thresholds']['ground'].tolist() == [41, 41, 41]


def test_two_runs_give_the_same_bits():
    arrays = cpu._frames_as_arrays(ref.random_frames(2))
    a = evaluate.evaluate_frames(*arrays, device='cuda')
    b = evaluate.evaluate_frames(*arrays, device='cuda')
    assert_same(a, b)
    for name in evaluate.CLASSES:
        if name in a:
            for k in (c for c in CURVES if c in a[name]):
                assert a[name][k].tobytes() == b[name][k].tobytes()


def test_launch_count_does_not_depend_on_the_number_of_frames():
    L = _lib.lib()
    few, many = ref.random_frames(0, 3), ref.random_frames(0, 60)
    assert sum(len(d) for _, d in few.values()) > 0
    moved = []
    stream = torch.cuda.Stream()
    for frames in (few, many):
        arrays = cpu._frames_as_arrays(frames)
        with torch.cuda.stream(stream):
            before = L.egn_launch_count()
            evaluate.evaluate_frames(*arrays, device='cuda')
            moved.append(L.egn_launch_count() - before)
        before = L.egn_launch_count()
        evaluate.evaluate_frames(*arrays, device='cpu')
        assert L.egn_launch_count() == before
    assert moved[0] == moved[1] == 4, moved
