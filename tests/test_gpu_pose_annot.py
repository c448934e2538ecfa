"""The 2-D pose annotations on the device (csrc/pose_annot.hip egn_pose2d_annot_f64, egonet_amd/common/pose_annot.py)
against the reference's ``annot_2dpose`` (tests/golden/pose_annot.npz) and against the host path of the same module,
at the bound of tests/test_pose_annot_cpu.py (pose_annot_cases.BOUND, measured on the CPU); boxes, counts, ``src`` and
the order are equal; the cases and flat builds with a larger ``min_visible`` are the ones where the two filter levels
(raw_kpts against kpts / boxes / rots / src) hold different rows.  Then the entry point's edges: no label, one label,
33 labels in one frame (two blocks), 65 over three frames, two streams, a workspace that is too small."""
import numpy as np
import pytest
import torch

import pose_annot_cases as pc
from egonet_amd import _lib
from egonet_amd.common import pose_annot as pa

pytestmark = pytest.mark.gpu
G, CASES = pc.load()
_HOST = {}


def _builders(name, min_visible=None):
    cfg = pc.cfgs_of(CASES[name]['coef'])
    mv = CASES[name]['min_visible'] if min_visible is None else min_visible
    return pa.PoseAnnotBuilder(cfg, min_visible=mv), pa.PoseAnnotBuilder(cfg, device='cpu', min_visible=mv)


def _host_annotations(name):
    """The host path's result per case, computed once and left unchanged."""
    if name not in _HOST:
        _HOST[name] = _builders(name)[1](pc.records_of(G, name))
    return _HOST[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_device_path_matches_the_reference_and_the_host_path(name):
    dev, host = _builders(name)
    assert dev.device.type == 'cuda'
    before = _lib.lib().egn_launch_count()
    got = dev(pc.records_of(G, name))
    assert _lib.lib().egn_launch_count() - before == 4            # flags, two scans, write: the native path ran
    pc.assert_annotations(got, pc.expected(G, name), what='device/' + name)
    want = _host_annotations(name)
    pc.assert_annotations(got, dict(want, paths=list(want['paths'])), what='device vs host/' + name)
    host(pc.records_of(G, name))
    assert dev.last_counts == host.last_counts
    assert all(np.array_equal(a, b) for a, b in zip(dev.last_src, host.last_src))
    if CASES[name]['min_visible'] > pa.MIN_VISIBLE:         # the cases that tell the two filter levels apart
        assert dev.last_counts['dropped_visible'] > 0
        assert any(len(r) > len(k) for r, k in zip(got['raw_kpts'], got['kpts']))


def _flat_case(A):
    """(labels, alpha, label_frame, frames) with A labels from the fixture's 'main' case."""
    _, host = _builders('main')
    labels, alpha, lf, frames, _ = host.gather(pc.records_of(G, 'main'))
    if A == 1:
        return labels[:1], alpha[:1], lf[:1] * 0, frames[1:2]
    if A == 33:                                                  # frame 5: the 33 cars of one frame
        m = lf == 5
        return labels[m], alpha[m], np.zeros(33, dtype=np.int32), frames[5:6]
    assert A == 65
    idx = np.concatenate([np.arange(42), np.arange(6, 29)])
    lab = labels[idx].copy()
    lab[42:, 3] += 0.37                                          # the repeated labels are moved sideways
    return lab, alpha[idx], np.repeat([0, 1, 2], [20, 33, 12]).astype(np.int32), frames[[1, 5, 3]]


def _compare_flat(got, want):
    for key in ('totals', 'frame_raw', 'frame_kept', 'src', 'boxes', 'rots'):
        assert np.array_equal(got[key], want[key]), key
    assert got['boxes'].dtype == np.int32 and got['src'].dtype == np.int32
    assert np.array_equal(got['raw_kpts'][..., 2], want['raw_kpts'][..., 2])
    worst = 0.0
    for key in ('kpts', 'raw_kpts'):
        assert got[key].shape == want[key].shape
        if got[key].size:
            worst = max(worst, np.abs(got[key][..., :2] - want[key][..., :2]).max())
    print('largest |device - host| %.3e px (bound %.3e)' % (worst, pc.BOUND))
    assert worst <= pc.BOUND


@pytest.mark.parametrize('A, min_visible', [(1, 4), (33, 4), (65, 4), (33, 13), (65, 13), (65, 34)])
def test_flat_build_against_the_host_path(A, min_visible):
    """min_visible 13: the second level drops labels the first kept -- among the first 32 labels, so the later
    blocks' two row offsets differ, and the per-frame counts and the totals of the two levels differ; 34: nothing is
    kept, the raw rows are all there."""
    dev, host = _builders('main', min_visible)
    case = _flat_case(A)
    want = host.build_host(*case)
    if min_visible == 4:
        assert want['totals'][1] > 0 and (A == 1 or want['totals'][0] < A)  # something kept, something dropped
    elif min_visible == 13:
        assert 0 < want['totals'][1] < want['totals'][0] < A
        assert not np.array_equal(want['frame_raw'], want['frame_kept'])
        if A == 65:                                              # frame 0 = labels 0..19, inside the first block
            assert want['frame_raw'][0] > want['frame_kept'][0] > 0
        else:                                                    # the two cars with 12 visible points
            assert want['totals'][0] - want['totals'][1] == 2
    else:
        assert want['totals'][1] == 0 and want['totals'][0] > 0 and not want['frame_kept'].any()
    _compare_flat(dev.build_device(*case), want)


def test_no_label_gives_empty_outputs():
    dev, host = _builders('main')
    frames = host.gather(pc.records_of(G, 'main'))[3]
    empty = (np.zeros((0, 7)), np.zeros(0), np.zeros(0, dtype=np.int32))
    got = dev.build_device(*empty, frames)                        # rc 0: build_device raises otherwise
    _compare_flat(got, host.build_host(*empty, frames))
    assert got['totals'].tolist() == [0, 0] and not got['frame_raw'].any() and got['kpts'].shape == (0, 33, 2)
    got = dev.build_device(*empty, np.zeros((0, 14)))
    assert got['totals'].tolist() == [0, 0] and got['frame_kept'].shape == (0,)
    assert dev(pc.records_of(G, 'main')[:1]) == {'paths': [], 'boxes': [], 'rots': [], 'kpts': [], 'raw_kpts': []}


def test_two_streams_give_identical_bytes():
    dev, _ = _builders('main')
    case = _flat_case(65)
    up = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in case]
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(dev.launch(*up))
    torch.cuda.synchronize()
    a, b = outs
    n_raw, n = a['totals'].tolist()
    assert a['totals'].tolist() == b['totals'].tolist() and n > 0
    for key, rows in (('raw_kpts', n_raw), ('kpts', n), ('boxes', n), ('rots', n), ('src', n), ('frame_raw', None),
                      ('frame_kept', None)):
        x, y = a[key][:rows].cpu().numpy(), b[key][:rows].cpu().numpy()
        assert x.tobytes() == y.tobytes(), key


def test_short_workspace_is_refused():
    dev, _ = _builders('main')
    L = _lib.lib()
    assert L.egn_pose2d_annot_ws_bytes(-1) == -1
    case = _flat_case(33)
    up = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in case]
    need = L.egn_pose2d_annot_ws_bytes(33)
    assert need > 0
    before = L.egn_launch_count()
    with pytest.raises(ValueError, match='bad argument'):
        dev.launch(*up, ws=torch.empty(need - 1, dtype=torch.uint8, device='cuda'))
    assert L.egn_launch_count() == before                         # refused, not used
    dev.launch(*up, ws=torch.empty(need, dtype=torch.uint8, device='cuda'))
    torch.cuda.synchronize()
