"""The 2-D pose annotation front end on the host (egonet_amd/common/pose_annot.py, ``device='cpu'``) against the
reference's ``annot_2dpose`` (tests/golden/pose_annot.npz), its config handling, and ``PoseFrames`` as the input of
``TrainSampleBuilder``."""
import numpy as np
import pytest

import pose_annot_cases as pc
from egonet_amd.common import pose_annot as pa

G, CASES = pc.load()


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_path_matches_the_reference(name):
    """boxes, rots, paths, the kept / dropped sets and the visibility flags equal the reference's; kpts / raw_kpts lie
    within pose_annot_cases.BOUND = 4 x 2.27e-13 px = 9.09e-13 px, four times the largest difference measured here
    on the CPU (2.2737367544323206e-13 px, case 'main'; 'tiny' gives 7.1e-15 px).  The cases with a larger
    ``min_visible`` (main_t13, c21_t9) are the ones where the two filter levels differ."""
    b = pa.PoseAnnotBuilder(pc.cfgs_of(CASES[name]['coef']), device='cpu', min_visible=CASES[name]['min_visible'])
    assert b.num_joints == 9 + 12 * len(CASES[name]['coef'])
    got = b(pc.records_of(G, name))
    pc.assert_annotations(got, pc.expected(G, name), what='host/' + name)
    visible = G[name + '/visible']
    raw = visible / b.num_joints >= pa.INLIER_SHARE
    kept = raw & (visible >= CASES[name]['min_visible'])
    assert np.array_equal(np.concatenate(b.last_src), np.nonzero(kept)[0])
    c = b.last_counts
    assert (c['labels'], c['kept_inlier'], c['kept_visible']) == (len(visible), raw.sum(), kept.sum())
    assert c['dropped_inlier'] == (~raw).sum() and c['dropped_visible'] == (raw & ~kept).sum()
    assert c['frames'] == len(pc.sizes_of(G, name)) and c['frames_kept'] == len(got['paths'])
    if CASES[name]['min_visible'] > pa.MIN_VISIBLE:         # the two levels are told apart
        assert c['dropped_visible'] > 0
        assert sum(len(r) for r in got['raw_kpts']) > sum(len(k) for k in got['kpts'])
        assert any(len(r) > len(k) for r, k in zip(got['raw_kpts'], got['kpts']))


def test_the_second_filter_skips_a_frame_whose_raw_instances_are_all_dropped():
    want, base = pc.expected(G, 'main_t13'), pc.expected(G, 'main')
    assert '000002.png' in base['paths'] and '000002.png' not in want['paths']      # its one raw car has 10 visible
    f5 = want['paths'].index('000005.png')
    assert len(want['raw_kpts'][f5]) == 30 and len(want['kpts'][f5]) == 28


def test_the_cases_are_the_ones_the_kernel_can_get_wrong():
    visible, want = G['main/visible'], pc.expected(G, 'main')
    assert list(visible[:3]) == [33, 9, 10]                     # fully inside; 9 of 33 dropped, 10 of 33 kept
    assert want['paths'] == ['000001.png', '000002.png', '000003.png', '000005.png', '000006.png']   # 0 and 4 skipped
    border = want['raw_kpts'][2]                                # frame 3: behind the camera, u = 0, u = width
    assert border[1][0, 0] == 0.0 and border[1][0, 2] == 0.0
    assert border[2][0, 0] == float(pc.sizes_of(G, 'main')[3][0]) and border[2][0, 2] == 0.0
    assert len(visible) > 32 and 1 < len(want['boxes'][3]) < 33


def test_enlarge_factor_and_the_default():
    assert pa.PoseAnnotBuilder(pc.cfgs_of([0.332, 0.667]), device='cpu').enlarge == 1.1
    b = pa.PoseAnnotBuilder(pc.cfgs_of([0.332, 0.667], enlarge=1.3), device='cpu')
    got = b(pc.records_of(G, 'tiny'))
    k = got['kpts'][0][0]
    mn, mx = k.min(axis=0), k.max(axis=0)
    c, s = (mn + mx) / 2, (mx - mn) * 1.3 / 2
    assert np.array_equal(got['boxes'][0][0], [int(c[0] - s[0]), int(c[1] - s[1]), int(c[0] + s[0]), int(c[1] + s[1])])


def test_no_label_and_no_record():
    b = pa.PoseAnnotBuilder(pc.cfgs_of([0.332, 0.667]), device='cpu')
    for records in ([], pc.records_of(G, 'main')[:1]):
        got = b(records)
        assert got == {'paths': [], 'boxes': [], 'rots': [], 'kpts': [], 'raw_kpts': []}
        assert b.last_counts['labels'] == 0 and b.last_counts['frames'] == len(records)


@pytest.mark.parametrize('edit, where', [
    ({'2d_kpt_style': 'bbox8'}, '734-736'), ({'3d_kpt_sample_style': 'centroid'}, '734-736'),
    ({'interpolate': {'flag': False}}, ':741'), ({'interpolate': {'flag': True, 'style': 'bbox12l'}}, ':745'),
    ({'interpolate': {'flag': True, 'style': 'bbox12', 'coef': [0.2, 0.4, 0.6]}}, ':727')])
def test_unsupported_config_raises_with_the_reference_line(edit, where):
    cfg = pc.cfgs_of([0.332, 0.667])
    cfg['dataset'].update(edit)
    with pytest.raises(NotImplementedError, match=where):
        pa.PoseAnnotBuilder(cfg, device='cpu')


def test_label_frame_outside_the_table_is_refused():
    b = pa.PoseAnnotBuilder(pc.cfgs_of([0.332, 0.667]), device='cpu')
    labels, alpha, lf, frames, _ = b.gather(pc.records_of(G, 'tiny'))
    with pytest.raises(ValueError):
        b.build(labels, alpha, lf + 1, frames)
    with pytest.raises(ValueError):
        b.build(labels, alpha[:-1], lf, frames)


def test_size_from_the_image_header_and_pose_frames_feed_the_sample_builder(tmp_path):
    from PIL import Image
    from egonet_amd import configs
    from egonet_amd.common import train_samples as ts
    rng = np.random.RandomState(5)
    records = pc.records_of(G, 'tiny', root=str(tmp_path))
    images = []
    for rec in records:
        w, h = rec.pop('size')                                  # the builder must read it from the PNG header
        images.append(rng.randint(0, 256, (h, w, 3), dtype=np.uint8))
        Image.fromarray(images[-1]).save(rec['path'])
    annot = pa.PoseAnnotBuilder(pc.cfgs_of(CASES['tiny']['coef']), device='cpu')(records)
    pc.assert_annotations(annot, pc.expected(G, 'tiny'), what='host/tiny from files')
    frames = pa.PoseFrames(annot)
    assert len(frames) == 3 and frames.num_joints == 33
    items = ts.collate_frames([frames[i] for i in range(len(frames))])
    for it, img, path in zip(items, images, annot['paths']):
        assert it['path'] == path and it['image'].dtype == np.uint8 and np.array_equal(it['image'], img)
    cfg = configs.tiny_config('coordinates', num_joints=33)
    cfg['heatmapModel'].update(sigma=1, target_type='gaussian')
    builder = ts.TrainSampleBuilder(cfg, device='cpu')          # gather is host math: no GPU is touched
    boxes, joints, frame = builder.gather(items)
    assert boxes.shape == (5, 4) and np.array_equal(boxes, G['tiny/boxes'].astype(np.float64))
    assert joints.shape == (5, 33, 3) and np.array_equal(joints[..., :2], np.concatenate(annot['kpts']))
    assert (joints[..., 2] == 1.0).all() and list(frame) == [0, 0, 1, 2, 2]
