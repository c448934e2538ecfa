"""Training-sample front end, host side (egonet_amd/common/train_samples.py): the vectorised per-box math against
the reference's own values (tests/golden/train_samples.npz, make_golden_train_samples.py), the per-box
get_affine_transform, the config refusals and the picklable collate function.  No GPU."""
import json
import pickle

import numpy as np
import pytest

from conftest import arr_crc, golden
from egonet_amd import synth
from egonet_amd.common import img_proc
from egonet_amd.common import train_samples as ts


def case_cfgs(settings, num_joints=33):
    """The YAML keys the builder reads, as the shipped KITTI_train_IGRs*.yml write them."""
    return {'train': True,
            'dataset': {'pth_transform': {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}},
            'heatmapModel': {'add_xy': False, 'jitter_bbox': True,
                             'jitter_params': {'shift': [0.1, 0.1], 'scaling': list(settings['scaling'])},
                             'input_size': list(settings['input_size']),
                             'heatmap_size': list(settings['heatmap_size']),
                             'num_joints': num_joints, 'target_type': 'gaussian', 'sigma': settings['sigma']}}


def case_records(g, name, with_images=False):
    """The fixture's records: its boxes / joints per frame; frames regenerated from the case's seed."""
    c = json.loads(str(g['cases']))[name]
    p = name + '/'
    frame, boxes, joints = g[p + 'frame'], g[p + 'boxes'], g[p + 'joints']
    paths = json.loads(str(g[p + 'paths']))
    imgs = None
    if with_images:
        imgs = [r['image'] for r in synth.synth_frame_records(c['n_frames'], c['boxes_per_frame'], joints.shape[1],
                                                              seed=c['seed'], hw=tuple(c['hw']))]
        assert [arr_crc(i) for i in imgs] == list(g[p + 'frames_crc'])
    return [{'image': imgs[f] if imgs else None, 'boxes': boxes[frame == f], 'joints': joints[frame == f],
             'path': paths[f]} for f in range(c['n_frames'])], c


G = golden('train_samples.npz')
CASES = sorted(json.loads(str(G['cases'])))


def test_fixture_frames_regenerate():
    for name in CASES:
        case_records(G, name, with_images=True)


@pytest.mark.parametrize('name', CASES)
def test_host_math_equals_the_reference(name):
    recs, c = case_records(G, name)
    b = ts.TrainSampleBuilder(case_cfgs(c['settings']), split=c['split'], device='cpu')
    assert b.jitter == (c['split'] == 'train')
    np.random.seed(int(G[name + '/np_seed']))
    p = b.plan(recs)
    pre = name + '/'
    kept = G[pre + 'kept']
    assert int(G['max_ins_cnt']) == ts.MAX_INS_CNT
    assert np.array_equal(p['kept'], kept)
    if b.jitter:
        np.testing.assert_allclose(p['draws'], G[pre + 'draws'], rtol=0, atol=1e-9)
    else:
        assert p['draws'] is None and G[pre + 'draws'].size == 0
    np.testing.assert_allclose(p['trans'], G[pre + 'warps'][kept], rtol=0, atol=1e-9)
    m = p['meta']
    for key in ('center', 'scale', 'transformed_joints', 'joints_vis', 'original_joints'):
        assert m[key].dtype == G[pre + key].dtype and m[key].shape == G[pre + key].shape, key
        np.testing.assert_allclose(m[key], G[pre + key], rtol=0, atol=1e-9, err_msg=key)
    assert m['path'] == json.loads(str(G[pre + 'paths']))
    assert np.array_equal(p['frame'], G[pre + 'frame'][kept])


def test_length_limit_draws_after_all_jitter_draws():
    recs, c = case_records(G, 'limit')
    assert sum(len(r['boxes']) for r in recs) == 150
    b = ts.TrainSampleBuilder(case_cfgs(c['settings']), device='cpu')
    np.random.seed(int(G['limit/np_seed']))
    draws = np.random.rand(150, 4)
    chosen = np.random.choice(150, ts.MAX_INS_CNT, replace=False)
    np.random.seed(int(G['limit/np_seed']))
    p = b.plan(recs)
    assert np.array_equal(p['draws'], draws) and np.array_equal(p['kept'], chosen)


def test_affines_bitwise_equal_the_per_box_function():
    rng = np.random.RandomState(11)
    for input_size in ([256, 256], [192, 256]):
        b = ts.TrainSampleBuilder(case_cfgs({'input_size': input_size, 'heatmap_size': [64, 64], 'sigma': 1,
                                             'scaling': [0.4, 0.4]}), device='cpu')
        c = np.stack([rng.uniform(-100, 1400, 1000), rng.uniform(-50, 420, 1000)], axis=1)
        s = rng.uniform(0.05, 3.0, (1000, 2))
        got = b.affines(c, s)
        want = np.stack([img_proc.get_affine_transform(c[i], s[i], 0, b.input_hw) for i in range(1000)])
        assert np.array_equal(got, want)


def test_resize_and_jitter_match_the_per_box_helpers():
    """resize_boxes equals img_proc.resize_bbox bit for bit (both branches of the aspect test)."""
    b = ts.TrainSampleBuilder(case_cfgs({'input_size': [192, 256], 'heatmap_size': [48, 64], 'sigma': 2,
                                         'scaling': [0.4, 0.4]}), device='cpu')
    boxes = synth.synth_boxes(300, seed=5)
    c, s = b.resize_boxes(boxes)
    for i, bb in enumerate(boxes):
        r = img_proc.resize_bbox(*bb, target_ar=b.input_hw[0] / b.input_hw[1])
        assert np.array_equal(r['c'], c[i]) and np.array_equal(r['s'], s[i])


def test_missing_visibility_column_means_visible():
    b = ts.TrainSampleBuilder(case_cfgs({'input_size': [256, 256], 'heatmap_size': [64, 64], 'sigma': 1,
                                         'scaling': [0.4, 0.4]}, num_joints=5), split='valid', device='cpu')
    rec = synth.synth_frame_records(1, 3, 5, seed=2, hw=(100, 200))[0]
    p3 = b.plan([dict(rec, joints=np.concatenate([rec['joints'][..., :2], np.ones((3, 5, 1))], axis=2))])
    p2 = b.plan([dict(rec, joints=rec['joints'][..., :2])])
    for k in ('transformed_joints', 'joints_vis', 'original_joints', 'center', 'scale'):
        assert np.array_equal(p2['meta'][k], p3['meta'][k]), k
    assert (p2['meta']['joints_vis'] == 1).all()


def _base():
    return case_cfgs({'input_size': [256, 256], 'heatmap_size': [64, 64], 'sigma': 1, 'scaling': [0.4, 0.4]})


@pytest.mark.parametrize('edit,exc,words', [
    (lambda c: c['heatmapModel'].update(target_type='offset'), NotImplementedError, 'gaussian'),
    (lambda c: c['heatmapModel'].update(use_different_joints_weight=True), NotImplementedError, 'joints_weight'),
    (lambda c: c['heatmapModel'].update(add_xy=True), NotImplementedError, 'add_xy'),
    (lambda c: c['dataset']['pth_transform'].update(mean=[0.485, 0.456, 0.406, 0., 0.]), ValueError, '3 entries'),
    (lambda c: c['dataset']['pth_transform'].update(std=[0.2, 0.2]), ValueError, '3 entries'),
])
def test_config_refusals(edit, exc, words):
    cfg = _base()
    edit(cfg)
    with pytest.raises(exc, match=words):
        ts.TrainSampleBuilder(cfg, device='cpu')


def test_jitter_needs_train_split_and_train_flag():
    assert ts.TrainSampleBuilder(_base(), split='train', device='cpu').jitter
    assert not ts.TrainSampleBuilder(_base(), split='valid', device='cpu').jitter
    cfg = _base()
    cfg['train'] = False
    assert not ts.TrainSampleBuilder(cfg, split='train', device='cpu').jitter


def test_bad_records_are_refused():
    b = ts.TrainSampleBuilder(_base(), device='cpu')
    rec = synth.synth_frame_records(1, 2, 33, seed=1, hw=(50, 80))[0]
    with pytest.raises(ValueError, match='no box'):
        b.plan([dict(rec, boxes=np.zeros((0, 4)), joints=np.zeros((0, 33, 3)))])
    with pytest.raises(ValueError, match='num_joints'):
        b.plan([dict(rec, joints=rec['joints'][:, :5])])


def test_collate_frames_survives_pickling():
    f = pickle.loads(pickle.dumps(ts.collate_frames))
    recs = synth.synth_frame_records(2, 1, 3, seed=0, hw=(8, 12))
    out = f(recs)
    assert isinstance(out, list) and out[0] is recs[0] and out[1] is recs[1]


def test_synth_frame_records_are_seeded():
    a = synth.synth_frame_records(2, 3, 33, seed=4, hw=(40, 60))
    b = synth.synth_frame_records(2, 3, 33, seed=4, hw=(40, 60))
    for x, y in zip(a, b):
        assert np.array_equal(x['image'], y['image']) and np.array_equal(x['joints'], y['joints'])
        assert x['image'].dtype == np.uint8 and x['image'].shape == (40, 60, 3) and x['joints'].shape == (3, 33, 3)
    assert set(np.unique(a[0]['joints'][..., 2])) <= {0.0, 0.3, 1.0}
