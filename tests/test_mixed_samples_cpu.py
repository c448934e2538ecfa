"""Mixed batches, host side (egonet_amd/common/train_samples.py with cfgs['ss'], MixedFrames): the draw order, the
instance order, the affines, the meta and the three length_limit cases against the reference's own run
(tests/golden/mixed_samples.npz, make_golden_mixed.py), and the composition of the mixed loss from the oracle's parts
against the reference's JointsCompositeLoss (tests/golden/mixed_loss.npz).  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import arr_crc, golden
from egonet_amd import synth
from egonet_amd.common import train_samples as ts
from oracle.hrnet_train_oracle import _composite_supervised, cross_ratio_loss
from test_train_samples_cpu import case_cfgs

G = golden('mixed_samples.npz')
GL = golden('mixed_loss.npz')
ALL = json.loads(str(G['cases']))
CASES = sorted(ALL)
POOL = json.loads(str(G['pool']))
META_KEYS = ('center', 'scale', 'transformed_joints', 'joints_vis', 'original_joints')


def mixed_cfgs(c):
    cfg = case_cfgs(c['settings'])
    cfg['ss'] = {'flag': True, 'max_per_img': c['max_per_img'], 'img_root': POOL['img_root']}
    return cfg


def mixed_records(name, with_images=False):
    """The fixture's labelled records (frames regenerated from the case's seed) and the case's settings."""
    c = ALL[name]
    p = name + '/'
    frame, boxes, joints = G[p + 'frame'], G[p + 'boxes'], G[p + 'joints']
    paths = json.loads(str(G[p + 'paths']))
    imgs = None
    if with_images:
        imgs = [r['image'] for r in synth.synth_frame_records(len(c['per_frame']), max(c['per_frame']), joints.shape[1],
                                                              seed=c['seed'], hw=tuple(c['hw']))]
        assert [arr_crc(i) for i in imgs] == list(G[p + 'frames_crc'])
    return [{'image': imgs[f] if imgs else None, 'boxes': boxes[frame == f], 'joints': joints[frame == f],
             'path': paths[f]} for f in range(len(c['per_frame']))], c


def mixed_pool(with_images=False):
    """The unlabelled pool: boxes from the fixture, frames regenerated from the pool's seed."""
    imgs = None
    if with_images:
        imgs = [r['image'] for r in synth.synth_frame_records(POOL['n_frames'], POOL['boxes_per_frame'],
                                                              G['pool/joints'].shape[2], seed=POOL['seed'],
                                                              hw=tuple(POOL['hw']))]
        assert [arr_crc(i) for i in imgs] == list(G['pool/frames_crc'])
    return [{'image': imgs[i] if imgs else None, 'boxes': G['pool/boxes'][i], 'path': POOL['paths'][i]}
            for i in range(POOL['n_frames'])]


def mixed_loss(out, target, joints_xy, img_size, w_hm, w_coor, w_cr, cr_indices, target_cr, cr_loss_thres,
               cr_type='sl1'):
    """function.py:170-202 for ``n_fs = len(target) <= N``: the supervised terms of the oracle on the sliced prediction,
    its cross-ratio term on all rows.  Returns (total, supervised part, weighted cross-ratio term)."""
    n_fs = len(target)
    sliced = (out[0][:n_fs], out[1][:n_fs]) if isinstance(out, tuple) else out[:n_fs]
    sup = _composite_supervised(sliced, target, joints_xy, img_size, w_hm, w_coor)
    if w_cr is None or not isinstance(out, tuple):
        return sup, sup, None
    cr = cross_ratio_loss(out[1], cr_indices, target_cr, cr_loss_thres, cr_type) * w_cr
    return sup + cr, sup, cr


def check_plan(p, name, pool, recs):
    """A plan against the reference's batch of case ``name`` (everything but the draws)."""
    pre = name + '/'
    kept, n_fs = G[pre + 'kept'], int(G[pre + 'n_fs'])
    assert np.array_equal(p['kept'], kept)
    assert p.get('n_fs', len(p['kept'])) == n_fs
    np.testing.assert_allclose(p['trans'], G[pre + 'warps'][G[pre + 'inst_warp'][kept]], rtol=0, atol=1e-9)
    # the source frame of every instance: a labelled record, or the pool frame the reference drew
    sources = p.get('sources', recs)
    want_src = G[pre + 'inst_frame'][kept]
    for f, w in zip(p['frame'], want_src):
        assert sources[f] is (recs[w] if w < len(recs) else pool[w - len(recs)])
    m = p['meta']
    for key in META_KEYS:
        assert m[key].dtype == G[pre + key].dtype and m[key].shape == G[pre + key].shape, key
        np.testing.assert_allclose(m[key], G[pre + key], rtol=0, atol=1e-9, err_msg=key)
        assert len(m[key]) == n_fs
    assert m['path'] == json.loads(str(G[pre + 'paths']))
    cnt = int(G[pre + 'fs_instance_cnt'])
    assert ('fs_instance_cnt' in m) == (cnt >= 0)
    if cnt >= 0:
        assert m['fs_instance_cnt'] == cnt


class _Recorder(object):
    """The global np.random behind the three calls the builder may make, each logged."""

    def __init__(self):
        self.log = {'rand': [], 'randint': [], 'choice': []}

    def rand(self, *a):
        v = np.random.rand(*a)
        self.log['rand'].append(np.asarray(v, dtype=np.float64).reshape(-1, 4))
        return v

    def randint(self, *a, **k):
        v = np.random.randint(*a, **k)
        self.log['randint'].append(int(v))
        return v

    def choice(self, *a, **k):
        v = np.random.choice(*a, **k)
        self.log['choice'].append(np.asarray(v))
        return v


@pytest.mark.parametrize('name', CASES)
def test_plan_reproduces_the_reference_batch_and_its_draws(name):
    recs, c = mixed_records(name)
    pool = mixed_pool()
    b = ts.TrainSampleBuilder(mixed_cfgs(c), split=c['split'], device='cpu')
    assert b.mix == (c['split'] == 'train') and int(G['max_ins_cnt']) == ts.MAX_INS_CNT
    rng = _Recorder()
    np.random.seed(int(G[name + '/np_seed']))
    p = b.plan(recs, rng, unlabelled=pool)
    pre = name + '/'
    got = np.concatenate(rng.log['rand']) if rng.log['rand'] else np.zeros((0, 4))
    assert got.shape == G[pre + 'rand'].shape
    assert np.array_equal(got, G[pre + 'rand'])
    assert rng.log['randint'] == list(G[pre + 'randint'])
    assert len(rng.log['choice']) == (1 if G[pre + 'choice'].size else 0)
    if rng.log['choice']:
        assert np.array_equal(rng.log['choice'][0], G[pre + 'choice'])
    if b.mix:
        assert np.array_equal(p['draws'], G[pre + 'rand']) and p['ss_idx'] == list(G[pre + 'randint'])
    check_plan(p, name, pool, recs)
    # what the case is there for
    n_ss = len(p['kept']) - p.get('n_fs', len(p['kept']))
    want = {'mix': (6, 6, 3), 'full': (11, 2, 1), 'valid': (6, 0, 0), 'limit_fs': (140, 0, 25),
            'limit_ss': (120, 20, 20)}[name]
    assert (p.get('n_fs', len(p['kept'])), n_ss, len(rng.log['randint'])) == want
    if name == 'mix':
        assert [k for _, k in p['ss_boxes']] == [2, 3, 1]
    if name == 'full':
        assert [f for f, _ in p['ss_boxes']] == [1]              # no draw for the frames with 4 and 5 boxes


@pytest.mark.parametrize('name', ['mix', 'full', 'limit_ss'])
def test_records_that_carry_ss_give_the_same_plan_without_a_randint(name):
    recs, c = mixed_records(name)
    pool = mixed_pool()
    drawn = list(G[name + '/randint'])
    short = [f for f, r in enumerate(recs) if len(r['boxes']) < c['max_per_img']]
    assert len(short) == len(drawn)
    carried = list(recs)
    for f, idx in zip(short, drawn):
        carried[f] = dict(recs[f], ss=pool[idx])
    b = ts.TrainSampleBuilder(mixed_cfgs(c), split=c['split'], device='cpu')

    class _NoRandint(_Recorder):
        def randint(self, *a, **k):
            raise AssertionError('the record carries its unlabelled frame: no randint')
    # the reference's stream without its randint draws: replay the recorded rand values
    rng = _NoRandint()
    seq = iter(G[name + '/rand'])
    rng.rand = lambda n, k: np.array([next(seq) for _ in range(n)], dtype=np.float64).reshape(n, k)
    p = b.plan(carried, rng)
    assert next(seq, None) is None and p['ss_idx'] == []
    # (the sources are the carried dicts' pool entries, and the labelled records are the carried ones)
    check_plan(p, name, pool, carried)


def test_a_short_frame_without_ss_and_without_a_pool_is_refused():
    recs, c = mixed_records('mix')
    b = ts.TrainSampleBuilder(mixed_cfgs(c), device='cpu')
    with pytest.raises(ValueError, match='MixedFrames'):
        b.plan(recs)


@pytest.mark.parametrize('mix', [False, True])
def test_labelled_only_records_consume_the_stream_as_today(mix):
    """Without unlabelled boxes -- the mix off, or on with every frame at max_per_img -- the per-frame draws are the
    stream of one rand(n_all, 4), followed by the choice."""
    for n_frames, bpf in ((4, 3), (25, 6)):
        recs = synth.synth_frame_records(n_frames, bpf, 33, seed=5, hw=(60, 90))
        cfg = case_cfgs({'input_size': [256, 256], 'heatmap_size': [64, 64], 'sigma': 1, 'scaling': [0.4, 0.4]})
        if mix:
            cfg['ss'] = {'flag': True, 'max_per_img': bpf}
        n_all = n_frames * bpf
        np.random.seed(91)
        draws = np.random.rand(n_all, 4)
        chosen = np.random.choice(n_all, ts.MAX_INS_CNT, replace=False) if n_all > ts.MAX_INS_CNT else np.arange(n_all)
        after = np.random.rand()
        np.random.seed(91)
        p = ts.TrainSampleBuilder(cfg, device='cpu').plan(recs)
        assert np.random.rand() == after
        assert np.array_equal(p['draws'], draws) and np.array_equal(p['kept'], chosen)
        plain = ts.TrainSampleBuilder(dict(cfg, ss={'flag': False}), device='cpu')
        np.random.seed(91)
        q = plain.plan(recs)
        assert np.array_equal(p['trans'], q['trans']) and np.array_equal(p['frame'], q['frame'])
        for key in META_KEYS:
            assert np.array_equal(p['meta'][key], q['meta'][key]), key
        assert 'fs_instance_cnt' not in q['meta']


def test_the_angle_targets_ignore_the_flag():
    cfg = mixed_cfgs(ALL['mix'])
    assert not ts.TrainSampleBuilder(cfg, device='cpu', target='alpha').mix
    assert not ts.TrainSampleBuilder(dict(cfg, exp_type='baselinetheta'), device='cpu').mix
    assert not ts.TrainSampleBuilder(cfg, split='valid', device='cpu').mix
    assert ts.TrainSampleBuilder(cfg, device='cpu').mix
    off = dict(cfg, ss={'flag': False, 'max_per_img': 4})
    assert not ts.TrainSampleBuilder(off, device='cpu').mix


class _Frames(object):
    num_joints = 33

    def __init__(self, records):
        self.records = records

    def __len__(self):
        return len(self.records)

    def __getitem__(self, i):
        return self.records[i]


def test_mixed_frames_adds_ss_only_below_max_per_img(tmp_path):
    from PIL import Image
    pool = mixed_pool(with_images=True)
    root = str(tmp_path / 'images')
    os.makedirs(root)
    for r in pool:
        Image.fromarray(r['image']).save(os.path.join(root, os.path.basename(r['path'])))
    record = {'paths': [r['path'] for r in pool], 'boxes': [r['boxes'] for r in pool]}
    assert all(os.path.dirname(p) and not os.path.exists(p) for p in record['paths'])     # only the basename counts
    recs, _ = mixed_records('full')                                                       # 4, 2 and 5 boxes
    npy = str(tmp_path / 'ss_record.npy')
    np.save(npy, np.array(dict(record, kpts=[None] * len(pool)), dtype=object))
    for source in (record, npy):
        ds = ts.MixedFrames(_Frames(recs), source, root, 4)
        assert len(ds) == 3 and ds.num_joints == 33
        np.random.seed(3)
        want = [int(np.random.randint(0, len(pool)))]
        state = np.random.get_state()[1].copy()
        np.random.seed(3)
        items = [ds[i] for i in range(3)]
        assert np.array_equal(np.random.get_state()[1], state)           # one randint, for the frame with 2 boxes
        assert 'ss' not in items[0] and 'ss' not in items[2] and items[0] is recs[0]
        ss = items[1]['ss']
        assert ss['path'] == os.path.join(root, os.path.basename(pool[want[0]]['path']))
        assert np.array_equal(ss['image'], pool[want[0]]['image']) and ss['image'].dtype == np.uint8
        assert np.array_equal(ss['boxes'], pool[want[0]]['boxes'])
        assert items[1]['boxes'] is recs[1]['boxes'] and 'ss' not in recs[1]
    with pytest.raises(ValueError, match='at least one frame'):
        ts.MixedFrames(_Frames(recs), {'paths': [], 'boxes': []}, root, 4)


def test_mixed_loss_composition_equals_the_reference():
    """The helper the GPU tests use as the reference of a mixed step, pinned on the reference's own
    JointsCompositeLoss.forward with 3 predictions and 2 targets (make_golden_mixed.py), term by term; 2e-6 relative,
    the bound of the cr_loss.npz pin (tests/test_oracle_golden.py)."""
    maps, coords = torch.from_numpy(GL['maps']), torch.from_numpy(GL['coords'])
    target, joints = torch.from_numpy(GL['target']), torch.from_numpy(GL['joints'])[:, :, :2]
    w = [float(v) for v in GL['weights']]
    assert len(maps) == 3 and len(target) == 2 and len(joints) == 2
    kw = dict(cr_indices=GL['cr_indices'], target_cr=float(GL['target_cr']), cr_loss_thres=float(GL['cr_loss_thres']))
    out = (maps, coords)
    total, sup, cr = mixed_loss(out, target, joints, GL['img_size'], w[0], w[1], w[2], **kw)
    hm = mixed_loss(out, target, joints, GL['img_size'], w[0], 0.0, None, **kw)[0]
    coor = mixed_loss(out, target, joints, GL['img_size'], 0.0, w[1], None, **kw)[0]
    for got, key in ((total, 'total'), (hm, 'hm'), (coor, 'coor'), (cr, 'cr')):
        print('%-5s %.9g (reference %.9g)' % (key, float(got), float(GL[key])))
        np.testing.assert_allclose(float(got), float(GL[key]), rtol=2e-6, atol=0, err_msg=key)
    # the unlabelled row counts in L_cr only: the labelled prefix alone gives another total, and the same L_hm + L_2d
    alone, sup2, _ = mixed_loss((maps[:2], coords[:2]), target, joints, GL['img_size'], w[0], w[1], w[2], **kw)
    assert abs(float(alone) - float(GL['total'])) > 1e-3 * float(GL['total'])
    assert float(sup2) == float(sup)
