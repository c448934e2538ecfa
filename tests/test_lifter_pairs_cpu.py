"""Lifter pair front end, host side: the numpy restatement (tests/lifter_pairs_ref.py) against the fixture the
reference wrote (tests/golden/lifter_pairs.npz), the parsers, the draw layout, the device loader's index order and
the ``get_loader`` hook.  No device."""
import json

import numpy as np
import pytest
import torch

import lifter_pairs_ref as ref
from conftest import golden
from egonet_amd import trainer
from egonet_amd.common import lifter_pairs as lp

G = golden('lifter_pairs.npz')
CASES = json.loads(str(G['cases']))
COEF = [float(c) for c in G['coef']]
SIZE = tuple(int(v) for v in G['size'])


def case_frames(name):
    """[(labels [n,7], P [3,4] float32, size)] of a case, parsed from the fixture's text."""
    labels = json.loads(str(G[name + '/label_text']))
    calibs = json.loads(str(G[name + '/calib_text']))
    return [(lp.parse_label_text(lt, ('Car',)), lp.parse_calib_text(ct), SIZE) for lt, ct in zip(labels, calibs)]


def case_cfgs(name):
    c = CASES[name]
    return {'dataset': {'3d_kpt_sample_style': 'bbox9', 'detect_classes': ['Car'],
                        'interpolate': {'flag': True, 'style': 'bbox12', 'coef': list(COEF)},
                        'lft_in_rep': 'coordinates2d', 'lft_out_rep': c['out_rep']},
            'training_settings': {'lft_aug': c['lft_aug'], 'lft_aug_times': c['T']}}


def case_records(name):
    return [{'labels': lab, 'P': P, 'size': size, 'path': '%06d.png' % f}
            for f, (lab, P, size) in enumerate(case_frames(name))]


def case_shape(name):
    """(T in effect, whether the split draws) as the reference decides them (car_instance.py:767, 1063)."""
    c = CASES[name]
    train = c['split'] == 'train'
    return (c['T'] if (c['lft_aug'] and train) else 0), train


def case_draws(name):
    """The recorded draws [A, 7T+1] -- the reference's calls in order are one row per label."""
    T, train = case_shape(name)
    if not train:
        return None
    return np.asarray(G[name + '/draws']).reshape(-1, 7 * T + 1)


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_reproduces_the_reference(name):
    """array_equal on the float32 rows: same numpy, same libm as the fixture's generator.  On a platform whose
    cos / sin or matrix product differs in the last float64 bit an element may round the other way; the bar that
    holds everywhere is the GPU test's (1 float32 ulp)."""
    T, train = case_shape(name)
    got = ref.build(case_frames(name), COEF, T, train, CASES[name]['out_rep'], case_draws(name))
    assert np.array_equal(got['keep'], G[name + '/keep'])
    assert np.array_equal(got['input'], G[name + '/input'])
    assert np.array_equal(got['output'], G[name + '/output'])
    if CASES[name]['out_rep'] == 'R3d':
        assert np.array_equal(got['roots'], G[name + '/root_list'])
    src = CASES[name]['statistics_of']
    st = ref.statistics(got['input'], got['output']) if src is None else \
        {k: G[src + '/' + k] for k in ('mean_in', 'std_in', 'mean_out', 'std_out')}
    for k in st:
        assert np.array_equal(st[k], G[name + '/' + k]), k
    assert np.array_equal(ref.normalize(got['input'], st['mean_in'], st['std_in']), G[name + '/input_norm'])
    assert np.array_equal(ref.normalize(got['output'], st['mean_out'], st['std_out']), G[name + '/output_norm'])


def test_fixture_exercises_the_filter_and_negative_depth():
    keep = G['train8/keep']
    assert 0.05 <= 1 - keep.mean() <= 0.5
    got = ref.build(case_frames('train8'), COEF, 8, True, 'R3d+T', case_draws('train8'))
    z = got['output'].reshape(len(got['output']), -1, 3)[:, :, 2]
    assert (z[:, 1:] < 0).any()                                  # points nearer than the root, relative depth < 0
    root_z = got['output'][:, 2]
    assert ((root_z[:, None] + z[:, 1:]) < 0).any(), 'no kept row with a point behind the camera'


def test_parsers_on_the_fixture_text(tmp_path):
    labels = json.loads(str(G['train8/label_text']))
    calibs = json.loads(str(G['train8/calib_text']))
    counts = [len(lp.parse_label_text(t, ('Car',))) for t in labels]
    assert counts == [3, 3, 0, 3, 3, 3, 3]                       # one frame has no Car line
    assert all(len(lp.parse_label_text(t, ('Pedestrian',))) == 1 for t in labels)
    assert all(len(lp.parse_label_text(t, ('Car', 'Pedestrian', 'DontCare'))) == c + 2 for t, c in zip(labels, counts))
    # dimensions are stored h w l and returned l h w; then x y z rot_y
    row = lp.parse_label_text('Car 0.00 0 -1.57 1 2 3 4 1.50 1.60 3.90 -2.00 1.70 20.00 0.30\n', ('Car',))
    assert row.tolist() == [[3.9, 1.5, 1.6, -2.0, 1.7, 20.0, 0.3]]
    p = tmp_path / 'c.txt'
    p.write_text(calibs[0])
    P = lp.read_calib_file(str(p))
    assert P.dtype == np.float32 and P.shape == (3, 4) and abs(P[2, 2] - 1) == 0
    q = tmp_path / 'l.txt'
    q.write_text(labels[0])
    assert np.array_equal(lp.read_label_file(str(q), ('Car',)), lp.parse_label_text(labels[0], ('Car',)))
    fr = lp.frame_row(P, SIZE)
    K = P[:, :3]
    assert np.array_equal(fr[:9], K.astype(np.float64).reshape(-1))
    assert np.array_equal(fr[9:12], (np.linalg.inv(K) @ P[:, 3].reshape(3, 1)).astype(np.float64).reshape(-1))
    assert fr[9:12].astype(np.float32).astype(np.float64).tolist() == fr[9:12].tolist()     # computed in float32
    assert fr[12:].tolist() == [1242.0, 375.0]


def test_offset_quirk_in_the_restatement():
    box = ref.box_3d(3.9, 1.5, 1.6, COEF)
    assert box.shape == (3, 33)
    assert box[0, 0] != 0.0 and abs(box[0, 0] - (0.5 * 3.9 - float(np.float32(3.9)) / 2)) == 0.0
    assert abs(box[0, 0]) < 1e-7


@pytest.mark.parametrize('T', [4, 100])
def test_draw_layout_equals_the_per_call_stream(T):
    """One randn(A, 7T+1) equals the reference's calls: per label randn(T,3), randn(T,3), T+1 single draws."""
    A = 3
    np.random.seed(5)
    calls = []
    for _ in range(A):
        calls += [np.random.randn(T, 3).reshape(-1), np.random.randn(T, 3).reshape(-1)]
        calls += [np.array([np.random.randn()]) for _ in range(T + 1)]
    np.random.seed(5)
    assert np.array_equal(np.random.randn(A, 7 * T + 1).reshape(-1), np.concatenate(calls))


@pytest.mark.parametrize('name', sorted(CASES))
def test_builder_draws_are_the_recorded_ones(name):
    b = lp.LifterPairBuilder(case_cfgs(name), CASES[name]['split'], device='cpu')
    labels, lf, frames = b.gather(case_records(name))
    np.random.seed(CASES[name]['seed'])
    d = b.draw(len(labels))
    want = case_draws(name)
    if want is None:
        assert d is None
    else:
        assert np.array_equal(d, want)
    assert (b.T, b.yaw_draws) == case_shape(name)
    assert lf.dtype == np.int32 and frames.shape == (7 if len(lf) > 3 else 2, 14)
    assert len(G[name + '/keep']) == len(labels) * (b.T + 1)


class _Index(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


@pytest.mark.parametrize('shuffle', [False, True])
@pytest.mark.parametrize('n,bs', [(23, 5), (16, 4), (7, 16)])
def test_epoch_indices_follow_the_dataloader(shuffle, n, bs):
    torch.manual_seed(1234)
    want = [torch.cat([b for b in torch.utils.data.DataLoader(_Index(n), batch_size=bs, shuffle=shuffle)])
            for _ in range(2)]
    after_want = torch.rand(3)
    torch.manual_seed(1234)
    got = [lp.epoch_indices(n, shuffle) for _ in range(2)]
    after_got = torch.rand(3)
    for w, g in zip(want, got):
        assert torch.equal(w, g)
    assert torch.equal(after_want, after_got)                     # the global generator was consumed the same way
    if shuffle and n > 7:
        assert not torch.equal(got[0], got[1])

    class _DS(object):
        def __len__(self):
            return n
    assert len(lp.DeviceLoader(_DS(), bs, shuffle)) == len(torch.utils.data.DataLoader(_Index(n), batch_size=bs))


def test_get_loader_keeps_the_dataloader_for_plain_sets():
    cfgs = {'training_settings': {'batch_size': 4, 'num_threads': 0, 'shuffle': True}}
    loader = trainer.get_loader(_Index(10), cfgs, 'training')
    assert type(loader) is torch.utils.data.DataLoader
    assert loader.batch_size == 4 and isinstance(loader.sampler, torch.utils.data.RandomSampler)

    class _Dev(_Index):
        def device_loader(self, batch_size, shuffle):
            return ('device', batch_size, shuffle)
    assert trainer.get_loader(_Dev(10), cfgs, 'training') == ('device', 4, True)


@pytest.mark.parametrize('section,key,value', [
    ('dataset', '3d_kpt_sample_style', 'bbox27'),
    ('dataset', 'lft_in_rep', 'coordinates2d+area'),
    ('dataset', 'lft_out_rep', 'T'),
    ('dataset', 'interpolate', {'flag': True, 'style': 'bbox12l', 'coef': [0.5]}),
    ('dataset', 'interpolate', {'flag': False, 'style': 'bbox12', 'coef': [0.5]}),
    ('dataset', 'interpolate', {'flag': True, 'style': 'bbox12', 'coef': [0.2, 0.4, 0.6]}),
])
def test_unsupported_configurations_raise(section, key, value):
    cfgs = case_cfgs('train8')
    cfgs[section][key] = value
    with pytest.raises(NotImplementedError, match='car_instance.py'):
        lp.LifterPairBuilder(cfgs, 'train', device='cpu')


def test_builder_refuses_a_frame_index_outside_the_frames():
    b = lp.LifterPairBuilder(case_cfgs('valid'), 'valid', device='cpu')
    labels, lf, frames = b.gather(case_records('valid'))
    for bad in (-1, len(frames)):
        lf2 = lf.copy()
        lf2[0] = bad
        with pytest.raises(ValueError, match='label_frame'):
            b.build(labels, lf2, frames, None)


def test_synth_kitti_labels_are_seeded_records():
    from egonet_amd import synth
    a, b = synth.synth_kitti_labels(10, seed=3), synth.synth_kitti_labels(10, seed=3)
    assert [len(r['labels']) for r in a] == [4, 4, 2]
    assert all(np.array_equal(x['labels'], y['labels']) and np.array_equal(x['P'], y['P']) for x, y in zip(a, b))
    assert a[0]['P'].dtype == np.float32 and a[0]['labels'].shape == (4, 7) and a[0]['size'] == (1242, 375)
