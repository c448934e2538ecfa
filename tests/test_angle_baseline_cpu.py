"""The angle-regression baselines ('baselinealpha' / 'baselinetheta'), host side: the metric, the criteria, the sample
front end's angle targets and the trainer's criterion mapping against the reference's own values
(tests/golden/angle_baseline.npz, make_golden_angle.py).  No GPU."""
import logging

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import golden
from egonet_amd import configs, synth, trainer
from egonet_amd.common import pose_annot
from egonet_amd.common import train_samples as ts
from egonet_amd.loss import function as loss_func
from egonet_amd.metric import criterions as mc
from egonet_amd.model.heatmapModel import hrnet

G = golden('angle_baseline.npz')
NB = len(G['ns'])


def _cfgs(**top):
    """The YAML keys the sample builder reads (KITTI_train_IGRs.yml), at a small size."""
    return dict({'train': True,
                 'dataset': {'pth_transform': {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}},
                 'heatmapModel': {'add_xy': False, 'jitter_bbox': True,
                                  'jitter_params': {'shift': [0.1, 0.1], 'scaling': [0.4, 0.4]},
                                  'input_size': [64, 64], 'heatmap_size': [16, 16], 'num_joints': 33,
                                  'target_type': 'gaussian', 'sigma': 1}}, **top)


class _Last(logging.Handler):
    def emit(self, record):
        self.text = record.getMessage()


def test_fixture_holds_what_the_kernel_test_needs():
    assert list(G['ns']) == [1, 3, 257]
    for b in range(1, NB):
        d = np.abs(G['gt%d' % b] - np.arctan2(G['pred%d' % b][:, 1].astype(np.float64),
                                              G['pred%d' % b][:, 0].astype(np.float64))) * 180 / np.pi
        assert (d > 180).any() and (d < 180).any() and np.abs(d - 180).min() >= 1e-3


@pytest.mark.parametrize('as_tensor', [False, True])
def test_host_angle_error_and_running_mean_equal_the_reference(as_tensor):
    metric = mc.AngleError(None)
    for b in range(NB):
        pred = torch.from_numpy(G['pred%d' % b]) if as_tensor else G['pred%d' % b]
        meta = {'angles_gt': G['gt%d' % b]}
        avg, cnt, others = mc.get_angle_error(pred, meta)
        assert (avg, cnt, others) == (G['err%d' % b][0], int(G['err%d' % b][1]), None)
        metric.update(pred, meta)
        assert (metric.mean, metric.count) == (G['running%d' % b][0], int(G['running%d' % b][1]))
    log = logging.getLogger('egonet_amd.test_angle_cpu')
    log.setLevel(logging.INFO)
    last = _Last()
    log.handlers = [last]
    metric.report(log)
    assert last.text == str(G['report']) and metric.name == 'Angle error in degrees'


def test_criteria_equal_the_reference():
    for b in range(NB):
        p, t = torch.from_numpy(G['pred%d' % b]), torch.from_numpy(G['tgt%d' % b])
        assert float(loss_func.MSELoss1D()(p, t, torch.ones(1), {})) == float(G['mse%d' % b])
        assert float(loss_func.SmoothL1Loss1D()(p, t, torch.ones(1), {})) == float(G['sl1%d' % b])
    assert float(loss_func.MSELoss1D(use_target_weight=True, reduction='sum')(p, t)) == \
        float(nn.MSELoss(reduction='sum')(p, t))
    assert loss_func.SmoothL1Loss1D(True).use_target_weight is True


def test_pose_frames_returns_rots(tmp_path):
    from PIL import Image
    paths = []
    for f in range(2):
        paths.append(str(tmp_path / ('%d.png' % f)))
        Image.fromarray(np.zeros((8, 12, 3), dtype=np.uint8)).save(paths[-1])
    rots = G['rots']
    annot = {'paths': paths, 'boxes': [np.zeros((2, 4)), np.zeros((3, 4))],
             'kpts': [np.zeros((2, 33, 2)), np.zeros((3, 33, 2))], 'rots': [rots[:2], rots[2:]]}
    frames = pose_annot.PoseFrames(annot)
    rec = frames[1]
    assert np.array_equal(rec['rots'], rots[2:]) and rec['image'].shape == (8, 12, 3)
    assert set(rec) == {'image', 'boxes', 'joints', 'path', 'rots'}
    del annot['rots']                                   # annotations without angles: the records of before
    assert set(pose_annot.PoseFrames(annot)[0]) == {'image', 'boxes', 'joints', 'path'}
    with pytest.raises(ValueError):
        pose_annot.PoseFrames(dict(annot, rots=[rots]))


def _records(n_frames, per_frame, seed=4):
    recs = synth.synth_frame_records(n_frames, per_frame, 33, seed=seed, hw=(96, 128))
    rng = np.random.RandomState(seed)
    for r in recs:
        r['rots'] = rng.uniform(-np.pi, np.pi, (per_frame, 2))
    return recs


@pytest.mark.parametrize('target,exp', [('alpha', 'baselinealpha'), ('theta', 'baselinetheta')])
def test_plan_targets_equal_the_reference(target, exp):
    rots = G['rots']
    recs = synth.synth_frame_records(1, len(rots), 33, seed=1, hw=(96, 128))
    recs[0]['rots'] = rots
    cfgs = _cfgs()
    for b in (ts.TrainSampleBuilder(cfgs, device='cpu', target=target),
              ts.TrainSampleBuilder(dict(cfgs, exp_type=exp), device='cpu')):
        assert b.target == target
        p = b.plan(recs, np.random.RandomState(0))
        assert p['targets'].dtype == np.float32 and np.array_equal(p['targets'], G[exp + '_targets'])
        assert p['meta']['angles_gt'].dtype == np.float64
        assert np.array_equal(p['meta']['angles_gt'], G[exp + '_angles_gt'])


@pytest.mark.parametrize('n_frames,per_frame', [(2, 3), (3, 50)])           # 150 boxes: length_limit chooses 140
def test_plan_keeps_the_heatmap_modes_subset_and_the_default_is_unchanged(n_frames, per_frame):
    recs = _records(n_frames, per_frame)
    cfgs = _cfgs()
    plans = {}
    for target in (None, 'heatmap', 'alpha', 'theta'):
        b = ts.TrainSampleBuilder(cfgs, device='cpu') if target is None else \
            ts.TrainSampleBuilder(cfgs, device='cpu', target=target)
        plans[target] = b.plan(recs, np.random.RandomState(5))
    base = plans[None]
    assert ts.TrainSampleBuilder(dict(cfgs, exp_type='instanceto2d'), device='cpu').target == 'heatmap'
    assert len(base['kept']) == min(n_frames * per_frame, ts.MAX_INS_CNT)
    assert set(base) == {'kept', 'frame', 'trans', 'draws', 'meta'} == set(plans['heatmap'])
    assert set(base['meta']) == {'path', 'original_joints', 'transformed_joints', 'center', 'scale', 'joints_vis'}
    all_rots = np.concatenate([r['rots'] for r in recs])
    for target, col in (('heatmap', None), ('alpha', 0), ('theta', 1)):
        p = plans[target]
        for key in ('kept', 'frame', 'trans', 'draws'):
            assert np.array_equal(p[key], base[key]), (target, key)
        for key in base['meta']:
            assert np.array_equal(p['meta'][key], base['meta'][key]) if key != 'path' else \
                p['meta'][key] == base['meta'][key], (target, key)
        if col is not None:                                 # targets and angles_gt follow ``kept``
            want = all_rots[base['kept'], col]
            assert np.array_equal(p['meta']['angles_gt'], want)
            assert np.array_equal(p['targets'], np.stack([np.cos(want), np.sin(want)], axis=1).astype(np.float32))


def test_angle_mode_needs_rots_and_a_known_target():
    recs = synth.synth_frame_records(1, 2, 33, seed=1, hw=(96, 128))
    with pytest.raises(ValueError, match='rots'):
        ts.TrainSampleBuilder(_cfgs(), device='cpu', target='alpha').plan(recs)
    with pytest.raises(ValueError, match='target'):
        ts.TrainSampleBuilder(_cfgs(), device='cpu', target='beta')


def test_make_step_reads_the_angle_criterion_by_name():
    class MSELoss1D(object):                                # the reference's own class: only the name is read
        pass
    hm = {'heatmapModel': {'loss_type': 'SmoothL1Loss1D'}}
    assert trainer._angle_type(loss_func.MSELoss1D(), hm) == 'mse'              # the object wins over the config
    assert trainer._angle_type(MSELoss1D(), {}) == 'mse'
    assert trainer._angle_type(nn.MSELoss(), {}) == 'mse'
    assert trainer._angle_type(loss_func.SmoothL1Loss1D(), {}) == 'sl1'
    assert trainer._angle_type(nn.SmoothL1Loss(), {}) == 'sl1'
    assert trainer._angle_type(None, hm) == 'sl1'
    assert trainer._angle_type(nn.L1Loss(), {'heatmapModel': {'loss_type': 'MSELoss1D'}}) == 'mse'
    with pytest.raises(NotImplementedError, match='mean'):
        trainer._angle_type(loss_func.MSELoss1D(reduction='sum'), {})


def test_make_step_refuses_an_angle_head_without_a_criterion():
    cfg = configs.tiny_config('angleregression', input_size=(256, 256))
    net = hrnet.get_pose_net(cfg, is_train=False)
    cfg = dict(cfg, optimizer={'lr': 1e-3})
    for lf, hm in ((None, {}), (nn.L1Loss(), {'loss_type': 'JointsCompositeLoss'})):
        cfg['heatmapModel'] = dict(cfg['heatmapModel'], **hm)
        with pytest.raises(NotImplementedError, match=r'function\.py:204-228'):
            trainer.make_step(net, cfg, lf, None)
