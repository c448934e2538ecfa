"""Mixed batches on the device: labelled crops followed by crops of unlabelled frames (cfgs['ss'],
car_instance.py:1145-1169, 1292-1298, 1344-1391; function.py:170-202).

1. ``TrainSampleBuilder`` against the reference's batch (tests/golden/mixed_samples.npz, case 'mix'): N crops in the
   reference's order from one crop launch, n_fs targets from one target launch;
2. ``HRNetTrainStep.step`` with ``n_fs < N`` against the oracle's forward over all N crops and the loss composition of
   tests/test_mixed_samples_cpu.py (pinned on the reference's JointsCompositeLoss): loss, gradients, BatchNorm
   statistics; the 'coordinates' head with L_cr off and on, and the plain 'heatmap' head;
3. the combinations that are refused;
4. ``trainer.train`` over a ``MixedFrames`` set, and tools/train_IGRs.py with ``--ss-record``.
"""
import logging
import os

import numpy as np
import pytest
import torch

from egonet_amd import _lib, configs, synth, trainer
from egonet_amd.common import crop_gpu, train_samples as ts
from egonet_amd.common.img_proc import get_cr_indices
from egonet_amd.metric.criterions import DistanceSrcMeter
from egonet_amd.model.heatmapModel import hrnet as hip_hrnet
from egonet_amd.train_hrnet import HRNetTrainStep
from oracle import hrnet_oracle
from oracle.hrnet_train_oracle import HRNetTrainOracle
from test_gpu_train_samples import _oracle_crops
from test_mixed_samples_cpu import G, mixed_cfgs, mixed_loss, mixed_pool, mixed_records
from train_checks import gradient_agreement

pytestmark = pytest.mark.gpu
MEAN, STD = crop_gpu.IMAGENET_MEAN, crop_gpu.IMAGENET_STD


@pytest.fixture(autouse=True)
def _no_autotune(monkeypatch):
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')      # cost-model tile choice: keeps the tests short


# ------------------------------------------------------------------------------------------------------------
# 1. the builder
# ------------------------------------------------------------------------------------------------------------
def test_builder_matches_the_reference_mixed_batch():
    recs, c = mixed_records('mix', with_images=True)
    pool = mixed_pool(with_images=True)
    b = ts.TrainSampleBuilder(mixed_cfgs(c), split='train')
    b(recs, np.random.RandomState(0), unlabelled=pool)            # first call: allocations, constants
    torch.cuda.synchronize()
    L = _lib.lib()
    np.random.seed(int(G['mix/np_seed']))
    c0 = L.egn_launch_count()
    images, targets, weights, meta = b(recs, unlabelled=pool)
    assert L.egn_launch_count() - c0 == 2                         # one crop launch over all N, one target launch
    torch.cuda.synchronize()
    kept, n_fs = G['mix/kept'], int(G['mix/n_fs'])
    N = len(kept)
    assert (N, n_fs) == (12, 6) and meta['fs_instance_cnt'] == n_fs
    iw, ih = c['settings']['input_size']
    hw, hh = c['settings']['heatmap_size']
    assert tuple(images.shape) == (N, 3, ih, iw) and images.is_cuda
    assert tuple(targets.shape) == (n_fs, 33, hh, hw) and tuple(weights.shape) == (n_fs, 33, 1)
    for key in ('center', 'scale', 'transformed_joints', 'joints_vis', 'original_joints'):
        assert meta[key].dtype == G['mix/' + key].dtype and len(meta[key]) == n_fs
        np.testing.assert_allclose(meta[key], G['mix/' + key], rtol=0, atol=1e-9, err_msg=key)
    # targets and weights of the labelled prefix: the bounds of tests/test_gpu_train_samples.py
    want_t, want_w = G['mix/targets'], G['mix/target_weights']
    got_t, got_w = targets.cpu().numpy(), weights.cpu().numpy()
    assert np.array_equal(got_w, want_w)
    assert np.array_equal(got_t > 0, want_t > 0)
    np.testing.assert_allclose(got_t, want_t, rtol=0, atol=2e-7)
    # the pixels of all N crops, labelled and unlabelled, in the reference's order: the oracle's warp on the
    # reference's own matrices, bit for bit
    frames = [r['image'] for r in recs] + [r['image'] for r in pool]
    src = G['mix/inst_frame'][kept]
    assert (src[:n_fs] < len(recs)).all() and (src[n_fs:] >= len(recs)).all()
    want = _oracle_crops(frames, src, G['mix/warps'][G['mix/inst_warp'][kept]].reshape(-1, 6), (iw, ih))
    assert np.array_equal(images.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------
# 2. the step
# ------------------------------------------------------------------------------------------------------------
def _tiny_model(cfg, seed):
    net = hip_hrnet.get_pose_net(cfg, is_train=False)
    sd = synth.synth_state_dict(net.state_dict(), seed=seed)
    net.load_state_dict(sd)
    return net.cuda().train(), sd


def _oracle_mixed(sd, cfg, x, tgt, jt, w_coor, cr):
    """Forward over ALL crops (BatchNorm statistics and running buffers over N), the mixed loss, backward.
    Returns (loss, parameter gradients, the oracle's state dict after the forward)."""
    orc = HRNetTrainOracle(sd, cfg, lr=1e-3, w_coor=w_coor)
    out = hrnet_oracle.hrnet_forward_train(orc.sd, cfg, x)
    kw = dict(cr_indices=None, target_cr=4 / 3, cr_loss_thres=0.15)
    kw.update({k: v for k, v in cr.items() if k != 'w_cr'})
    loss = mixed_loss(out, tgt, jt, cfg['heatmapModel']['input_size'], 1.0, w_coor, cr.get('w_cr'), **kw)[0]
    loss.backward()
    return float(loss.detach()), orc.grads(), orc.sd


CR = dict(w_cr=0.05, cr_indices=get_cr_indices(), cr_loss_thres=0.05)


@pytest.mark.parametrize('use_cr', [False, True])
def test_coordinate_head_step_with_a_labelled_prefix_vs_oracle(use_cr):
    cfg = configs.tiny_config('coordinates', num_joints=33)
    net, sd = _tiny_model(cfg, seed=9)
    gen = torch.Generator().manual_seed(4)
    x = synth.synth_crops(3, 3, 64, 64, seed=8)
    tgt = torch.rand(2, 33, 16, 16, generator=gen)
    jt = torch.rand(2, 33, 2, generator=gen) * 64
    cr = CR if use_cr else {}
    want_loss, want_grads, want_sd = _oracle_mixed(sd, cfg, x, tgt, jt, 0.1, cr)
    # the case is live: the labelled crops alone (other BatchNorm statistics, no third row in L_cr) give another loss
    alone = HRNetTrainOracle(sd, cfg, lr=1e-3, cr=cr).step(x[:2], tgt, jt, update=False)[0]
    assert abs(alone - want_loss) > 1e-3 * abs(want_loss), (alone, want_loss)
    if use_cr:
        plain = _oracle_mixed(sd, cfg, x, tgt, jt, 0.1, {})[0]
        assert abs(want_loss - plain) > 1e-3 * abs(plain)                 # and so is the cross-ratio term
    tr = HRNetTrainStep(net, lr=1e-3, w_cr=0.05, cr_loss_thres=0.05)
    tr.apply_cr_loss = use_cr
    loss = float(tr.step(x.cuda(), tgt.cuda(), jt.cuda(), update=False).item())
    gl2, cos, med = gradient_agreement(dict(net.named_parameters()), want_grads)
    print('L_cr %s: loss %.8f (oracle %.8f, rel %.2e), gradients rel-L2 %.2e cosine %.6f median %.2e'
          % ('on' if use_cr else 'off', loss, want_loss, abs(loss - want_loss) / abs(want_loss), gl2, cos, med))
    assert tuple(tr.last_maps.shape) == (3, 33, 16, 16) and tuple(tr.last_coords.shape) == (3, 33, 2)
    assert abs(loss - want_loss) < (2e-3 if use_cr else 2e-5) * abs(want_loss), (loss, want_loss)
    assert cos > 0.9999 and gl2 < 1e-2 and med < 5e-3, (gl2, cos, med)
    # train-mode BatchNorm ran over all 3 crops
    np.testing.assert_allclose(net.state_dict()['bn1.running_mean'].cpu().numpy(),
                               want_sd['bn1.running_mean'].detach().numpy(), rtol=1e-3, atol=1e-5)
    two = HRNetTrainOracle(sd, cfg, lr=1e-3)
    two.step(x[:2], tgt, jt, update=False)
    assert not np.allclose(two.sd['bn1.running_mean'].detach().numpy(), want_sd['bn1.running_mean'].detach().numpy(),
                           rtol=1e-3, atol=1e-5)


def test_all_labelled_batch_is_unchanged_by_the_prefix_path():
    """n_fs == N: the same launches as before -- the loss equals the oracle's plain composite loss under the bounds of
    test_cross_ratio_term_in_the_step_vs_oracle, and the launch count does not depend on the path taken."""
    cfg = configs.tiny_config('coordinates', num_joints=33)
    gen = torch.Generator().manual_seed(4)
    x = synth.synth_crops(3, 3, 64, 64, seed=8)
    tgt = torch.rand(3, 33, 16, 16, generator=gen)
    jt = torch.rand(3, 33, 2, generator=gen) * 64
    net, sd = _tiny_model(cfg, seed=9)
    want = HRNetTrainOracle(sd, cfg, lr=1e-3, cr=CR).step(x, tgt, jt, update=False)[0]
    tr = HRNetTrainStep(net, lr=1e-3, w_cr=0.05, cr_loss_thres=0.05)
    tr.apply_cr_loss = True
    L = _lib.lib()
    tr.step(x.cuda(), tgt.cuda(), jt.cuda(), update=False)
    c0 = L.egn_launch_count()
    loss = float(tr.step(x.cuda(), tgt.cuda(), jt.cuda(), update=False).item())
    full = L.egn_launch_count() - c0
    assert abs(loss - want) < 2e-3 * abs(want), (loss, want)
    c0 = L.egn_launch_count()
    tr.step(x.cuda(), tgt[:2].cuda(), jt[:2].cuda(), update=False)
    assert L.egn_launch_count() - c0 == full                     # the prefix changes arguments, not launches


def test_heatmap_head_step_with_a_labelled_prefix_vs_oracle():
    cfg = configs.tiny_config('heatmap')
    net, sd = _tiny_model(cfg, seed=5)
    gen = torch.Generator().manual_seed(1)
    x = synth.synth_crops(3, 3, 64, 64, seed=2)
    tgt = torch.rand(2, 5, 16, 16, generator=gen)
    want_loss, want_grads, want_sd = _oracle_mixed(sd, cfg, x, tgt, None, 0.0, {})
    alone = HRNetTrainOracle(sd, cfg, lr=1e-3, w_coor=0.0).step(x[:2], tgt, None, update=False)[0]
    assert abs(alone - want_loss) > 1e-3 * abs(want_loss), (alone, want_loss)
    tr = HRNetTrainStep(net, lr=1e-3, w_coor=0.0)
    loss = float(tr.step(x.cuda(), tgt.cuda(), None, update=False).item())
    gl2, cos, med = gradient_agreement(dict(net.named_parameters()), want_grads)
    print('heat-map head: loss %.8f (oracle %.8f, rel %.2e), gradients rel-L2 %.2e cosine %.6f median %.2e'
          % (loss, want_loss, abs(loss - want_loss) / abs(want_loss), gl2, cos, med))
    assert tuple(tr.last_maps.shape) == (3, 5, 16, 16)
    assert abs(loss - want_loss) < 2e-5 * abs(want_loss), (loss, want_loss)
    assert cos > 0.9999 and gl2 < 1e-2 and med < 5e-3, (gl2, cos, med)
    np.testing.assert_allclose(net.state_dict()['bn1.running_mean'].cpu().numpy(),
                               want_sd['bn1.running_mean'].detach().numpy(), rtol=1e-3, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------
# 3. the refusals
# ------------------------------------------------------------------------------------------------------------
def test_prefix_batches_are_refused_where_the_reference_has_no_slice():
    x = synth.synth_crops(3, 3, 64, 64, seed=2).cuda()
    gen = torch.Generator().manual_seed(1)
    tgt = torch.rand(2, 5, 16, 16, generator=gen).cuda()
    jt = (torch.rand(2, 5, 2, generator=gen) * 64).cuda()
    # JointsMSELoss(use_target_weight=True)
    net, _ = _tiny_model(configs.tiny_config('heatmap'), seed=5)
    tr = HRNetTrainStep(net, lr=1e-3, w_coor=0.0, use_target_weight=True)
    with pytest.raises(ValueError, match='labelled prefix.*use_target_weight'):
        tr.step(x, tgt, None, update=False, target_weight=torch.ones(2, 5, 1))
    # the pixel-shuffle head
    cfg = configs.tiny_config('heatmap')
    cfg['heatmapModel']['pixel_shuffle'] = True
    cfg['heatmapModel']['heatmap_size'] = [32, 32]
    net, _ = _tiny_model(cfg, seed=5)
    with pytest.raises(ValueError, match='labelled prefix.*pixel-shuffle head'):
        HRNetTrainStep(net, lr=1e-3, w_coor=0.0).step(x, torch.rand(2, 5, 32, 32).cuda(), None, update=False)
    # the angle head
    net, _ = _tiny_model(configs.tiny_config('angleregression', input_size=(256, 256)), seed=5)
    with pytest.raises(ValueError, match='labelled prefix.*angle head'):
        HRNetTrainStep(net, lr=1e-3, angle_type='mse').step(torch.zeros(3, 3, 256, 256).cuda(),
                                                            torch.rand(2, 2).cuda(), update=False)
    # device-drawn targets, and a captured graph
    net, _ = _tiny_model(configs.tiny_config('coordinates'), seed=9)
    tr = HRNetTrainStep(net, lr=1e-3)
    with pytest.raises(ValueError, match='labelled prefix.*device-drawn targets'):
        tr.step(x, None, jt, update=False)
    from egonet_amd.graph import GraphedStep
    with pytest.raises(ValueError, match='GraphedStep with a labelled prefix'):
        GraphedStep(tr, x, tgt, jt)
    with pytest.raises(ValueError, match='target has 4 rows for 3 images'):
        tr.step(x, torch.rand(4, 5, 16, 16).cuda(), jt, update=False)
    with pytest.raises(ValueError, match='joints_xy must be'):
        tr.step(x, tgt, torch.rand(3, 5, 2).cuda() * 64, update=False)
    # nothing above ran a step: the refused calls left the weights alone, and a good call still works
    assert np.isfinite(float(tr.step(x, tgt, jt, update=False).item()))


# ------------------------------------------------------------------------------------------------------------
# 4. trainer.train and the tool
# ------------------------------------------------------------------------------------------------------------
class _Frames(torch.utils.data.Dataset):
    """Records whose frames are decoded in __getitem__ (PNG files)."""
    num_joints = 33

    def __init__(self, records, root):
        from PIL import Image
        self.items = []
        os.makedirs(root)
        for i, r in enumerate(records):
            path = os.path.join(root, 'f%03d.png' % i)
            Image.fromarray(r['image']).save(path)
            self.items.append({'path': path, 'boxes': r['boxes'], 'joints': r['joints']})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return dict(self.items[i], image=crop_gpu.load_rgb(self.items[i]['path']))


def _write_unlabelled(root, n=3, boxes=3, hw=(70, 110), seed=61):
    """An unlabelled record (the reference's dictionary, as its .npy file) and its images under ``root``."""
    from PIL import Image
    os.makedirs(root)
    recs = synth.synth_frame_records(n, boxes, 33, seed=seed, hw=hw)
    paths = []
    for i, r in enumerate(recs):
        name = 'u%03d.png' % i
        Image.fromarray(r['image']).save(os.path.join(root, name))
        paths.append(os.path.join('somewhere', 'else', name))
    npy = os.path.join(root, 'ss_record.npy')
    np.save(npy, np.array({'paths': paths, 'boxes': [r['boxes'] for r in recs],
                           'kpts': [r['joints'] for r in recs]}, dtype=object))
    return npy


def test_trainer_train_over_mixed_frames(tmp_path, monkeypatch):
    per = [2, 1, 3, 2]
    records = [dict(r, boxes=r['boxes'][:n], joints=r['joints'][:n])
               for r, n in zip(synth.synth_frame_records(4, 3, 33, seed=12, hw=(96, 160)), per)]
    npy = _write_unlabelled(str(tmp_path / 'unlabelled'))
    cfg = configs.tiny_config('coordinates', num_joints=33)
    cfg['heatmapModel'].update(jitter_bbox=True, jitter_params={'shift': [0.1, 0.1], 'scaling': [0.4, 0.4]},
                               sigma=1, target_type='gaussian', loss_spec_list=['mse', 'l1', 'sl1'],
                               loss_weight_list=[1.0, 0.1, 0.05], cr_loss_threshold=0.05)
    cfg.update(train=True, use_gpu=True, exp_type='test',
               dataset={'pth_transform': {'mean': list(MEAN), 'std': list(STD)}},
               ss={'flag': True, 'max_per_img': 3},
               optimizer={'optim_type': 'adam', 'lr': 1e-3, 'weight_decay': 0.0, 'momentum': 0.9,
                          'milestones': [3], 'gamma': 0.5},
               training_settings={'total_epochs': 2, 'batch_size': 2, 'num_threads': 0, 'shuffle': False,
                                  'report_every': 1, 'eval_during': False, 'plot_loss': False})
    ds = ts.MixedFrames(_Frames(records, str(tmp_path / 'frames')), npy, str(tmp_path / 'unlabelled'), 3)
    net, _ = _tiny_model(cfg, seed=31)
    steps, seen = [], []
    make_step = trainer.make_step
    monkeypatch.setattr(trainer, 'make_step', lambda *a, **k: steps.append(make_step(*a, **k)) or steps[-1])
    builder = ts.TrainSampleBuilder(cfg)

    def spy(batch):
        out = builder(batch)
        seen.append((len(out[0]), len(out[1]), int(np.count_nonzero(out[3]['original_joints'][:, :, 2])),
                     steps[0].apply_cr_loss))
        return out
    optim, _ = trainer.prepare_optim(net, cfg)
    lg = logging.getLogger('egonet_amd.test_mixed_batches')
    lg.handlers = [logging.NullHandler()]
    meter = DistanceSrcMeter(cfg)
    np.random.seed(5)
    record = trainer.train(ds, net, None, optim, None, cfg, lg, metric_func=meter, collate_fn=ts.collate_frames,
                           sample_builder=spy)
    assert len(record['loss']) == 4 and all(np.isfinite(record['loss']))
    # frames with 2, 1, 3, 2 cars and up to 3 crops per frame: 1 + 2 unlabelled crops in the first batch, 0 + 1 in
    # the second; targets for the labelled ones only
    assert [(n, n_fs) for n, n_fs, _, _ in seen] == [(6, 3), (6, 5)] * 2
    assert [on for _, _, _, on in seen] == [False, False, True, True]     # L_cr from the second epoch on
    assert steps[0].w_cr == 0.05
    # the meter (reset at the start of an epoch) counted the visible LABELLED joints of the last epoch
    count = meter.read()[1]
    assert count == sum(v for _, _, v, _ in seen[2:]) and 0 < count < (3 + 5) * 33


def test_tool_trains_on_mixed_batches(tmp_path, monkeypatch, capsys):
    from test_gpu_train_igrs_tool import _write_tree
    from tools import train_IGRs as tool
    root, out_dir, ss_root = str(tmp_path / 'kitti'), str(tmp_path / 'out'), str(tmp_path / 'unlabelled')
    _write_tree(root)
    npy = _write_unlabelled(ss_root, hw=(48, 64))
    common = ['--kitti', root, '--out', out_dir, '--tiny', '--seed', '0', '--batch-frames', '2', '--workers', '0',
              '--report-every', '1', '--epochs', '2', '--max-steps', '3']
    mixed = ['--ss-record', npy, '--ss-img-root', ss_root, '--ss-max-per-img', '4']
    with pytest.raises(SystemExit):
        tool.main(common + mixed)                                 # the cross-ratio weight is off
    assert 'unlabelled crops then only change BatchNorm statistics' in capsys.readouterr().err
    assert not os.path.exists(os.path.join(out_dir, 'HC.pth'))
    shapes = []
    call = ts.TrainSampleBuilder.__call__

    def spy(self, *a, **k):
        out = call(self, *a, **k)
        shapes.append((len(out[0]), len(out[1])))
        return out
    monkeypatch.setattr(ts.TrainSampleBuilder, '__call__', spy)
    out = tool.main(common + mixed + ['--cr-weight', '0.05'])
    assert out['steps'] == 3 and np.isfinite(out['last_loss'])
    assert out['out'] == os.path.join(out_dir, 'HC.pth')
    # 5 cars over 3 frames, up to 4 crops per frame: every batch is mixed
    assert len(shapes) == 3 and all(n > n_fs > 0 for n, n_fs in shapes), shapes
    assert sum(n_fs for _, n_fs in shapes[:2]) == 5
    state = torch.load(out['out'])
    import argparse
    cfgs = tool.igr_cfgs(argparse.Namespace(tiny=True, lr=1e-3, epochs=1, batch_frames=2, workers=0, report_every=1,
                                            eval_every=0))
    net = hip_hrnet.get_pose_net(cfgs, is_train=False)
    net.load_state_dict(state, strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in state.values() if v.is_floating_point())
