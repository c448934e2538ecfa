"""The angle-regression baselines ('baselinealpha' / 'baselinetheta') on the device: the metric kernel
(csrc/angle_metrics.hip) against the reference's values (tests/golden/angle_baseline.npz) and a float64 restatement,
the native step of the angle head against a float64 CPU forward / backward of the same module graph and against the
autograd bridge, the meter inside ``trainer.train`` / ``trainer.evaluate``, the sample front end's angle modes and
tools/train_IGRs.py.  The net is the tiny angle config of test_gpu_train_heads.py (256 x 256 crops: the head pools a
4 x 4 map behind four stride-2 blocks).

Bounds.  Kernel against the reference: 1e-4 degrees on the mean -- the reference takes atan2 in float32, the kernel in
float64; one or two float32 ulps at pi are <= 5e-7 rad = 3e-5 degrees per row.  Kernel against float64 numpy: 1e-12
relative (two libm-grade atan2 and a sum of at most 261 terms).  Step: the bounds of the pixel-shuffle step in
test_gpu_train_heads.py (loss 2e-5 relative, cos > 0.9999, gl2 < 1e-2, med < 5e-3)."""
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import golden
from egonet_amd import _lib, configs, synth, trainer
from egonet_amd.common import train_samples as ts
from egonet_amd.loss import function as loss_function
from egonet_amd.metric import criterions as mc
from egonet_amd.model.heatmapModel import hrnet as hip_hrnet
from egonet_amd.train_hrnet import HRNetTrainStep
from train_checks import gradient_agreement

pytestmark = pytest.mark.gpu
G = golden('angle_baseline.npz')
NB = len(G['ns'])
NOISE = ('final_fc.0.bias',)          # a bias in front of BatchNorm: its gradient is rounding noise (test_gpu_train_heads.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _no_autotune(monkeypatch):
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')


def _cfg():
    return configs.tiny_config('angleregression', input_size=(256, 256))


def _net(seed):
    net = hip_hrnet.get_pose_net(_cfg(), is_train=False)
    sd = synth.synth_state_dict(net.state_dict(), seed=seed)
    net.load_state_dict(sd)
    return net.cuda().train(), sd


def _errors64(pred, gt):
    d = np.abs(gt - np.arctan2(pred[:, 1].astype(np.float64), pred[:, 0].astype(np.float64))) * 180 / np.pi
    return np.where(d > 180, 360 - d, d)


# ---- 1. the kernel ----------------------------------------------------------------------------------------------
def _run_kernel(ld):
    """The three fixture batches folded into one accumulator -> its two float64 on the host."""
    L, st = _lib.lib(), _lib.current_stream()
    acc = torch.full((2,), 7.0, dtype=torch.float64, device='cuda')
    assert L.egn_angle_metrics_reset(_lib.ptr(acc), st) == 0
    assert acc.cpu().tolist() == [0.0, 0.0]
    for b in range(NB):
        pred = G['pred%d' % b]
        n = len(pred)
        rows = torch.full((n, ld), float('nan'), dtype=torch.float32)
        rows[:, :2] = torch.from_numpy(pred)
        rows, gt = rows.cuda(), torch.from_numpy(G['gt%d' % b]).cuda()
        nb = L.egn_angle_metrics_ws_bytes(n)
        assert nb == 16 * ((n + 255) // 256)
        ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
        c0 = L.egn_launch_count()
        assert L.egn_angle_metrics_update_f32(_lib.ptr(rows), n, ld, _lib.ptr(gt), _lib.ptr(ws), nb, _lib.ptr(acc), st) == 0
        assert L.egn_launch_count() - c0 == 2               # rows + fold
    return acc


@pytest.mark.parametrize('ld', [2, 4])
def test_kernel_vs_reference_and_float64(ld):
    L, st = _lib.lib(), _lib.current_stream()
    acc = _run_kernel(ld)
    got = acc.cpu().numpy()
    want_mean, want_cnt = G['running%d' % (NB - 1)]
    assert got[0] == want_cnt == sum(G['ns'])
    print('mean error: kernel %.12f, reference %.12f' % (got[1] / got[0], want_mean))
    assert abs(got[1] / got[0] - want_mean) < 1e-4
    s64 = sum(_errors64(G['pred%d' % b], G['gt%d' % b]).sum() for b in range(NB))
    assert abs(got[1] - s64) < 1e-12 * s64, (got[1], s64)
    assert _run_kernel(ld).cpu().numpy().tobytes() == got.tobytes()            # equal inputs, equal bits
    # N = 0: no launch, nothing changes (the pointers are not read)
    c0 = L.egn_launch_count()
    assert L.egn_angle_metrics_update_f32(None, 0, ld, None, None, 0, _lib.ptr(acc), st) == 0
    assert L.egn_launch_count() == c0 and acc.cpu().numpy().tobytes() == got.tobytes()
    assert L.egn_angle_metrics_reset(_lib.ptr(acc), st) == 0
    assert acc.cpu().tolist() == [0.0, 0.0]


def test_kernel_refuses_bad_arguments():
    L, st = _lib.lib(), _lib.current_stream()
    acc = torch.zeros(2, dtype=torch.float64, device='cuda')
    rows = torch.zeros(3, 2, device='cuda')
    gt = torch.zeros(3, dtype=torch.float64, device='cuda')
    ws = torch.zeros(16, dtype=torch.uint8, device='cuda')
    p = _lib.ptr
    c0 = L.egn_launch_count()
    assert L.egn_angle_metrics_update_f32(p(rows), 3, 1, p(gt), p(ws), 16, p(acc), st) == -1        # ld < 2
    assert L.egn_angle_metrics_update_f32(p(rows), 3, 2, p(gt), p(ws), 8, p(acc), st) == -1         # a short workspace
    assert L.egn_angle_metrics_update_f32(p(rows), 3, 2, None, p(ws), 16, p(acc), st) == -1
    assert L.egn_angle_metrics_update_f32(p(rows), 3, 2, p(gt), p(ws), 16, None, st) == -1
    assert L.egn_angle_metrics_update_f32(p(rows), -1, 2, p(gt), p(ws), 16, p(acc), st) == -1
    assert L.egn_angle_metrics_ws_bytes(-1) == -1 and L.egn_angle_metrics_reset(None, st) == -1
    assert L.egn_launch_count() == c0


# ---- 2. the native step -----------------------------------------------------------------------------------------
def _cpu64(sd, x, tgt, crit):
    """This package's module graph in float64 on the CPU, train mode -> (loss, gradients, output)."""
    ref = hip_hrnet.get_pose_net(_cfg(), is_train=False)
    ref.load_state_dict(sd)
    ref = ref.double().train()
    out = ref(x.double())
    loss = (F.mse_loss if crit == 'mse' else F.smooth_l1_loss)(out, tgt.double())
    loss.backward()
    return float(loss), {k: p.grad.float() for k, p in ref.named_parameters() if k not in NOISE}, out.detach()


@pytest.fixture(scope='module')
def step_case():
    """Inputs of the step tests and the float64 references, computed once."""
    _, sd = _net(seed=21)
    x = synth.synth_crops(3, 3, 256, 256, seed=30)
    out = _cpu64(sd, x, torch.zeros(3, 2), 'mse')[2]
    gen = torch.Generator().manual_seed(3)
    # differences on both sides of the SmoothL1 knee |d| = 1: 0.3 .. 0.9 and 1.5 .. 2.5 away from the prediction
    off = torch.cat([0.3 + 0.6 * torch.rand(3, 1, generator=gen), -(1.5 + torch.rand(3, 1, generator=gen))], dim=1)
    tgt = (out.float() + off).contiguous()
    d = (out - tgt.double()).abs()
    assert bool((d < 1).any()) and bool((d > 1).any())
    refs = {c: _cpu64(sd, x, tgt, c) for c in ('mse', 'sl1')}
    return sd, x, tgt, refs


@pytest.mark.parametrize('crit', ['mse', 'sl1'])
def test_native_angle_step_vs_float64(step_case, crit):
    sd, x, tgt, refs = step_case
    want_loss, want_grads, want_out = refs[crit]
    net, _ = _net(seed=21)
    tr = HRNetTrainStep(net, lr=1e-3, angle_type=crit)
    loss = float(tr.step(x.cuda(), tgt.cuda(), update=False).item())
    print('%s loss: native %.9f, float64 %.9f' % (crit, loss, want_loss))
    assert abs(loss - want_loss) < 2e-5 * abs(want_loss), (loss, want_loss)
    assert tuple(tr.last_angles.shape) == (3, 2) and tr.last_angles.is_contiguous()
    np.testing.assert_allclose(tr.last_angles.cpu().double().numpy(), want_out.numpy(), rtol=0, atol=2e-4)
    gl2, cos, med = gradient_agreement(dict(net.named_parameters()), want_grads)
    print('%s gradients: gl2 %.3e cos %.8f med %.3e' % (crit, gl2, cos, med))
    assert cos > 0.9999 and gl2 < 1e-2 and med < 5e-3, (gl2, cos, med)


@pytest.mark.parametrize('crit', ['mse', 'sl1'])
def test_two_updates_lower_the_loss_on_a_fixed_batch(step_case, crit):
    _, x, tgt, _ = step_case
    net, _ = _net(seed=21)
    tr = HRNetTrainStep(net, lr=1e-3, angle_type=crit)
    xs, ts_ = x.cuda(), tgt.cuda()
    losses = [float(tr.step(xs, ts_).item()) for _ in range(3)]           # the third reading is after two updates
    assert losses[2] < losses[0], losses
    assert int(net.final_fc[1].num_batches_tracked) == 3


def test_angle_step_refuses_the_other_heads_arguments(step_case):
    _, x, tgt, _ = step_case
    net, _ = _net(seed=21)
    with pytest.raises(NotImplementedError, match='angle_type'):
        HRNetTrainStep(net, lr=1e-3)
    with pytest.raises(NotImplementedError):
        HRNetTrainStep(net, lr=1e-3, angle_type='l1')
    for kw in (dict(w_hm=2.0), dict(w_coor=0.0), dict(w_cr=0.01), dict(hm_type='l1')):
        with pytest.raises(ValueError, match=list(kw)[0]):
            HRNetTrainStep(net, lr=1e-3, angle_type='mse', **kw)
    tr = HRNetTrainStep(net, lr=1e-3, angle_type='mse')
    with pytest.raises(ValueError, match='joints_xy'):
        tr.step(x.cuda(), tgt.cuda(), torch.zeros(3, 5, 2))
    with pytest.raises(ValueError, match='target must be'):
        tr.step(x.cuda(), torch.zeros(3, 5, 64, 64).cuda())
    hm_net = hip_hrnet.get_pose_net(configs.tiny_config('heatmap'), is_train=False).cuda().train()
    with pytest.raises(ValueError, match='angle_type'):
        HRNetTrainStep(hm_net, lr=1e-3, w_coor=0.0, angle_type='mse')


# ---- 3. the bridge ----------------------------------------------------------------------------------------------
def test_bridge_and_native_step_agree(step_case):
    _, x, tgt, refs = step_case
    net, _ = _net(seed=21)
    loss = nn.MSELoss()(net(x.cuda()), tgt.cuda())
    assert loss.grad_fn is not None
    loss.backward()
    bridge = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if k not in NOISE}
    net2, _ = _net(seed=21)
    tr = HRNetTrainStep(net2, lr=1e-3, angle_type='mse')
    native = float(tr.step(x.cuda(), tgt.cuda(), update=False).item())
    assert abs(native - float(loss.item())) < 2e-5 * abs(native), (native, float(loss.item()))
    gl2, cos, med = gradient_agreement(dict(net2.named_parameters()), bridge)
    print('native vs bridge: gl2 %.3e cos %.8f med %.3e' % (gl2, cos, med))
    assert cos > 0.9999 and gl2 < 1e-2 and med < 5e-3, (gl2, cos, med)


# ---- 4. meter, trainer, evaluator -------------------------------------------------------------------------------
class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _logger(name):
    lg = logging.getLogger('egonet_amd.test_angle.' + name)
    lg.setLevel(logging.INFO)
    lg.propagate = False
    h = _Lines()
    lg.handlers = [h]
    return lg, h


def test_meter_accumulates_without_a_read_back():
    L = _lib.lib()
    meter = mc.AngleErrorMeter()
    assert meter.read() == (0.0, 0)
    preds = [torch.from_numpy(G['pred%d' % b]).cuda() for b in range(NB)]
    meter.accumulate(preds[0], {'angles_gt': G['gt0']})
    c0 = L.egn_launch_count()
    meter.accumulate(preds[1], {'angles_gt': torch.from_numpy(G['gt1'])})              # a CPU tensor
    meter.accumulate(preds[2], {'angles_gt': torch.from_numpy(G['gt2']).cuda()}, None)  # labels already on the device
    assert L.egn_launch_count() - c0 == 4 and meter._dev.pending      # launches only; nothing was read
    mean, cnt = meter.read()
    assert cnt == int(G['running2'][1]) and meter.read()[1] == cnt    # reading does not clear
    assert abs(mean - G['running2'][0]) < 1e-4
    avg, n, others = meter(preds[2], {'angles_gt': G['gt2']})         # the drop-in call: get_angle_error's return
    assert n == 257 and others is None and abs(avg - G['err2'][0]) < 1e-4
    assert meter.read()[1] == cnt                                     # ... on an accumulator of its own
    meter.reset()
    assert meter.read() == (0.0, 0)
    for _ in range(3):                                                # more turns than pinned buffers
        meter.accumulate(preds[1], {'angles_gt': G['gt1']})
    assert meter.read()[1] == 9
    with pytest.raises(TypeError):
        meter.accumulate(G['pred0'], {'angles_gt': G['gt0']})
    # a padded view of a wider tensor: the row pitch is handed to the kernel
    wide = torch.full((257, 4), float('nan'), device='cuda')
    wide[:, :2] = preds[2]
    avg_w = mc.get_angle_error(wide[:, :2], {'angles_gt': G['gt2']})[0]
    assert avg_w == mc.get_angle_error(preds[2], {'angles_gt': G['gt2']})[0]


def test_angle_error_metric_on_cuda_predictions_reports_like_the_host_path():
    L = _lib.lib()
    dev_m, host_m = mc.AngleError(None), mc.AngleError(None)
    for b in range(NB):
        meta = {'angles_gt': G['gt%d' % b]}
        c0 = L.egn_launch_count()
        dev_m.update(torch.from_numpy(G['pred%d' % b]).cuda(), meta)
        assert L.egn_launch_count() - c0 == 2 + (b == 0) and dev_m._count == 0          # (+ the first reset)
        host_m.update(G['pred%d' % b], meta)
    (lg_d, h_d), (lg_h, h_h) = _logger('dev'), _logger('host')
    dev_m.report(lg_d)
    host_m.report(lg_h)
    assert h_h.lines[0] == str(G['report'])
    head_d, val_d = h_d.lines[0].rstrip('\t').rsplit(' ', 1)
    head_h, val_h = h_h.lines[0].rstrip('\t').rsplit(' ', 1)
    assert head_d == head_h and abs(float(val_d) - float(val_h)) < 1e-4
    assert '%.3f' % float(val_d) == '%.3f' % float(val_h)             # to the precision the 1e-4 bound allows
    assert dev_m.count == host_m.count == 261 and type(dev_m.count) is int
    # a device update merges with a host update of the same object
    dev_m.update(G['pred1'], {'angles_gt': G['gt1']})
    host_m.update(G['pred1'], {'angles_gt': G['gt1']})
    assert dev_m.count == 264 and abs(dev_m.mean - host_m.mean) < 1e-4


class _AngleSet(torch.utils.data.Dataset):
    """Four frames in the form ``PoseFrames`` yields them (decoded image, boxes, joints, rots, path)."""
    num_joints = 5

    def __init__(self):
        self.recs = synth.synth_frame_records(4, 2, 5, seed=3, hw=(96, 128))
        rng = np.random.RandomState(8)
        for r in self.recs:
            r['rots'] = rng.uniform(-np.pi, np.pi, (2, 2))

    def __len__(self):
        return len(self.recs)

    def __getitem__(self, i):
        return self.recs[i]


def _train_cfg():
    cfg = configs.clone(_cfg())
    cfg.update(use_gpu=True, train=True, exp_type='baselinetheta',
               dataset={'pth_transform': {'mean': [0.485, 0.456, 0.406], 'std': [0.229, 0.224, 0.225]}},
               optimizer={'optim_type': 'adam', 'lr': 1e-3, 'weight_decay': 0.0, 'momentum': 0.9, 'milestones': [3],
                          'gamma': 0.5},
               training_settings={'total_epochs': 1, 'batch_size': 1, 'num_threads': 0, 'shuffle': False,
                                  'report_every': 1, 'eval_during': False, 'plot_loss': False},
               testing_settings={'batch_size': 2, 'num_threads': 0, 'shuffle': False, 'apply_dropout': False,
                                 'unnormalize': False})
    cfg['heatmapModel'].update(jitter_bbox=False, target_type='gaussian', sigma=1, loss_type='MSELoss1D')
    return cfg


class _Spy(mc.AngleErrorMeter):
    """The meter of the run, keeping what it was handed for the host restatement."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def accumulate(self, prediction, meta, cfgs=None):
        self.seen.append((prediction.detach().clone(), np.array(meta['angles_gt'])))
        super().accumulate(prediction, meta, cfgs)

    def reset(self):
        self.seen = []
        super().reset()


def test_trainer_train_and_evaluate_on_an_angle_config():
    cfg = _train_cfg()
    net, _ = _net(seed=9)
    optim, sche = trainer.prepare_optim(net, cfg)
    step = trainer.make_step(net, cfg, loss_function.SmoothL1Loss1D(), optim)
    assert isinstance(step, HRNetTrainStep) and step.angle_crit == HRNetTrainStep.CR_CRITERIA['sl1']
    assert trainer.make_step(net, cfg, None, optim).angle_crit == HRNetTrainStep.CR_CRITERIA['mse']   # loss_type
    lg, lines = _logger('train')
    meter = _Spy()
    data = _AngleSet()
    rec = trainer.train(data, net, loss_function.MSELoss1D(), optim, None, cfg, lg, metric_func=meter,
                        collate_fn=ts.collate_frames, sample_builder=ts.TrainSampleBuilder(cfg, split='train'))
    assert len(rec['loss']) == 4 and all(np.isfinite(rec['loss']))
    assert int(net.final_fc[1].num_batches_tracked) == 4 and len(meter.seen) == 4
    mean, cnt = meter.read()
    host = [mc.get_angle_error(p.cpu().numpy(), {'angles_gt': g}) for p, g in meter.seen]
    want = sum(a * n for a, n, _ in host) / sum(n for _, n, _ in host)
    assert cnt == 8 and abs(mean - want) < 1e-4, (mean, want)
    assert any('metric' in ln and 'running mean over 8' in ln for ln in lines.lines)

    # validation: Evaluator(['AngleError']) on CUDA predictions against the host path on the same predictions
    builder = ts.TrainSampleBuilder(cfg, split='valid', target='theta')
    evaluator = mc.Evaluator(['AngleError'], cfg)
    lg, lines = _logger('eval')
    val = trainer.evaluate(data, net, loss_function.MSELoss1D(), cfg, lg, evaluator,
                           collate_fn=lambda b: builder(ts.collate_frames(b)))
    assert val is not None and np.isfinite(val) and not net.training
    host_m = mc.AngleError(cfg)
    for i in range(0, 4, 2):
        x, _, _, meta = builder(data.recs[i:i + 2])
        host_m.update(net(x).detach().cpu().numpy(), meta)
    assert evaluator.metrics[0].count == host_m.count == 8
    got = float(lines.lines[0].rstrip('\t').rsplit(' ', 1)[1])
    assert lines.lines[0].startswith('Error type: Angle error in degrees\tError: ') and abs(got - host_m.mean) < 1e-4


# ---- 5. the sample front end ------------------------------------------------------------------------------------
def test_builder_angle_modes_on_the_device():
    L = _lib.lib()
    cfg = _train_cfg()
    cfg['heatmapModel'].update(jitter_bbox=True, jitter_params={'shift': [0.1, 0.1], 'scaling': [0.4, 0.4]})
    recs = _AngleSet().recs
    out, launches = {}, {}
    for target in ('heatmap', 'alpha', 'theta'):
        b = ts.TrainSampleBuilder(cfg, split='train', target=target)
        plan = b.plan(recs, np.random.RandomState(6))
        c0 = L.egn_launch_count()
        out[target] = b(recs, np.random.RandomState(6))
        launches[target] = L.egn_launch_count() - c0
        images, targets, weights, meta = out[target]
        if target == 'heatmap':
            assert targets.dim() == 4 and targets.shape[:2] == (8, 5) and 'angles_gt' not in meta
            continue
        assert targets.is_cuda and targets.dtype == torch.float32 and tuple(targets.shape) == (8, 2)
        assert np.array_equal(targets.cpu().numpy(), plan['targets'])
        all_rots = np.concatenate([r['rots'] for r in recs])[:, 0 if target == 'alpha' else 1]
        assert meta['angles_gt'].dtype == np.float64 and np.array_equal(meta['angles_gt'], all_rots)
        assert torch.equal(weights, torch.ones(1)) and not weights.is_cuda
        assert torch.equal(images, out['heatmap'][0])                 # the same crops, bit for bit
    assert launches['alpha'] == launches['theta'] == launches['heatmap'] - 1, launches


# ---- 6. the tool ------------------------------------------------------------------------------------------------
def test_tool_trains_an_angle_baseline_in_a_child_process(tmp_path):
    from test_gpu_train_igrs_tool import _write_tree
    root, out_dir = str(tmp_path / 'kitti'), str(tmp_path / 'out')
    _write_tree(root)
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'train_IGRs.py'), '--kitti', root, '--out', out_dir, '--tiny',
           '--max-steps', '3', '--exp-type', 'baselinetheta', '--loss-type', 'SmoothL1Loss1D', '--batch-frames', '3',
           '--workers', '0', '--report-every', '1', '--epochs', '3', '--valid-split-file', os.path.join(root, 'val.txt')]
    done = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, EGONET_AMD_AUTOTUNE='0'), stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:]
    out = json.loads(done.stdout.strip().splitlines()[-1])
    assert out['steps'] == 3 and np.isfinite(out['last_loss'])
    assert out['out'] == os.path.join(out_dir, 'baselinetheta.pth')
    assert out['eval']['metric'] == 'AngleError' and 0.0 <= out['eval']['mean'] <= 180.0
    assert out['eval']['count'] == 3                            # the three cars of the two validation frames
    state = torch.load(out['out'])
    assert all(torch.is_tensor(v) and not v.is_cuda for v in state.values())
    net = hip_hrnet.get_pose_net(configs.hrnet_config(8, (256, 256), 33, 'angleregression', modules=(1, 1, 1),
                                                      num_blocks=1), is_train=False)
    net.load_state_dict(state, strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in state.values() if v.is_floating_point())
    assert int(state['final_fc.1.num_batches_tracked']) == 3
