"""The lifter's 3-D validation metrics on the device (csrc/lifter_metrics.hip through egonet_amd.metric.criterions):
per-row columns against the float64 restatement of the reference (tests/lifter_metrics_ref.py), the accumulator's
bookkeeping, the reference's recorded attributes (tests/golden/lifter_metrics.npz), and the trainer / tool wiring."""
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden, ROOT
from egonet_amd import _lib, configs, synth, trainer
from egonet_amd.common import lifter_pairs as lp
from egonet_amd.metric import criterions as cr
from egonet_amd.model import FCmodel
import lifter_metrics_ref as ref

pytestmark = pytest.mark.gpu

LAYOUTS = ('R3d', 'R3d+T')
_SUM, _MAX, _MIN = 8, 48, 88


@pytest.fixture(autouse=True)
def _no_autotune(monkeypatch):
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _logger():
    lg = logging.getLogger('egonet_amd.test_gpu_lifter_metrics')
    lg.setLevel(logging.INFO)
    lg.propagate = False
    h = _Lines()
    lg.handlers = [h]
    return lg, h


def _fixture(layout):
    g = golden('lifter_metrics.npz')
    p = layout + '/'
    return g, g[p + 'pred'], g[p + 'gt'], g[p + 'mean_out'].reshape(-1), g[p + 'std_out'].reshape(-1)


def _run(pred, gt, layout, mean=None, std=None, batches=None, rows=True, total=None):
    """Raw ABI: (accumulator [128] float64, per-row columns [n, cols] or None) after reset + one update per batch."""
    L = _lib.lib()
    dev = torch.device('cuda')
    lay = int(layout == 'R3d+T')
    p, t = torch.from_numpy(np.ascontiguousarray(pred)).to(dev), torch.from_numpy(np.ascontiguousarray(gt)).to(dev)
    m = s = None
    if mean is not None:
        m, s = torch.from_numpy(np.ascontiguousarray(mean)).to(dev), torch.from_numpy(np.ascontiguousarray(std)).to(dev)
    n, D = p.shape
    acc = torch.full((128,), float('nan'), dtype=torch.float64, device=dev)
    out = torch.full((n, ref.COLS[layout]), float('nan'), dtype=torch.float64, device=dev) if rows else None
    st = _lib.current_stream(dev)
    _lib.check(L.egn_lifter_metrics_reset(_lib.ptr(acc), lay, st))
    b0 = 0
    for b in (batches or [n]):
        nb = L.egn_lifter_metrics_ws_bytes(b)
        assert nb > 0
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        # (an empty slice has no address: n = 0 is called with the arrays' own, valid pointers)
        _lib.check(L.egn_lifter_metrics_update_f32(_lib.ptr(p[b0:b0 + b]) if b else _lib.ptr(p), _lib.ptr(t[b0:b0 + b])
                                                   if b else _lib.ptr(t), b, D, D, _lib.ptr(m), _lib.ptr(s), lay,
                                                   _lib.ptr(ws), nb, _lib.ptr(acc),
                                                   _lib.ptr(out[b0:b0 + b]) if rows and b else None, st))
        b0 += b
    assert b0 == (n if total is None else total)
    torch.cuda.synchronize()
    return acc.cpu().numpy(), (out.cpu().numpy() if rows else None)


def _check_rows(got, want):
    """Distances 1e-9 m; Euler errors 1e-9 rad, the bound of the pose solve's Kabsch angles (test_host_math.py:40)."""
    assert np.isfinite(got).all()
    d_ang = np.abs(np.deg2rad(got[:, 32:35]) - np.deg2rad(want[:, 32:35])).max()
    d_len = np.abs(np.delete(got, [32, 33, 34], axis=1) - np.delete(want, [32, 33, 34], axis=1)).max()
    print('per-row: max |angle diff| %.3e rad, max |distance diff| %.3e m' % (d_ang, d_len))
    assert d_ang <= 1e-9 and d_len <= 1e-9


@pytest.mark.parametrize('layout', LAYOUTS)
def test_rows_and_accumulator_on_the_fixture(layout):
    g, pred, gt, mean, std = _fixture(layout)
    cols = ref.COLS[layout]
    want = ref.rows(pred, gt, layout, mean, std)
    acc, got = _run(pred, gt, layout, mean, std)
    _check_rows(got, want)
    # the accumulator against the kernel's own rows: max / min exact, count exact, sums to the float64 bound
    assert acc[0] == len(pred) and acc[1] == int(layout == 'R3d+T')
    assert np.array_equal(acc[_MAX:_MAX + cols], got.max(axis=0))
    assert np.array_equal(acc[_MIN:_MIN + cols], got.min(axis=0))
    np.testing.assert_allclose(acc[_SUM:_SUM + cols], got.sum(axis=0), rtol=1e-13, atol=0)
    assert np.all(acc[_MAX + cols:_MAX + 40] == -1.0) and np.all(acc[_MIN + cols:_MIN + 40] == 1e16)
    # two runs: the same bits
    acc2, got2 = _run(pred, gt, layout, mean, std)
    assert acc.tobytes() == acc2.tobytes() and got.tobytes() == got2.tobytes()
    # ragged batches: max / min / count equal, sums to the float64 bound (another order of the same additions)
    acc3, got3 = _run(pred, gt, layout, mean, std, batches=[int(b) for b in g['batches']])
    assert got3.tobytes() == got.tobytes()
    assert acc3[0] == acc[0]
    assert np.array_equal(acc3[_MAX:_MAX + 40], acc[_MAX:_MAX + 40])
    assert np.array_equal(acc3[_MIN:_MIN + 40], acc[_MIN:_MIN + 40])
    np.testing.assert_allclose(acc3[_SUM:_SUM + cols], acc[_SUM:_SUM + cols], rtol=1e-13, atol=0)
    # the fused unnormalise is torch's float32 product and sum: the same rows, the same bits
    dev = torch.device('cuda')
    pu = (torch.from_numpy(pred).to(dev) * torch.from_numpy(std).to(dev) + torch.from_numpy(mean).to(dev)).cpu().numpy()
    gu = (torch.from_numpy(gt).to(dev) * torch.from_numpy(std).to(dev) + torch.from_numpy(mean).to(dev)).cpu().numpy()
    assert pu.dtype == np.float32
    acc4, got4 = _run(pu, gu, layout)
    assert got4.tobytes() == got.tobytes() and acc4.tobytes() == acc.tobytes()


@pytest.mark.parametrize('name', ['RError3D', 'RTError3D', 'JointDistance3D', 'RotationError3D', 'Evaluator'])
def test_classes_against_the_reference_attributes(name):
    """The reference's distances, H and SVD are float32: per attribute the bound is ten times the gap between the
    float64 restatement and the reference that the fixture's generator measured and stored (gap/...), absolute."""
    g = golden('lifter_metrics.npz')
    layout = str(g[name + '/layout'])
    _, pred, gt, mean, std = _fixture(layout)
    cfgs = json.loads(str(g['cfgs']))
    obj = {'RError3D': lambda: cr.RError3D(cfgs, 33), 'RTError3D': lambda: cr.RTError3D(cfgs, 33),
           'JointDistance3D': lambda: cr.JointDistance3D(cfgs), 'RotationError3D': lambda: cr.RotationError3D(cfgs),
           'Evaluator': lambda: cr.Evaluator(['RError3D'], cfgs, 33)}[name]()
    dev = torch.device('cuda')
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    stats = {'mean_out': mean.reshape(1, -1), 'std_out': std.reshape(1, -1)}
    L = _lib.lib()
    c0 = L.egn_launch_count()
    b0 = 0
    for b in g['batches']:
        obj.update(p[b0:b0 + b], ground_truth=t[b0:b0 + b], statistics=stats)
        b0 += int(b)
    assert L.egn_launch_count() - c0 == 1 + 2 * len(g['batches'])            # reset, then rows + fold per batch
    metric = obj.metrics[0] if name == 'Evaluator' else obj
    seen = 0
    for k in g.files:
        if not k.startswith(name + '/') or k.split('/')[1].split('_')[0] not in ('count', 'mean', 'max', 'min'):
            continue
        a = k.split('/')[1]
        want, got, bound = g[k], getattr(metric, a), 10.0 * float(g['gap/' + k])
        seen += 1
        if a.startswith('count'):
            assert int(got) == int(want) == len(pred)
            continue
        assert isinstance(got, np.ndarray) and got.shape == want.shape
        err = float(np.abs(got - want).max())
        print('%s.%s: max |device - reference| %.3e, bound %.3e' % (name, a, err, bound))
        assert err <= bound
    assert seen >= 4
    lg, h = _logger()
    obj.report(lg)
    assert len(h.lines) == 1 and h.lines[0].startswith('Error type: ' + metric.name)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_small_and_odd_batches_and_bad_arguments(layout):
    _, pred, gt, mean, std = _fixture(layout)
    want = ref.rows(pred[:7], gt[:7], layout, mean, std)
    for n in (1, 7):                                  # n = 1 and n odd: a half-empty wave
        acc, got = _run(pred[:n], gt[:n], layout, mean, std)
        _check_rows(got, want[:n])
        cols = ref.COLS[layout]
        assert acc[0] == n
        assert np.array_equal(acc[_MAX:_MAX + cols], got.max(axis=0))
        assert np.array_equal(acc[_MIN:_MIN + cols], got.min(axis=0))
    acc, _ = _run(pred[:4], gt[:4], layout, mean, std, batches=[0, 0], rows=False, total=0)    # n = 0: a no-op
    assert acc[0] == 0 and np.all(acc[_SUM:_SUM + 40] == 0) and np.all(acc[_MAX:_MAX + 40] == -1)
    assert np.all(acc[_MIN:_MIN + 40] == 1e16)
    L = _lib.lib()
    dev = torch.device('cuda')
    p = torch.from_numpy(pred[:4]).to(dev)
    acc_t = torch.zeros(128, dtype=torch.float64, device=dev)
    ws = torch.empty(L.egn_lifter_metrics_ws_bytes(4), dtype=torch.uint8, device=dev)
    st = _lib.current_stream(dev)
    lay, D = int(layout == 'R3d+T'), p.shape[1]

    def call(pp=p, tt=p, n=4, d=D, ld=D, m=None, s=None, la=lay, w=ws, wb=None, a=acc_t):
        return L.egn_lifter_metrics_update_f32(_lib.ptr(pp), _lib.ptr(tt), n, d, ld, _lib.ptr(m), _lib.ptr(s), la,
                                               _lib.ptr(w), ws.numel() if wb is None else wb, _lib.ptr(a), None, st)
    assert call() == 0
    assert call(n=-1) == -1 and call(d=D - 3) == -1 and call(la=1 - lay) == -1 and call(ld=D - 1) == -1
    assert call(pp=None) == -1 and call(tt=None) == -1 and call(w=None) == -1 and call(a=None) == -1
    assert call(m=p[0]) == -1 and call(wb=8) == -1 and call(la=2) == -1
    assert L.egn_lifter_metrics_ws_bytes(-1) == -1
    assert L.egn_lifter_metrics_reset(None, 0, st) == -1 and L.egn_lifter_metrics_reset(_lib.ptr(acc_t), 2, st) == -1
    torch.cuda.synchronize()


def test_degenerate_rows_never_give_nan():
    rng = np.random.RandomState(5)
    gt = rng.randn(4, 96).astype(np.float32)
    pred = gt.copy()
    pred[0] = np.tile(np.array([1.0, 2.0, 3.0], dtype=np.float32), 32)              # H = 0
    pred[1] = np.outer(np.linspace(-1, 1, 32), [1.0, 0.5, -2.0]).astype(np.float32).reshape(-1)    # rank 1
    acc, got = _run(pred, gt, 'R3d')
    assert np.isfinite(got).all() and np.isfinite(acc).all()
    assert np.array_equal(got[0, 32:35], np.zeros(3))
    assert np.array_equal(got[2, :32], np.zeros(32))                                # prediction == target:
    assert np.deg2rad(got[2, 32:35]).max() <= 1e-9                                  # the identity up to rounding


def _lifting_cfgs(epochs=1, batch=256):
    cfg = configs.clone(configs.w48_config())
    cfg['FCModel'].update(num_neurons=64, num_blocks=1, dropout=0.0)
    cfg.update(use_gpu=True, exp_type='2dto3d', cascade={'num_stages': 1},
               metrics={'R3D': {'T_style': 'direct', 'R_style': 'euler', 'style': 'euler'},
                        'RTError3D': {'T_style': 'direct', 'R_style': 'euler'}, 'JD3D': {'style': 'direct'}},
               dataset={'detect_classes': ['Car'], '3d_kpt_sample_style': 'bbox9',
                        'interpolate': {'flag': True, 'style': 'bbox12', 'coef': [0.332, 0.667]},
                        'lft_in_rep': 'coordinates2d', 'lft_out_rep': 'R3d'},
               optimizer={'optim_type': 'adam', 'lr': 1e-3, 'weight_decay': 0.0, 'momentum': 0.9,
                          'milestones': [1], 'gamma': 0.1},
               training_settings={'total_epochs': epochs, 'batch_size': batch, 'num_threads': 0, 'shuffle': True,
                                  'report_every': 100, 'eval_during': True, 'eval_every': 2, 'eval_start_epoch': 0,
                                  'eval_metrics': ['RError3D'], 'plot_loss': False, 'lft_aug': True,
                                  'lft_aug_times': 4},
               testing_settings={'batch_size': 64, 'num_threads': 0, 'shuffle': False, 'unnormalize': True})
    return cfg


class _Recorder(cr.Evaluator):
    """The device Evaluator, recording what evaluate() handed over."""

    def __init__(self, *a):
        super().__init__(*a)
        self.batches = []

    def update(self, prediction, ground_truth=None, meta_data=None, logger=None, statistics=None):
        assert torch.is_tensor(prediction) and prediction.is_cuda and ground_truth.is_cuda and statistics is not None
        self.batches.append((prediction.detach().clone(), ground_truth.detach().clone()))
        super().update(prediction, ground_truth=ground_truth, meta_data=meta_data, logger=logger,
                       statistics=statistics)


def test_evaluate_keeps_predictions_on_the_device(monkeypatch):
    cfg = _lifting_cfgs()
    train_set = lp.LifterPairBuilder(cfg, 'train')(synth.synth_kitti_labels(60, seed=0)).normalize()
    valid_set = lp.LifterPairBuilder(cfg, 'valid')(synth.synth_kitti_labels(300, seed=1)).normalize(
        train_set.statistics)
    n = len(valid_set)
    assert n > 130                                                 # at least three batches of 64
    net = FCmodel.get_fc_model(1, cfg, 66, 96)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=3))
    net = net.cuda()
    ev = _Recorder(['RError3D'], cfg, train_set.num_joints)
    lg, h = _logger()
    cpu_calls = []
    orig_cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        cpu_calls.append(tuple(self.shape))
        return orig_cpu(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, 'cpu', counting_cpu)
    trainer.evaluate(valid_set, net, None, cfg, lg, ev)
    monkeypatch.setattr(torch.Tensor, 'cpu', orig_cpu)
    nb = (n + 63) // 64
    assert len(ev.batches) == nb
    assert (128,) in cpu_calls                                     # the accumulator's read-back in report() ...
    assert not [s for s in cpu_calls if len(s) == 2]               # ... and no batch of rows
    assert any(l.startswith('Error type: RError3D') for l in h.lines)
    pred = torch.cat([b[0] for b in ev.batches]).cpu().numpy()
    gt = torch.cat([b[1] for b in ev.batches]).cpu().numpy()
    st = valid_set.statistics
    want = ref.statistics(ref.rows(pred, gt, 'R3d', st['mean_out'], st['std_out']), 'R3d')
    m = ev.metrics[0]
    assert m.count_rT == m.count_R == n
    for k in ('max_rT', 'min_rT'):
        np.testing.assert_allclose(getattr(m, k), want[k], rtol=0, atol=1e-9)
    for k in ('max_R', 'min_R'):
        np.testing.assert_allclose(np.deg2rad(getattr(m, k)), np.deg2rad(want[k]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(m.mean_rT, want['mean_rT'], rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.deg2rad(m.mean_R), np.deg2rad(want['mean_R']), rtol=0, atol=1e-9)
    # the host evaluator (device_update off) through the unchanged path agrees
    ev_h = cr.Evaluator(['RError3D'], cfg, train_set.num_joints)
    ev_h.device_update = False
    trainer.evaluate(valid_set, net, None, cfg, lg, ev_h)
    np.testing.assert_allclose(ev_h.metrics[0].mean_rT, m.mean_rT, rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.deg2rad(ev_h.metrics[0].mean_R), np.deg2rad(m.mean_R), rtol=0, atol=1e-9)
    # save=True with the device evaluator: the unnormalised arrays, as before
    path = os.path.join(ROOT, 'tests', '_build', 'lifter_metrics_eval.npy')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    trainer.evaluate(valid_set, net, None, cfg, lg, cr.Evaluator(['RError3D'], cfg, 33), save=True, save_path=path)
    saved = np.load(path, allow_pickle=True).item()
    assert np.array_equal(saved['pred'], ref.unnormalize_f32(pred, st['mean_out'], st['std_out']))
    assert np.array_equal(saved['gt'], ref.unnormalize_f32(gt, st['mean_out'], st['std_out']))


def test_train_cascade_validates_with_eval_metrics():
    cfg = _lifting_cfgs(epochs=1, batch=256)
    train_set = lp.LifterPairBuilder(cfg, 'train')(synth.synth_kitti_labels(300, seed=0)).normalize()
    valid_set = lp.LifterPairBuilder(cfg, 'valid')(synth.synth_kitti_labels(40, seed=1)).normalize(
        train_set.statistics)
    assert len(train_set) > 2 * 256                                # batch index 2 exists: one validation
    lg, h = _logger()
    trainer.train_cascade(train_set, valid_set, cfg, lg)
    lines = [l for l in h.lines if l.startswith('Error type: RError3D')]
    assert lines and 'MPJPE: ' in lines[0] and 'Mean error: [' in lines[0]
    assert not any('no validation during training' in l for l in h.lines)


def test_train_lifting_tool_logs_the_metric(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train_lifting.py'), '--synthetic', '300',
                          '--out', str(tmp_path), '--epochs', '1', '--batch-size', '256', '--aug-times', '4',
                          '--neurons', '64', '--blocks', '1', '--eval-every', '2'],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, text=True,
                         env=dict(os.environ, EGONET_AMD_AUTOTUNE='0'))
    assert out.returncode == 0, out.stdout[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('Error type: RError3D')]
    assert len(lines) >= 2, out.stdout[-3000:]                     # during training and the final pass
    assert os.path.isfile(str(tmp_path / 'L.pth'))
