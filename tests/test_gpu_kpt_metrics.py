"""get_distance_src / JointDistance2DSIP on the device (csrc/kpt_metrics.hip): bit-equality with the existing decoder,
parity with the REFERENCE's outputs (tests/golden/metric.npz) and with the host path of the same tree, the
accumulator's behaviour, and the two loops that use it (trainer.evaluate, trainer.train).

Tolerances.  Fixture: src_coord 5e-3 px and avg rtol 1e-5 against the golden (test_gpu_metric.py's bounds), avg
rtol 1e-12 against a float64 numpy evaluation of the kernel's own src_coord (at most a few hundred float64 additions
in another order).  Against the host path on the same inputs the decode is the same kernel (equal bits), the rescale
is one float32 product, and what is left is the closed-form affine against np.linalg.solve: 2.3e-13 px measured on the
CPU (test_kpt_metric_math_host.py), so src_coord is held to 1e-9 px; PCK counts are asserted only after the inputs'
margin to every threshold (>= 100 x that tolerance) has been."""
import logging

import numpy as np
import pytest
import torch

from conftest import golden
from egonet_amd import _lib, configs, synth, trainer
from egonet_amd.common import img_proc
from egonet_amd.metric import criterions
from egonet_amd.metric.criterions import DistanceSrcMeter, JointDistance2DSIP, _KptMetricsDevice

pytestmark = pytest.mark.gpu

HOST_ATOL = 1e-9
MODES = {'hard': 0, 'soft': 1, 'soft-np': 2}


def _meta(g, rotation=True, keys=('center', 'scale', 'original_joints')):
    m = {k: g[k] for k in keys}
    if rotation:
        m['rotation'] = g['rotation']
    return m


def _numpy_stats(src, joints):
    """(avg, cnt, correct) of get_distance / get_PCK over float64 src_coord [n,K,2]."""
    dists, correct = [], np.zeros(3)
    for s, gt in zip(src, joints):
        dists += criterions.get_distance(gt, s)
        correct += criterions.get_PCK(s, gt)
    return (sum(dists) / len(dists) if dists else 0.0), len(dists), correct


def _margin(src, joints):
    """Smallest |distance - threshold| over the visible joints."""
    joints = np.asarray(joints, dtype=np.float64)
    vis = joints[:, :, 2] != 0 if joints.shape[2] == 3 else np.ones(joints.shape[:2], dtype=bool)
    dist = np.sqrt(((joints[:, :, :2] - src) ** 2).sum(axis=2))
    den = (joints[:, :, 1].max(axis=1) - joints[:, :, 1].min(axis=1)) / 3
    return np.abs(dist[:, :, None] - criterions.PCK_THRES[None, None] * den[:, None, None])[vis].min()


# ---- bit-equality with the existing decoder ---------------------------------------------------------------------
@pytest.mark.parametrize('arg_max', ['hard', 'soft', 'soft-np'])
def test_heatmap_decode_is_bit_identical_to_the_decoder(arg_max):
    """165 maps (5 x 33, no multiple of the 4 waves of a block): joints_pred / max_vals == the decode entry point's
    output x the float32 factor.  A contraction mismatch between the two translation units shows here."""
    g = golden('metric.npz')
    hm = torch.from_numpy(g['heatmaps']).cuda()
    out = _KptMetricsDevice().update(hm, _meta(g), (64.0, 64.0), arg_max, want=('joints_pred', 'max_vals'))
    xy, mx, _ = img_proc._decode(hm, MODES[arg_max], want_idx=False)
    assert torch.equal(out['joints_pred'], xy * np.float32(64.0 / 16))
    assert torch.equal(out['max_vals'], mx)
    assert out['joints_pred'].dtype == torch.float32 and tuple(out['joints_pred'].shape) == (5, 33, 2)


def test_coordinate_tuple_is_rescaled_in_float32():
    g = golden('metric.npz')
    coords = torch.from_numpy(g['coords']).cuda()
    out = _KptMetricsDevice().update((None, coords), _meta(g), (64.0, 48.0), 'hard',
                                     want=('joints_pred', 'max_vals'))
    assert torch.equal(out['joints_pred'], coords * torch.tensor([64.0, 48.0], device='cuda'))
    assert 'max_vals' not in out


# ---- the reference's outputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize('arg_max,tag,rotation', [('hard', 'hard', True), ('soft-np', 'soft', True),
                                                  ('coords', 'coords', True), ('hard', 'norot', False)])
def test_fixture_parity(arg_max, tag, rotation):
    g = golden('metric.npz')
    if arg_max == 'coords':
        pred = (torch.from_numpy(g['heatmaps']).cuda(), torch.from_numpy(g['coords']).cuda())
    else:
        pred = torch.from_numpy(g['heatmaps']).cuda()
    meter = DistanceSrcMeter(image_size=(64.0, 64.0), arg_max=arg_max)
    avg, cnt, others = meter(pred, _meta(g, rotation))
    print('%s: avg %.15g cnt %d correct %s' % (tag, avg, cnt, others['correct_cnt']))
    np.testing.assert_allclose(others['src_coord'], g[tag + '/src_coord'], rtol=0, atol=5e-3)
    want_avg, want_cnt, want_correct = _numpy_stats(others['src_coord'], g['original_joints'])
    assert cnt == 103 and cnt == want_cnt
    ref = 'hard' if tag == 'norot' else tag                # the fixture's rotations move no joint across a threshold
    np.testing.assert_array_equal(others['correct_cnt'], g[ref + '/correct_cnt'])
    np.testing.assert_array_equal(others['correct_cnt'], want_correct)
    np.testing.assert_allclose(avg, float(g[tag + '/avg']), rtol=1e-5)
    np.testing.assert_allclose(avg, want_avg, rtol=1e-12)
    np.testing.assert_allclose(others['PCK_batch'], others['correct_cnt'] / cnt)
    if arg_max != 'coords':
        np.testing.assert_allclose(others['joints_pred'], g[ref + '/joints_pred'], rtol=0, atol=1e-3)
        assert (others['joints_pred'][0, 0] == 0).all()     # all-negative map: zeroed
        assert others['max_vals'].shape == (5, 33, 1)
    else:
        assert others['max_vals'] is None


# ---- the host path of the same tree -----------------------------------------------------------------------------
def _random_case(N, K, H, W, n, seed, two_columns=False):
    rng = np.random.RandomState(seed)
    hm = rng.randn(N, K, H, W).astype(np.float32)
    hm[0, 0] = -np.abs(hm[0, 0])                           # an all-negative map
    center = rng.rand(n, 2) * [1242.0, 375.0]
    s = 0.3 + rng.rand(n) * 1.5
    scale = np.stack([s, s * (0.7 + 0.6 * rng.rand(n))], axis=1)
    rotation = rng.choice([0.0, 90.0, -90.0, 180.0, 33.3, -12.5], n)
    joints = np.concatenate([center[:, None] + (rng.rand(n, K, 2) - 0.5) * 200 * scale[:, None],
                             (rng.rand(n, K, 1) > 0.3).astype(np.float64)], axis=2)
    if n > 1:
        joints[1, :, 2] = 0.0                              # an instance with no visible joint
    if two_columns:
        joints = joints[:, :, :2].copy()
    return hm, {'center': center, 'scale': scale, 'rotation': rotation, 'original_joints': joints}


def _against_host(pred_dev, pred_host, meta, image_size, arg_max, host_arg_max):
    meter = DistanceSrcMeter(image_size=image_size, arg_max=arg_max)
    avg, cnt, others = meter(pred_dev, meta)
    h_avg, h_cnt, h_others = criterions.get_distance_src(pred_host, meta, image_size=image_size, arg_max=host_arg_max)
    print('device avg %.15g cnt %d correct %s | host avg %.15g cnt %d correct %s | largest src_coord difference %.3e'
          % (avg, cnt, others['correct_cnt'], h_avg, h_cnt, h_others['correct_cnt'],
             np.abs(others['src_coord'] - h_others['src_coord']).max()))
    np.testing.assert_array_equal(others['joints_pred'], h_others['joints_pred'])
    if h_others['max_vals'] is not None:
        np.testing.assert_array_equal(others['max_vals'], h_others['max_vals'])
    np.testing.assert_allclose(others['src_coord'], h_others['src_coord'], rtol=0, atol=HOST_ATOL)
    assert _margin(h_others['src_coord'], meta['original_joints']) >= 100 * HOST_ATOL
    assert cnt == h_cnt
    np.testing.assert_array_equal(others['correct_cnt'], h_others['correct_cnt'])
    np.testing.assert_allclose(avg, h_avg, rtol=1e-12)
    return others


@pytest.mark.parametrize('arg_max,host_arg_max,as_numpy', [('hard', 'hard', False), ('soft', 'soft', False),
                                                           ('soft-np', 'soft', True)])
def test_scalar_decode_path_5x7_maps(arg_max, host_arg_max, as_numpy):
    """35 elements: no multiple of 4, the scalar two-pass decode.  N = 3, K = 5, two labelled; a non-square window whose
    factor 60 / 7 is no power of two."""
    hm, meta = _random_case(3, 5, 5, 7, 2, seed=21)
    if arg_max == 'soft-np':
        hm = np.abs(hm) + 0.1                              # weights hm / sum(hm): keep the sum away from zero
    t = torch.from_numpy(hm).cuda()
    _against_host(t, hm.copy() if as_numpy else t, meta, (60.0, 40.0), arg_max, host_arg_max)


@pytest.mark.parametrize('arg_max', ['hard', 'soft'])
def test_register_path_64x64_maps_many_blocks(arg_max):
    """N = 64, K = 33: 2112 maps, 528 blocks, so the fold runs over many partials; 60 labelled, one of them with no
    visible joint; rotations 0, +-90, 180, 33.3, -12.5; non-square scale."""
    hm, meta = _random_case(64, 33, 64, 64, 60, seed=22)
    t = torch.from_numpy(hm).cuda()
    others = _against_host(t, t, meta, (256.0, 256.0), arg_max, arg_max)
    assert others['src_coord'].shape == (60, 33, 2)


def test_two_column_joints_and_coordinate_head():
    hm, meta = _random_case(6, 33, 16, 16, 6, seed=23, two_columns=True)
    coords = torch.rand(6, 33, 2, generator=torch.Generator().manual_seed(4)).cuda()
    pred = (torch.from_numpy(hm).cuda(), coords)
    meter = DistanceSrcMeter(image_size=(256, 256))
    avg, cnt, others = meter(pred, meta)
    h_avg, h_cnt, h_others = criterions.get_distance_src(pred, meta, image_size=(256, 256))
    assert cnt == h_cnt == 6 * 33                          # no visibility column: every joint counts
    np.testing.assert_array_equal(others['joints_pred'], h_others['joints_pred'])       # x 256: exact in float32 too
    np.testing.assert_allclose(others['src_coord'], h_others['src_coord'], rtol=0, atol=HOST_ATOL)
    assert _margin(h_others['src_coord'], meta['original_joints']) >= 100 * HOST_ATOL
    np.testing.assert_array_equal(others['correct_cnt'], h_others['correct_cnt'])
    np.testing.assert_allclose(avg, h_avg, rtol=1e-12)


def test_no_labelled_instance_counts_nothing():
    hm, _ = _random_case(2, 5, 16, 16, 1, seed=24)
    t = torch.from_numpy(hm).cuda()
    meta = {'center': np.zeros((0, 2)), 'scale': np.zeros((0, 2)), 'original_joints': np.zeros((0, 5, 3))}
    dev = _KptMetricsDevice()
    out = dev.update(t, meta, (64.0, 64.0), 'hard', want=('src_coord', 'joints_pred'))
    assert np.array_equal(dev.peek(), np.zeros(8)) and tuple(out['src_coord'].shape) == (0, 5, 2)
    xy, _, _ = img_proc._decode(t, 0, want_idx=False)
    assert torch.equal(out['joints_pred'], xy * np.float32(4.0))
    avg, cnt, others = DistanceSrcMeter(image_size=(64.0, 64.0))(t, meta)
    assert (avg, cnt) == (0.0, 0) and np.array_equal(others['correct_cnt'], np.zeros(3))


def test_cuda_meta_and_bad_arguments():
    g = golden('metric.npz')
    hm = torch.from_numpy(g['heatmaps']).cuda()
    meta = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in _meta(g).items()}
    avg, cnt, others = DistanceSrcMeter(image_size=(64.0, 64.0))(hm, meta)
    avg2, cnt2, others2 = DistanceSrcMeter(image_size=(64.0, 64.0))(hm, _meta(g))
    assert (avg, cnt) == (avg2, cnt2) and np.array_equal(others['src_coord'], others2['src_coord'])
    with pytest.raises(NotImplementedError):
        DistanceSrcMeter(image_size=(64.0, 64.0), arg_max=None)(hm, _meta(g))
    with pytest.raises(TypeError):
        DistanceSrcMeter()(g['heatmaps'], _meta(g))
    with pytest.raises(ValueError):                         # more labelled instances than predictions
        DistanceSrcMeter(image_size=(64.0, 64.0))(hm[:3], _meta(g))
    L = _lib.lib()
    acc = torch.zeros(8, dtype=torch.float64, device='cuda')
    ws = torch.zeros(L.egn_kpt_metrics_ws_bytes(5, 33), dtype=torch.uint8, device='cuda')
    st = _lib.current_stream()
    args = [5, 33, 16, 16, 0, None, None, None, None, 0, 64.0, 64.0, _lib.ptr(ws), ws.numel(), _lib.ptr(acc), None,
            None, None, st]
    assert L.egn_kpt_metrics_update_f32(None, None, *args) == -1                        # neither prediction
    assert L.egn_kpt_metrics_update_f32(_lib.ptr(hm), _lib.ptr(hm), *args) == -1        # both
    short = list(args)
    short[13] = ws.numel() - 1
    assert L.egn_kpt_metrics_update_f32(_lib.ptr(hm), None, *short) == -1               # a short workspace
    assert L.egn_kpt_metrics_ws_bytes(1 << 20, 1 << 12) == -1 and L.egn_kpt_metrics_reset(None, st) == -1


# ---- the accumulator --------------------------------------------------------------------------------------------
def _cfgs(arg_max='hard'):
    return {'heatmapModel': {'num_joints': 33, 'input_size': [64.0, 64.0]}, 'testing_settings': {'arg_max': arg_max}}


def test_running_metric_accumulates_on_the_device_and_merges_with_host_updates():
    g = golden('metric.npz')
    hm = torch.from_numpy(g['heatmaps']).cuda()
    L = _lib.lib()
    m = JointDistance2DSIP(_cfgs())
    m.update(hm, _meta(g))
    c0 = L.egn_launch_count()
    m.update(hm, _meta(g))
    assert L.egn_launch_count() - c0 == 2                   # the maps kernel and the fold, nothing else
    assert m._count == 0 and m._dev.pending                 # nothing read back yet
    assert m.count == 2 * 103 and type(m.count) is int and not m._dev.pending
    assert isinstance(m.mean, float) and m.PCK_counts.dtype == np.float64 and m.PCK_counts.shape == (3,)
    np.testing.assert_allclose(m.mean, float(g['hard/avg']), rtol=1e-5)
    np.testing.assert_array_equal(m.PCK_counts, 2 * g['hard/correct_cnt'])
    one = JointDistance2DSIP(_cfgs())
    one.update(hm, _meta(g))
    np.testing.assert_allclose(m.mean, one.mean, rtol=1e-14)                 # count doubles, the mean stays
    # a device update followed by a numpy update of the same object
    mixed = JointDistance2DSIP(_cfgs())
    mixed.update(hm, _meta(g))
    mixed.update(g['heatmaps'].copy(), _meta(g))
    host = JointDistance2DSIP(_cfgs())
    host.update(g['heatmaps'].copy(), _meta(g))
    host.update(g['heatmaps'].copy(), _meta(g))
    assert mixed.count == host.count == 206
    np.testing.assert_allclose(mixed.mean, host.mean, rtol=1e-12)
    np.testing.assert_array_equal(mixed.PCK_counts, host.PCK_counts)
    mixed.update(hm, _meta(g))                              # and a device update after the read-back
    assert mixed.count == 309
    np.testing.assert_allclose(mixed.mean, host.mean, rtol=1e-12)


def test_equal_inputs_give_equal_bits():
    hm, meta = _random_case(64, 33, 64, 64, 64, seed=25)
    t = torch.from_numpy(hm).cuda()
    accs = []
    for _ in range(2):
        dev = _KptMetricsDevice()
        dev.update(t, meta, (256.0, 256.0), 'soft')
        dev.update(t, meta, (256.0, 256.0), 'soft')
        accs.append(dev.peek())
    assert accs[0].tobytes() == accs[1].tobytes() and accs[0][0] > 0


def test_meter_accumulate_read_reset():
    g = golden('metric.npz')
    hm = torch.from_numpy(g['heatmaps']).cuda()
    meter = DistanceSrcMeter(_cfgs())                       # image_size from cfgs
    assert meter.read()[1] == 0
    meter.accumulate(hm, _meta(g))
    meter.accumulate(hm, _meta(g), _cfgs())
    mean, cnt, pck = meter.read()
    assert cnt == 206 and meter.read()[1] == 206            # reading does not clear
    np.testing.assert_allclose(mean, float(g['hard/avg']), rtol=1e-5)
    np.testing.assert_array_equal(pck, 2 * g['hard/correct_cnt'])
    meter.reset()
    assert meter.read()[1] == 0
    for _ in range(3):                                      # more turns than pinned buffers
        meter.accumulate(hm, _meta(g))
    assert meter.read()[1] == 309


# ---- the loops --------------------------------------------------------------------------------------------------
class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _logger():
    lg = logging.getLogger('egonet_amd.test_kpt_metrics')
    lg.setLevel(logging.INFO)
    h = _Lines()
    lg.handlers = [h]
    return lg, h


class _FixtureSet(torch.utils.data.Dataset):
    def __init__(self, g):
        self.g = g

    def __len__(self):
        return 4

    def __getitem__(self, i):
        return torch.tensor([i]), torch.zeros(1), torch.ones(1), i


class _Stub(torch.nn.Module):
    """Returns the fixture maps of the batch: CUDA tensors, or numpy arrays (the host path)."""

    def __init__(self, maps, as_numpy):
        super().__init__()
        self.maps, self.as_numpy = maps, as_numpy

    def forward(self, data):
        idx = data.reshape(-1).cpu().numpy()
        return self.maps[idx].copy() if self.as_numpy else torch.from_numpy(self.maps[idx]).cuda()


def test_evaluate_reports_like_the_host_path():
    """trainer.evaluate over the fixture in two batches with Evaluator(['JointDistance2DSIP']): the report() lines
    equal the host path's."""
    g = golden('metric.npz')

    def collate(items):
        idx = [it[3] for it in items]
        meta = {k: g[k][idx] for k in ('center', 'scale', 'rotation', 'original_joints')}
        return (torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items]),
                torch.stack([it[2] for it in items]), meta)
    cfg = _cfgs()
    cfg['testing_settings'].update(batch_size=2, num_threads=0, shuffle=False, unnormalize=False, apply_dropout=False)
    cfg['use_gpu'] = True
    lines = []
    for as_numpy in (False, True):
        ev = criterions.Evaluator(['JointDistance2DSIP'], cfg)
        lg, h = _logger()
        trainer.evaluate(_FixtureSet(g), _Stub(g['heatmaps'], as_numpy), None, cfg, lg, ev, collate_fn=collate)
        lines.append(h.lines)
        assert ev.metrics[0].count == 103
    dev, host = lines
    print('\n'.join(dev + host))
    assert len(dev) == 5 and dev == host


class _LabelledCrops(torch.utils.data.Dataset):
    def __init__(self, n=16, K=5):
        g = torch.Generator().manual_seed(1)
        rng = np.random.RandomState(3)
        self.x = synth.synth_crops(n, 3, 64, 64, seed=3)
        self.t = torch.rand(n, K, 16, 16, generator=g)
        self.j = (torch.rand(n, K, 3, generator=g) * 64).numpy()
        self.center = rng.rand(n, 2) * [1242.0, 375.0]
        self.scale = np.repeat(0.3 + rng.rand(n, 1), 2, axis=1)
        self.joints = np.concatenate([self.center[:, None] + (rng.rand(n, K, 2) - 0.5) * 100,
                                      (rng.rand(n, K, 1) > 0.2).astype(np.float64)], axis=2)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.t[i], torch.ones(self.t.shape[1], 1), {
            'transformed_joints': self.j[i], 'center': self.center[i], 'scale': self.scale[i],
            'original_joints': self.joints[i]}


class _Spy(object):
    """A DistanceSrcMeter that also runs plain get_distance_src on the very same predictions."""

    def __init__(self, meter):
        self.meter, self.batch, self.host, self.reads = meter, -1, [], []

    def accumulate(self, prediction, meta, cfgs=None):
        self.batch += 1
        self.meter.accumulate(prediction, meta, cfgs)
        avg, cnt, _ = criterions.get_distance_src(prediction, {k: v.numpy() for k, v in meta.items()}, cfgs)
        self.host.append((avg, cnt))

    def read(self):
        got = self.meter.read()
        total = sum(c for _, c in self.host)
        self.reads.append((self.batch, got[0], got[1], sum(a * c for a, c in self.host) / total, total))
        return got

    def reset(self):
        self.meter.reset()
        self.host = []


def test_train_reads_the_meter_on_report_batches_only(monkeypatch, tmp_path):
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    from egonet_amd.model.heatmapModel import hrnet
    cfg = configs.clone(configs.tiny_config('coordinates'))
    cfg.update(use_gpu=True, exp_type='test',
               optimizer={'optim_type': 'adam', 'lr': 5e-3, 'weight_decay': 0.0, 'momentum': 0.9, 'milestones': [3],
                          'gamma': 0.5},
               training_settings={'total_epochs': 2, 'batch_size': 4, 'num_threads': 0, 'shuffle': False,
                                  'report_every': 2, 'eval_during': False, 'plot_loss': False})
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=9))
    net = net.cuda()
    optim, sche = trainer.prepare_optim(net, cfg)
    spy = _Spy(DistanceSrcMeter(cfg))
    lg, h = _logger()
    trainer.train(_LabelledCrops(), net, None, optim, sche, cfg, lg, metric_func=spy)
    assert [r[0] for r in spy.reads] == [0, 2, 4, 6]        # 4 batches per epoch, report every 2: never in between
    for _, mean, cnt, want_mean, want_cnt in spy.reads:
        assert cnt == want_cnt and cnt > 0                  # the running figures restart with the epoch
        np.testing.assert_allclose(mean, want_mean, rtol=1e-9)
    assert spy.reads[0][2] < spy.reads[1][2] and spy.reads[2][2] == spy.reads[0][2]
    metric_lines = [l for l in h.lines if 'running mean over' in l]
    assert metric_lines == ['          metric %.6f (running mean over %d)' % (r[1], r[2]) for r in spy.reads]
    # a plain callable keeps its path
    cfg['training_settings'].update(total_epochs=1, report_every=1)
    calls = []

    def plain(prediction, meta, cfgs):
        calls.append(1)
        return criterions.get_distance_src(prediction, {k: v.numpy() for k, v in meta.items()}, cfgs)
    lg, h = _logger()
    trainer.train(_LabelledCrops(8), net, None, optim, sche, cfg, lg, metric_func=plain)
    assert len(calls) == 2 and sum('running mean over' in l for l in h.lines) == 2
