"""The heat-map head's integral terms on the GPU: L_2d and L_cr on the soft-arg-max of the maps (function.py:187-201).

1. csrc/softargmax.hip: the kernels bit-equal to their host twins (accumulate on / off, n_rows < N, pad channels and
   the rows beyond n_rows bit-unchanged), and the forward against egn_decode_heatmaps_f32 mode 1 within the two
   kernels' derived bounds.
2. ``HRNetTrainStep`` on the tiny heat-map net of tests/test_gpu_train_heads.py against a float64 oracle step
   (oracle.hrnet_oracle.hrnet_forward_train + tests/integral_loss.py, pinned on the reference by
   tests/golden/integral_loss.npz): w_coor; w_cr with apply_cr_loss (K = 33); a mixed batch; non-square maps.
   The bounds are those of the existing heat-map-head step tests on this net (tests/test_gpu_train_hrnet.py::
   test_heatmap_head_vs_oracle, tests/test_gpu_mixed_batches.py): loss 2e-5 relative (2e-3 with L_cr), maps 2e-4,
   gradients cosine > 0.9999, rel-L2 < 1e-2, median per-tensor < 5e-3.  ``last_coords`` follows from the maps' bound:
   a map error of 2e-4 moves ex by at most 2e-4 x sum_p s_p |x_p - ex| <= 1e-4 (w - 1) pixels to first order (d ex /
   d z_p = s_p (x_p - ex); a mean absolute deviation on [0, w - 1] is at most half the range); twice that is allowed
   for the higher orders: x / div_x within 2e-4 w / div_x, which is 2e-4 on square maps and 2e-4 max(w / h, h / w) on
   non-square ones, where each axis is divided by the other's size.
3. With the terms off: the launches, the maps and every gradient (bit for bit) and the loss of a step built the old way.
4. ``trainer.train`` with heatmapModel.integral_terms against the step called directly; the refusals that stay.
"""
import logging

import numpy as np
import pytest
import torch

import integral_loss as IL
from egonet_amd import _lib, configs, softargmax, synth, trainer
from egonet_amd.common.img_proc import get_cr_indices
from egonet_amd.model.heatmapModel import hrnet as hip_hrnet
from egonet_amd.train_hrnet import HRNetTrainStep
from oracle import hrnet_oracle
from oracle.hrnet_train_oracle import HRNetTrainOracle
from program_ops_sweep import C_DEC
from train_checks import gradient_agreement

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_autotune(monkeypatch):
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')


# ---------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ---------------------------------------------------------------------------------------------------------------
# ``loss_dev`` is a float64 word the loss kernels fill by atomic adds of per-wave partials (csrc/train_ops.hip): their
# order is free, so two runs of the SAME step agree to a few float64 ulps, not to the bit.  Everything else -- maps,
# coordinates, every gradient -- is compared by bits where the same step is meant.
LOSS_ULPS = 16 * 2.0 ** -53
SHAPES = [(1, 1, 2, 2, 4), (2, 5, 16, 16, 8), (3, 33, 12, 16, 36), (2, 33, 64, 64, 36)]
SENTINEL = -7777.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('shape', SHAPES)
def test_kernels_bit_equal_to_the_host_twins(shape):
    n, K, h, w, cs = shape
    z, g = IL.sweep_inputs(shape + (3.0,))                                  # pad channels: NaN
    div_x, div_y = float(h), float(w)
    L = _lib.lib()
    zd, gd = torch.from_numpy(z).cuda(), torch.from_numpy(g).cuda()
    c0 = L.egn_launch_count()
    coords, save = softargmax.forward(zd, n, h, w, K, cs, div_x, div_y)
    assert L.egn_launch_count() - c0 == 1
    want_c, want_s = softargmax.forward_host(z, K, div_x, div_y)
    assert np.array_equal(_bits(coords.cpu().numpy()), _bits(want_c))
    assert np.array_equal(_bits(save.cpu().numpy()), _bits(want_s))
    rng = np.random.RandomState(7)
    for accumulate in (False, True):
        for n_rows in sorted({n, max(n - 1, 0)}):
            base = rng.randn(*z.shape).astype(np.float32)
            base[..., K:] = SENTINEL
            dz = torch.from_numpy(base).cuda()
            c0 = L.egn_launch_count()
            softargmax.backward(zd, save, gd, n, n_rows, h, w, K, cs, div_x, div_y, dz, accumulate)
            assert L.egn_launch_count() - c0 == (1 if n_rows else 0)
            want = softargmax.backward_host(z, want_s, g, div_x, div_y, base.copy(), n_rows=n_rows, accumulate=accumulate)
            got = dz.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(want)), (accumulate, n_rows)
            assert np.array_equal(_bits(got[..., K:]), _bits(base[..., K:]))            # pad channels
            assert np.array_equal(_bits(got[n_rows:]), _bits(base[n_rows:]))            # rows beyond n_rows
            if n_rows:
                assert not np.array_equal(got[:n_rows, ..., :K], base[:n_rows, ..., :K])


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_agrees_with_the_decode_kernels_soft_arg_max(shape):
    """Both are float32 soft-arg-maxes of the same maps, each within its own bound of float64: this kernel's
    C x 2^-24 x |value| (+ the underflow floor), the decode's (tests/program_ops_sweep.py: C_DEC U 2 |x64| +
    2 sum p_i (2 + 2.25 |z_i - m|) U |x_i - x64|).  They need not share bits."""
    n, K, h, w, cs = shape
    z, _ = IL.sweep_inputs(shape + (3.0,))
    L = _lib.lib()
    coords, _ = softargmax.forward(torch.from_numpy(z).cuda(), n, h, w, K, cs, 1.0, 1.0)        # pixels
    nchw = torch.from_numpy(np.ascontiguousarray(z[..., :K].transpose(0, 3, 1, 2))).cuda()
    xy = torch.empty(n, K, 2, device='cuda')
    mx = torch.empty(n, K, device='cuda')
    _lib.check(L.egn_decode_heatmaps_f32(_lib.ptr(nchw), n, K, h, w, 1, _lib.ptr(xy), _lib.ptr(mx), None, None))
    torch.cuda.synchronize()
    want, mag, (s, ex, ey) = IL.softargmax64(z, K, 1.0, 1.0)
    z64 = z[..., :K].astype(np.float64)
    d = 2 + 2.25 * np.abs(z64 - z64.max(axis=(1, 2), keepdims=True))
    xs, ys = np.arange(w)[None, None, :, None], np.arange(h)[None, :, None, None]
    spread = np.stack([(s * d * np.abs(xs - ex[:, None, None, :])).sum(axis=(1, 2)),
                       (s * d * np.abs(ys - ey[:, None, None, :])).sum(axis=(1, 2))], axis=2)
    floor = IL.underflow_floor(z, K, 1.0, 1.0, np.zeros((n, K, 2)))[0]
    mine = IL.C_BOUND['fwd'] * IL.EPS * mag + floor
    theirs = C_DEC * IL.EPS * 2 * mag + 2 * IL.EPS * spread + floor
    diff = np.abs(coords.cpu().numpy().astype(np.float64) - xy.cpu().numpy().astype(np.float64))
    print('%s: worst difference %.3e pixels, worst share of the bound %.3f' % (shape, diff.max(),
                                                                                float((diff / (mine + theirs)).max())))
    assert (diff <= mine + theirs).all()
    assert (np.abs(coords.cpu().numpy() - want) <= mine).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. the native step against the float64 oracle step
# ---------------------------------------------------------------------------------------------------------------
def _net(cfg, seed):
    net = hip_hrnet.get_pose_net(cfg, is_train=False)
    sd = synth.synth_state_dict(net.state_dict(), seed=seed)
    net.load_state_dict(sd)
    return net.cuda().train(), sd


def _oracle_step(sd, cfg, x, tgt, jt, spec, weights, **cr):
    """Forward over all crops in float64 (train-mode BatchNorm), the restated loss, backward."""
    orc = HRNetTrainOracle({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, cfg, lr=1e-3)
    maps = hrnet_oracle.hrnet_forward_train(orc.sd, cfg, x.double())
    iw, ih = cfg['heatmapModel']['input_size']
    hm_size = cfg['heatmapModel']['heatmap_size']
    loss, _ = IL.composite_loss_maps(maps, tgt.double(), jt.double(), (iw, ih), hm_size, spec, weights, **cr)
    loss.backward()
    coords = IL.soft_arg_max_norm(maps.detach(), hm_size)                  # all N rows, like last_coords
    return float(loss.detach()), maps.detach(), coords, {k: v.float() for k, v in orc.grads().items()}


def _compare(tr, net, loss, want, loss_rtol, coords_atol=2e-4):
    want_loss, want_maps, want_coords, want_grads = want
    gl2, cos, med = gradient_agreement(dict(net.named_parameters()), want_grads)
    dc = float(np.abs(tr.last_coords.cpu().numpy() - want_coords.numpy()).max())
    print('loss %.8f (oracle %.8f, rel %.2e), coords worst %.2e, gradients rel-L2 %.2e cosine %.6f median %.2e'
          % (loss, want_loss, abs(loss - want_loss) / abs(want_loss), dc, gl2, cos, med))
    assert abs(loss - want_loss) < loss_rtol * abs(want_loss), (loss, want_loss)
    np.testing.assert_allclose(tr.last_maps.cpu().numpy(), want_maps.numpy(), rtol=0, atol=2e-4)
    assert tuple(tr.last_coords.shape) == tuple(want_coords.shape) and dc <= coords_atol, dc
    assert cos > 0.9999 and gl2 < 1e-2 and med < 5e-3, (gl2, cos, med)


def test_step_with_the_coordinate_term_vs_oracle():
    cfg = configs.tiny_config('heatmap')
    net, sd = _net(cfg, seed=5)
    gen = torch.Generator().manual_seed(1)
    x = synth.synth_crops(3, 3, 64, 64, seed=2)
    tgt = torch.rand(3, 5, 16, 16, generator=gen)
    jt = torch.rand(3, 5, 2, generator=gen) * 64
    want = _oracle_step(sd, cfg, x, tgt, jt, ('mse', 'l1', 'None'), (1.0, 0.1, 'None'))
    plain = _oracle_step(sd, cfg, x, tgt, jt, ('mse', 'None', 'None'), (1.0, 0.1, 'None'))[0]
    assert abs(want[0] - plain) > 1e-3 * abs(plain)                        # the term is live
    tr = HRNetTrainStep(net, lr=1e-3, w_coor=0.1)
    loss = float(tr.step(x.cuda(), tgt.cuda(), jt.cuda(), update=False).item())
    _compare(tr, net, loss, want, 2e-5)
    # the default weight trains the term too (it raised before)
    net2, _ = _net(cfg, seed=5)
    loss2 = float(HRNetTrainStep(net2, lr=1e-3).step(x.cuda(), tgt.cuda(), jt.cuda(), update=False).item())
    assert abs(loss2 - loss) <= LOSS_ULPS * abs(loss)


def test_step_with_the_cross_ratio_term_vs_oracle():
    cfg = configs.tiny_config('heatmap', num_joints=33)
    net, sd = _net(cfg, seed=9)
    gen = torch.Generator().manual_seed(4)
    x = synth.synth_crops(3, 3, 64, 64, seed=8)
    tgt = torch.rand(3, 33, 16, 16, generator=gen)
    jt = torch.rand(3, 33, 2, generator=gen) * 64
    thres = _mid_threshold(sd, cfg, x)
    cr = dict(apply_cr_loss=True, cr_indices=get_cr_indices(), cr_loss_thres=thres)
    want = _oracle_step(sd, cfg, x, tgt, jt, ('mse', 'l1', 'sl1'), (1.0, 0.1, 0.05), **cr)
    plain = _oracle_step(sd, cfg, x, tgt, jt, ('mse', 'l1', 'None'), (1.0, 0.1, 'None'))[0]
    assert abs(want[0] - plain) > 1e-3 * abs(plain)
    tr = HRNetTrainStep(net, lr=1e-3, w_coor=0.1, w_cr=0.05, cr_loss_thres=thres)
    tr.apply_cr_loss = True
    loss = float(tr.step(x.cuda(), tgt.cuda(), jt.cuda(), update=False).item())
    _compare(tr, net, loss, want, 2e-3)
    # apply_cr_loss off (the first epoch): the coordinate term alone
    tr.apply_cr_loss = False
    off = float(tr.step(x.cuda(), tgt.cuda(), jt.cuda(), update=False).item())
    assert abs(off - plain) < 2e-5 * abs(plain)


def _mid_threshold(sd, cfg, x, rows=None):
    """A cross-ratio threshold that keeps some lines and drops others, from the oracle's own coordinates: the middle of
    the widest gap in the middle third of the lines' sorted smallest point distances -- no line sits near it, so
    float32 coordinates cannot move one across."""
    orc = HRNetTrainOracle({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, cfg, lr=1e-3)
    with torch.no_grad():
        maps = hrnet_oracle.hrnet_forward_train(orc.sd, cfg, x.double())
    c = IL.soft_arg_max_norm(maps, cfg['heatmapModel']['heatmap_size'])[:rows]
    pts = c[:, torch.as_tensor(get_cr_indices(), dtype=torch.long)]
    d = (pts[:, :, :, None, :] - pts[:, :, None, :, :]).pow(2).sum(-1).sqrt()
    d = torch.where(d == 0, torch.full_like(d, float('inf')), d).flatten(2).min(-1).values
    ds = np.sort(d.numpy().ravel())
    lo, hi = len(ds) // 3, 2 * len(ds) // 3
    i = lo + int(np.argmax(ds[lo + 1:hi + 1] - ds[lo:hi]))
    assert ds[i + 1] - ds[i] > 1e-4 * ds[i], 'no gap to put the threshold in'
    return float(0.5 * (ds[i] + ds[i + 1]))


def test_step_on_a_mixed_batch_vs_oracle():
    """3 crops, 2 labelled.  The reference cuts the maps to the labelled prefix before the soft-arg-max when the
    heat-map term is on (function.py:184-185; tests/golden/integral_loss.npz case 'mixed'): L_2d AND L_cr see the two
    labelled crops, BatchNorm all three, ``last_coords`` keeps three rows."""
    cfg = configs.tiny_config('heatmap', num_joints=33)
    net, sd = _net(cfg, seed=9)
    gen = torch.Generator().manual_seed(4)
    x = synth.synth_crops(3, 3, 64, 64, seed=8)
    tgt = torch.rand(2, 33, 16, 16, generator=gen)
    jt = torch.rand(2, 33, 2, generator=gen) * 64
    thres = _mid_threshold(sd, cfg, x, rows=2)
    cr = dict(apply_cr_loss=True, cr_indices=get_cr_indices(), cr_loss_thres=thres)
    want = _oracle_step(sd, cfg, x, tgt, jt, ('mse', 'l1', 'sl1'), (1.0, 0.1, 0.05), **cr)
    alone = _oracle_step(sd, cfg, x[:2], tgt, jt, ('mse', 'l1', 'sl1'), (1.0, 0.1, 0.05), **cr)[0]
    assert abs(alone - want[0]) > 1e-3 * abs(want[0])                      # the third crop counts (BatchNorm)
    tr = HRNetTrainStep(net, lr=1e-3, w_coor=0.1, w_cr=0.05, cr_loss_thres=thres)
    tr.apply_cr_loss = True
    loss = float(tr.step(x.cuda(), tgt.cuda(), jt.cuda(), update=False).item())
    assert tuple(tr.last_maps.shape) == (3, 33, 16, 16)
    _compare(tr, net, loss, want, 2e-3)


def test_step_on_non_square_maps_vs_oracle():
    cfg = configs.tiny_config('heatmap', input_size=(64, 96))               # W x H: maps 16 wide, 24 high
    net, sd = _net(cfg, seed=5)
    gen = torch.Generator().manual_seed(2)
    x = synth.synth_crops(3, 3, 96, 64, seed=3)
    tgt = torch.rand(3, 5, 24, 16, generator=gen)
    jt = torch.rand(3, 5, 2, generator=gen) * torch.tensor([64.0, 96.0])
    want = _oracle_step(sd, cfg, x, tgt, jt, ('mse', 'l1', 'None'), (1.0, 0.1, 'None'))
    # the quirk is live: dividing each axis by its own size gives another loss
    nat = dict(cfg, heatmapModel=dict(cfg['heatmapModel'], heatmap_size=[24, 16]))
    natural = _oracle_step(sd, nat, x, tgt, jt, ('mse', 'l1', 'None'), (1.0, 0.1, 'None'))[0]
    assert abs(natural - want[0]) > 1e-3 * abs(want[0])
    tr = HRNetTrainStep(net, lr=1e-3, w_coor=0.1)
    loss = float(tr.step(x.cuda(), tgt.cuda(), jt.cuda(), update=False).item())
    _compare(tr, net, loss, want, 2e-5, coords_atol=2e-4 * 24 / 16)


# ---------------------------------------------------------------------------------------------------------------
# 3. terms off: what the step did before
# ---------------------------------------------------------------------------------------------------------------
class _Composite(object):
    """What make_step reads of a JointsCompositeLoss."""

    def __init__(self):
        self.comp_dict = {'hm': (torch.nn.MSELoss(), 1.0), 'coor': (torch.nn.L1Loss(), 0.1),
                          'cr': (torch.nn.SmoothL1Loss(), 0.05)}
        self.cr_indices, self.target_cr, self.cr_loss_thres, self.apply_cr_loss = get_cr_indices(), 4 / 3, 0.15, True


def test_terms_off_is_the_step_built_the_old_way():
    cfg = configs.clone(configs.tiny_config('heatmap', num_joints=33))
    cfg['optimizer'] = {'optim_type': 'adam', 'lr': 1e-3, 'weight_decay': 0.0}
    gen = torch.Generator().manual_seed(1)
    x = synth.synth_crops(3, 3, 64, 64, seed=2).cuda()
    tgt = torch.rand(3, 33, 16, 16, generator=gen).cuda()
    jt = (torch.rand(3, 33, 2, generator=gen) * 64).cuda()
    L = _lib.lib()

    def run(make, joints):
        net, _ = _net(cfg, seed=5)
        tr = make(net)
        tr.step(x, tgt, joints, update=False)                               # first step: packs, allocations
        c0 = L.egn_launch_count()
        loss = tr.step(x, tgt, joints, update=False)
        return L.egn_launch_count() - c0, float(loss.item()), tr, tr.flat.grad.clone(), tr.last_maps.clone()

    old = run(lambda net: HRNetTrainStep(net, lr=1e-3, w_coor=0.0), None)
    assert old[2].last_coords is None
    # a criterion object without the key; a cross-ratio weight whose switch is off
    via_cfg = run(lambda net: trainer.make_step(net, cfg, _Composite(), None), None)
    gated = run(lambda net: HRNetTrainStep(net, lr=1e-3, w_coor=0.0, w_cr=0.05), None)
    for other in (via_cfg, gated):
        assert other[0] == old[0], (other[0], old[0])                       # the same launches
        assert abs(other[1] - old[1]) <= LOSS_ULPS * abs(old[1]), (other[1], old[1])
        assert torch.equal(other[3], old[3]) and torch.equal(other[4], old[4])      # every gradient, bit for bit
        assert other[2].last_coords is None
    on = run(lambda net: HRNetTrainStep(net, lr=1e-3, w_coor=0.1), jt)
    assert on[0] == old[0] + 2 and abs(on[1] - old[1]) > 1e-3 * old[1]      # the two soft-arg-max launches
    assert torch.equal(on[4], old[4]) and not torch.equal(on[3], old[3])


# ---------------------------------------------------------------------------------------------------------------
# 4. trainer.train, and what stays refused
# ---------------------------------------------------------------------------------------------------------------
class _Set(torch.utils.data.Dataset):
    def __init__(self, n=8):
        g = torch.Generator().manual_seed(1)
        self.x = synth.synth_crops(n, 3, 64, 64, seed=3)
        self.t = torch.rand(n, 5, 16, 16, generator=g)
        self.j = torch.cat([torch.rand(n, 5, 2, generator=g) * 64, torch.ones(n, 5, 1)], dim=2)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.t[i], torch.ones(5, 1), {'transformed_joints': self.j[i].numpy()}


def test_trainer_train_with_the_key_matches_the_step_called_directly():
    cfg = configs.clone(configs.tiny_config('heatmap'))
    cfg['heatmapModel'].update(integral_terms=True, loss_spec_list=['mse', 'l1', 'None'],
                               loss_weight_list=[1.0, 0.1, 'None'])
    cfg.update(use_gpu=True, exp_type='test',
               optimizer={'optim_type': 'adam', 'lr': 1e-3, 'weight_decay': 0.0, 'momentum': 0.9,
                          'milestones': [3], 'gamma': 0.5},
               training_settings={'total_epochs': 1, 'batch_size': 4, 'num_threads': 0, 'shuffle': False,
                                  'report_every': 1, 'eval_during': False, 'plot_loss': False})
    data = _Set()
    lg = logging.getLogger('egonet_amd.test_integral_loss')
    lg.handlers = [logging.NullHandler()]
    net, _ = _net(cfg, seed=9)
    optim, _ = trainer.prepare_optim(net, cfg)
    step = trainer.make_step(net, cfg, None, optim)
    assert isinstance(step, HRNetTrainStep) and step.w_coor == 0.1 and step.w_cr is None
    rec = trainer.train(data, net, None, optim, None, cfg, lg)
    assert len(rec['loss']) == 2 and all(np.isfinite(rec['loss']))
    net2, _ = _net(cfg, seed=9)
    optim2, _ = trainer.prepare_optim(net2, cfg)
    direct = trainer.make_step(net2, cfg, None, optim2)
    losses = [float(direct.step(data.x[i:i + 4].cuda(), data.t[i:i + 4].cuda(), data.j[i:i + 4]).item()) for i in (0, 4)]
    np.testing.assert_allclose(rec['loss'], losses, rtol=1e-6)
    # the terms were live: the same net without the key gives another loss
    cfg_off = configs.clone(cfg)
    del cfg_off['heatmapModel']['integral_terms']
    net3, _ = _net(cfg, seed=9)
    off = trainer.make_step(net3, cfg_off, None, None)
    assert off.w_coor == 0.0
    assert abs(float(off.step(data.x[:4].cuda(), data.t[:4].cuda(), None).item()) - losses[0]) > 1e-4 * losses[0]


def test_combinations_that_stay_refused():
    net, _ = _net(configs.tiny_config('heatmap'), seed=5)
    with pytest.raises(NotImplementedError, match='use_target_weight is JointsMSELoss'):
        HRNetTrainStep(net, lr=1e-3, w_coor=0.1, use_target_weight=True)
    with pytest.raises(NotImplementedError, match='use_target_weight is JointsMSELoss'):
        HRNetTrainStep(net, lr=1e-3, w_coor=0.0, w_cr=0.05, use_target_weight=True)
    cfg = configs.tiny_config('heatmap')
    cfg['heatmapModel']['pixel_shuffle'] = True
    cfg['heatmapModel']['heatmap_size'] = [32, 32]
    ps, _ = _net(cfg, seed=5)
    for kw in (dict(), dict(w_coor=0.0, w_cr=0.05)):                        # the default w_coor = 0.1 still raises here
        with pytest.raises(NotImplementedError, match='pixel-shuffle'):
            HRNetTrainStep(ps, lr=1e-3, **kw)
    # the coordinate term needs its ground truth
    tr = HRNetTrainStep(net, lr=1e-3, w_coor=0.1)
    with pytest.raises(ValueError, match='needs joints_xy'):
        tr.step(synth.synth_crops(2, 3, 64, 64, seed=1).cuda(), torch.rand(2, 5, 16, 16).cuda(), None, update=False)
