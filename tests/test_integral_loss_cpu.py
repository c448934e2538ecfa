"""The heat-map head's integral terms without a GPU.

1. The float64 restatement of libs/loss/function.py:170-202 for a heat-maps-only model (tests/integral_loss.py)
   against the REFERENCE's JointsCompositeLoss (tests/golden/integral_loss.npz: square, non-square, L_cr, mixed batch).
2. The host twins of csrc/softargmax.hip (egn_softargmax_fwd/bwd_host_f32, the text the kernels run) against the
   float64 soft-arg-max: |error| <= C x 2^-24 x the sum of absolute terms of each output (+ float32's underflow floor),
   C = 4 x the worst ratio an fp32 emulation of the kernel's summation order measures (held here).
3. The edge cases of the kernels' arithmetic, and every refused argument of the four entry points.
4. ``trainer.make_step``: heatmapModel.integral_terms switches the terms, a criterion alone does not; the tool's flag.
"""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import integral_loss as IL
from conftest import golden
from egonet_amd import _lib, configs, softargmax, trainer
from egonet_amd.model.heatmapModel import hrnet as hip_hrnet


# ---------------------------------------------------------------------------------------------------------------
# 1. the restatement against the reference
# ---------------------------------------------------------------------------------------------------------------
def _fixture_case(name):
    g = golden('integral_loss.npz')
    c = json.loads(str(g['cases']))[name]
    p = name + '/'
    return g, c, {k: g[p + k] for k in ('maps', 'target', 'joints', 'loss', 'dmaps')}


def _restated(g, c, a, hm_size=None):
    maps = torch.from_numpy(a['maps']).double().requires_grad_(True)
    h, w = c['h'], c['w']
    loss, coords = IL.composite_loss_maps(
        maps, torch.from_numpy(a['target']).double(), torch.from_numpy(a['joints']).double(), (4 * w, 4 * h),
        hm_size or [w, h], c['spec'], c['weights'], apply_cr_loss=c['spec'][2] != 'None',
        cr_indices=g['bbox12'].tolist(), cr_loss_thres=c.get('thres', 0.15))
    loss.backward()
    return float(loss.detach()), maps.grad.numpy(), coords


@pytest.mark.parametrize('name', ['sq', 'nsq', 'cr', 'mixed'])
def test_restatement_reproduces_the_reference_fixture(name):
    """Tolerances = float32 noise of the reference's own arithmetic, from the fixture's magnitudes.  The loss (0.36 ..
    0.97) is a handful of float32 means over <= 6 336 elements, pairwise: 1e-6 relative is ~16 x 2^-24.  The gradient
    entries (largest 1.2e-3 .. 1.1e-2) are sums of three terms, the cross-ratio one through differences of coordinates
    0.1 .. 1 apart: 1e-5 of the largest entry (~170 x 2^-24; 1.6e-6 is what the four cases show)."""
    g, c, a = _fixture_case(name)
    loss, grad, _ = _restated(g, c, a)
    print('%s: loss %.9f (reference %.9f), worst gradient difference %.2e of the largest entry %.2e'
          % (name, loss, float(a['loss']), float(np.abs(grad - a['dmaps']).max()), float(np.abs(a['dmaps']).max())))
    assert abs(loss - float(a['loss'])) <= 1e-6 * abs(float(a['loss']))
    assert float(np.abs(grad - a['dmaps']).max()) <= 1e-5 * float(np.abs(a['dmaps']).max())


def test_fixture_pins_the_divisor_quirk_and_the_prefix_cut():
    # non-square maps: x / hm_size[1] = h, y / hm_size[0] = w; the natural order gives another loss
    g, c, a = _fixture_case('nsq')
    swapped = _restated(g, c, a, hm_size=[c['h'], c['w']])[0]
    assert abs(swapped - float(a['loss'])) > 1e-3 * float(a['loss'])
    # the mixed batch: the maps are cut to the labelled prefix before the soft-arg-max, so the unlabelled crop gets no
    # gradient at all -- L_cr (on in this case, lines kept and lines dropped) included
    g, c, a = _fixture_case('mixed')
    assert (c['n'], c['n_fs']) == (3, 2) and not a['dmaps'][2:].any() and a['dmaps'][:2].any()
    for name in ('cr', 'mixed'):
        m = g[name + '/cr_mask']
        assert 0 < m.sum() < m.size, name


# ---------------------------------------------------------------------------------------------------------------
# 2. the host twins within the derived bound
# ---------------------------------------------------------------------------------------------------------------
def test_bound_constant_is_four_times_the_emulation():
    got = IL.measure_ratio()
    print('fp32 emulation of the summation order, worst ratio: forward %.2f backward %.2f' % (got['fwd'], got['bwd']))
    for k in ('fwd', 'bwd'):
        assert got[k] <= IL.MEASURED_RATIO[k] <= 1.01 * got[k] + 0.01, (k, got[k], IL.MEASURED_RATIO[k])
        assert IL.C_BOUND[k] == math.ceil(4 * IL.MEASURED_RATIO[k]), k


def _host(z, K, g, div_x, div_y, accumulate=False, base=None, n_rows=None):
    coords, save = softargmax.forward_host(z, K, div_x, div_y)
    dz = np.full(z.shape, -7777.0, np.float32) if base is None else base.copy()
    softargmax.backward_host(z, save, g, div_x, div_y, dz, n_rows=n_rows, accumulate=accumulate)
    return coords, save, dz


@pytest.mark.parametrize('case', IL.SWEEP_CASES)
def test_host_twins_vs_float64_within_the_bound(case):
    n, K, h, w, cs, _ = case
    z, g = IL.sweep_inputs(case)                       # pad channels hold NaN: never read
    coords, save, dz = _host(z, K, g, float(h), float(w))
    assert np.isfinite(coords).all() and np.isfinite(save).all() and np.isfinite(dz[..., :K]).all()
    assert (dz[..., K:] == -7777.0).all()              # pad channels: never written
    rf, rb = IL.ratios(coords, dz[..., :K], z, K, float(h), float(w), g)
    print('%s: worst ratio forward %.2f (bound %g) backward %.2f (bound %g)' % (case, rf, IL.C_BOUND['fwd'], rb,
                                                                                IL.C_BOUND['bwd']))
    assert rf <= IL.C_BOUND['fwd'] and rb <= IL.C_BOUND['bwd']
    # save = (ex, ey, max, sum e): pixels, the exact maximum, a normaliser in [1, h w]
    np.testing.assert_array_equal(save[..., 2], z[..., :K].max(axis=(1, 2)))
    assert (save[..., 3] >= 1.0).all() and (save[..., 3] <= h * w * (1 + 1e-6)).all()
    np.testing.assert_array_equal(coords[..., 0], save[..., 0] / np.float32(h))
    # accumulate: old + new, one rounding
    base = np.random.RandomState(3).randn(*z.shape).astype(np.float32)
    acc = _host(z, K, g, float(h), float(w), accumulate=True, base=base)[2]
    np.testing.assert_array_equal(acc[..., :K], base[..., :K] + dz[..., :K])
    np.testing.assert_array_equal(acc[..., K:], base[..., K:])
    # equal inputs, equal bits
    again = _host(z, K, g, float(h), float(w))
    assert np.array_equal(again[0], coords) and np.array_equal(again[2][..., :K], dz[..., :K])


def test_host_forward_on_the_reference_fixture_uses_the_swapped_divisors():
    g, c, a = _fixture_case('nsq')
    h, w = c['h'], c['w']
    want = IL.soft_arg_max_norm(torch.from_numpy(a['maps']).double(), [w, h]).numpy()
    z = IL.to_nhwc(a['maps'], 8, fill=np.nan)
    coords, _ = softargmax.forward_host(z, c['k'], float(h), float(w))       # div_x = hm_size[1], div_y = hm_size[0]
    assert float(np.abs(coords - want).max()) <= IL.C_BOUND['fwd'] * IL.EPS * float(np.abs(want).max())


# ---------------------------------------------------------------------------------------------------------------
# 3. edge cases and refusals
# ---------------------------------------------------------------------------------------------------------------
def test_one_pixel_and_two_by_two_maps():
    z = np.full((1, 1, 1, 4), np.nan, np.float32)
    z[..., 0] = 3.5
    coords, save, dz = _host(z, 1, np.ones((1, 1, 2), np.float32), 1.0, 1.0)
    assert coords.tolist() == [[[0.0, 0.0]]] and save.tolist() == [[[0.0, 0.0, 3.5, 1.0]]] and dz[0, 0, 0, 0] == 0.0
    z = np.full((1, 2, 2, 4), np.nan, np.float32)
    z[0, :, :, 0] = [[0.0, 0.0], [0.0, math.log(3.0)]]           # weights 1 1 1 3 (to rounding) / 6
    coords, save, _ = _host(z, 1, np.ones((1, 1, 2), np.float32), 2.0, 2.0)
    np.testing.assert_allclose(coords[0, 0], [4.0 / 6 / 2, 4.0 / 6 / 2], rtol=4 * IL.EPS)
    assert save[0, 0, 2] == np.float32(math.log(3.0))


def test_single_joint_and_pad_channels_keep_their_sentinel():
    rng = np.random.RandomState(0)
    for K, cs in ((1, 4), (5, 8)):
        z = np.full((2, 6, 5, cs), np.nan, np.float32)
        z[..., :K] = rng.randn(2, 6, 5, K)
        g = rng.randn(2, K, 2).astype(np.float32)
        for accumulate in (False, True):
            base = np.full(z.shape, -7777.0, np.float32)
            base[..., :K] = 1.0
            dz = _host(z, K, g, 6.0, 5.0, accumulate=accumulate, base=base)[2]
            assert (dz[..., K:] == -7777.0).all() and np.isfinite(dz[..., :K]).all()
        want, _, _ = IL.softargmax64(z, K, 6.0, 5.0)
        np.testing.assert_allclose(_host(z, K, g, 6.0, 5.0)[0], want, rtol=IL.C_BOUND['fwd'] * IL.EPS)


def test_huge_logits_stay_finite():
    rng = np.random.RandomState(1)
    z = np.zeros((1, 8, 8, 4), np.float32)
    z[..., :2] = np.where(rng.rand(1, 8, 8, 2) > 0.5, 1e4, -1e4)
    z[0, 3, 5, 2] = 1e4                                            # one hot pixel among zeros
    z[..., 3] = -1e4                                               # a constant map far below zero
    g = np.ones((1, 4, 2), np.float32)
    coords, save, dz = _host(z, 4, g, 8.0, 8.0)
    assert np.isfinite(coords).all() and np.isfinite(save).all() and np.isfinite(dz).all()
    np.testing.assert_array_equal(coords[0, 2], [5.0 / 8, 3.0 / 8])             # the others weigh e^-10000 = 0
    np.testing.assert_array_equal(coords[0, 3], [3.5 / 8, 3.5 / 8])
    hot = z[0, :, :, 0] == 1e4                                     # the mean position of the pixels at +1e4
    ys, xs = np.nonzero(hot)
    np.testing.assert_allclose(coords[0, 0], [xs.mean() / 8, ys.mean() / 8], rtol=8 * IL.EPS)


def test_constant_map_gives_the_centre_and_a_gradient_that_cancels():
    """A constant map: every weight is exactly 1 / (h w), the sums of small integers are exact -- the coordinates are
    the centre to the last bit, d maps is exactly antisymmetric about it (so its sum is exactly zero), and zero
    dcoords give an exactly zero gradient."""
    h, w = 6, 8
    z = np.full((1, h, w, 4), 2.5, np.float32)
    g = np.array([[[0.7, -1.3]]], np.float32)
    coords, save, dz = _host(z, 1, g, float(h), float(w))
    assert coords[0, 0].tolist() == [np.float32(3.5) / np.float32(h), np.float32(2.5) / np.float32(w)]
    assert save[0, 0].tolist() == [3.5, 2.5, 2.5, float(h * w)]
    d = dz[0, :, :, 0]
    assert d.any() and np.array_equal(d, -d[::-1, ::-1]) and float(d.astype(np.float64).sum()) == 0.0
    assert not _host(z, 1, np.zeros((1, 1, 2), np.float32), float(h), float(w))[2][..., 0].any()


@pytest.mark.parametrize('case', IL.SWEEP_CASES[:4])
def test_gradient_of_a_map_sums_to_zero_within_the_bound(case):
    """sum_p s_p (x_p - ex) = 0: the softmax Jacobian's rows cancel.  The float32 outputs cancel to within the sum of
    their own bounds."""
    n, K, h, w, cs, _ = case
    z, g = IL.sweep_inputs(case)
    dz = _host(z, K, g, float(h), float(w))[2][..., :K]
    _, mag = IL.softargmax_bwd64(z, K, float(h), float(w), g)
    floor = IL.underflow_floor(z, K, float(h), float(w), g)[1]
    total = np.abs(dz.astype(np.float64).sum(axis=(1, 2)))
    assert (total <= (IL.C_BOUND['bwd'] * IL.EPS * mag + floor).sum(axis=(1, 2))).all()


def test_n_rows_leaves_the_tail_untouched():
    case = (3, 5, 7, 6, 8, 2.0)
    z, g = IL.sweep_inputs(case)
    z[2] = np.nan                                                  # rows beyond n_rows are not read either
    zf = np.nan_to_num(z)
    coords, save = softargmax.forward_host(zf, 5, 7.0, 6.0)
    base = np.full(z.shape, -7777.0, np.float32)
    for accumulate in (False, True):
        dz = softargmax.backward_host(z, save, g, 7.0, 6.0, base.copy(), n_rows=2, accumulate=accumulate)
        full = softargmax.backward_host(zf, save, g, 7.0, 6.0, base.copy(), accumulate=accumulate)
        assert (dz[2] == -7777.0).all() and np.array_equal(dz[:2], full[:2]) and np.isfinite(full).all()
        assert (full[..., :5] != -7777.0).any(axis=(1, 2, 3)).all()
    assert (softargmax.backward_host(z, save, g, 7.0, 6.0, base.copy(), n_rows=0) == -7777.0).all()


def test_every_refused_argument():
    L = _lib.lib()
    z = np.zeros((2, 4, 4, 8), np.float32)
    coords, save = np.zeros((2, 5, 2), np.float32), np.zeros((2, 5, 4), np.float32)
    g, dz = np.ones((2, 5, 2), np.float32), np.zeros_like(z)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + off)           # noqa: E731
    ok_f = dict(z=P(z), N=2, h=4, w=4, K=5, cs=8, div_x=4.0, div_y=4.0, coords=P(coords), save=P(save))
    ok_b = dict(z=P(z), save=P(save), dcoords=P(g), N=2, n_rows=2, h=4, w=4, K=5, cs=8, div_x=4.0, div_y=4.0,
                accumulate=1, dz=P(dz))
    shape_bad = [dict(N=0), dict(K=0), dict(K=9), dict(cs=6, K=5), dict(h=0), dict(w=0), dict(div_x=0.0),
                 dict(div_y=-1.0), dict(div_x=float('nan'))]
    bad_f = shape_bad + [dict(z=None), dict(coords=None), dict(save=None), dict(z=P(z, 4)), dict(coords=P(coords, 4)),
                         dict(save=P(save, 8))]
    bad_b = shape_bad + [dict(z=None), dict(save=None), dict(dcoords=None), dict(dz=None), dict(z=P(z, 4)),
                         dict(dz=P(dz, 8)), dict(save=P(save, 4)), dict(dcoords=P(g, 4)), dict(n_rows=-1),
                         dict(n_rows=3)]
    # the device entry points refuse before they touch the runtime: no GPU needed, the launch count does not move
    c0 = L.egn_launch_count()
    for host in (True, False):
        fwd = L.egn_softargmax_fwd_host_f32 if host else L.egn_softargmax_fwd_f32
        bwd = L.egn_softargmax_bwd_host_f32 if host else L.egn_softargmax_bwd_f32
        tail = () if host else (None,)
        for bad in bad_f:
            assert fwd(*dict(ok_f, **bad).values(), *tail) == -1, (host, bad)
        for bad in bad_b:
            assert bwd(*dict(ok_b, **bad).values(), *tail) == -1, (host, bad)
    assert L.egn_launch_count() == c0
    assert L.egn_softargmax_fwd_host_f32(*ok_f.values()) == 0 and L.egn_softargmax_bwd_host_f32(*ok_b.values()) == 0


# ---------------------------------------------------------------------------------------------------------------
# 4. the opt-in
# ---------------------------------------------------------------------------------------------------------------
class _Criterion(object):
    """What make_step reads of a JointsCompositeLoss (function.py:61-93, train_IGRs.py:33-46)."""

    def __init__(self):
        self.comp_dict = {'hm': (torch.nn.MSELoss(), 1.0), 'coor': (torch.nn.SmoothL1Loss(), 0.2),
                          'cr': (torch.nn.SmoothL1Loss(), 0.05)}
        self.cr_indices, self.target_cr, self.cr_loss_thres = [[0, 1, 2, 3]], 4.0 / 3.0, 0.1
        self.apply_cr_loss = True


def _made_step(monkeypatch, cfg, loss_func):
    made = {}

    class Recorder(object):
        def __init__(self, model, **kw):
            made.update(kw)

    monkeypatch.setattr(trainer, 'HRNetTrainStep', Recorder)
    net = hip_hrnet.get_pose_net(cfg, is_train=False)
    step = trainer.make_step(net, cfg, loss_func, None)
    return made, step


def test_make_step_switches_the_terms_by_the_key_alone(monkeypatch):
    base = configs.clone(configs.tiny_config('heatmap'))
    base['optimizer'] = {'optim_type': 'adam', 'lr': 1e-3}
    # no key: today's behaviour, whatever the criterion or the weight lists say
    for loss_func in (None, _Criterion()):
        cfg = configs.clone(base)
        cfg['heatmapModel'].update(loss_spec_list=['mse', 'l1', 'sl1'], loss_weight_list=[1.0, 0.1, 0.05])
        made, _ = _made_step(monkeypatch, cfg, loss_func)
        assert made['w_coor'] == 0.0 and 'w_cr' not in made and 'coor_type' not in made and 'cr_indices' not in made
    # the key: the weights are read as for the coordinate head, apply_cr_loss from the criterion
    cfg = configs.clone(base)
    cfg['heatmapModel']['integral_terms'] = True
    made, step = _made_step(monkeypatch, cfg, _Criterion())
    assert (made['w_hm'], made['w_coor'], made['w_cr']) == (1.0, 0.2, 0.05)
    assert made['coor_type'] == 'sl1' and made['cr_type'] == 'sl1' and made['cr_indices'] == [[0, 1, 2, 3]]
    assert made['cr_loss_thres'] == 0.1 and made['use_target_weight'] is False and step.apply_cr_loss is True
    # ... or from the config's lists
    cfg['heatmapModel'].update(loss_spec_list=['mse', 'l1', 'None'], loss_weight_list=[1.0, 0.3, 'None'])
    made, step = _made_step(monkeypatch, cfg, None)
    assert made['w_coor'] == 0.3 and 'w_cr' not in made and step.apply_cr_loss is False


def test_integral_terms_key_parsing():
    for v, want in ((True, True), (False, False), (1, True), (0, False), ('true', True), ('False', False), ('on', True),
                    (None, False)):
        assert trainer.integral_terms({'heatmapModel': {'integral_terms': v}}) is want, v
    assert trainer.integral_terms({}) is False and trainer.integral_terms({'heatmapModel': {}}) is False
    with pytest.raises(ValueError, match='integral_terms'):
        trainer.integral_terms({'heatmapModel': {'integral_terms': 'maybe'}})


def test_tool_flag_selects_the_heat_map_head_and_sets_the_key():
    from tools import train_IGRs as tool
    import argparse
    a = argparse.Namespace(tiny=True, exp_type='instanceto2d', cr_weight=0.05, lr=1e-3, epochs=1, batch_frames=2,
                           workers=0, report_every=1, eval_every=0, integral_terms=True)
    cfg = tool.igr_cfgs(a)
    assert cfg['heatmapModel']['integral_terms'] is True and cfg['heatmapModel']['head_type'] == 'heatmap'
    assert cfg['heatmapModel']['loss_weight_list'] == [1.0, 0.1, 0.05]
    a.integral_terms = False
    cfg = tool.igr_cfgs(a)
    assert 'integral_terms' not in cfg['heatmapModel'] and cfg['heatmapModel']['head_type'] == 'coordinates'
