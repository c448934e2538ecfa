"""The convolution requests the product makes, and every tile configuration the tuner could answer each with.

Helper module of tests/test_gpu_conv_sweep.py and tests/test_conv_sweep_cpu.py (imported, not a conftest).
``tuner.choose`` keeps whichever of ``tuner.candidates`` MEASURED fastest, so every one of them has to compute its
convolution correctly -- not only the ones the shipped table names.  No hand-written shape list, no rule restated:
the requests are the product's recordings, each with what its caller told the tuner; the tuner's predicate does the rest.

A request is a dict:
  key      the ``tuner.shape_key`` arguments (n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, nchw)
  act      the epilogue activation (EGN_ACT_* | EGN_ACT_RES_AFTER)
  entry    'program' (egn_program_add_conv2d: the inference engine), 'tape' (train_hrnet._Tape._conv_launch:
           egn_conv2d_ex_f32 / egn_conv2d_bnstats_f32 / egn_conv2d_f32 by configuration) or 'conv2d'
           (egn_conv2d_f32 with a tuner-chosen configuration: the 4x3 GEMM of the pedestrian data gradient, the
           lifter's row GEMMs)
  kinds, ticket_cap, inplace_res: as the caller passed them to ``tuner.choose`` (the filter kinds it packs, the
           ticket words it owns, whether it said that the residual is y)
  alias    the launch reads its residual from y itself (the tape's in-place data-gradient add)
  stats    the caller asks for fused BatchNorm statistics (the tape's BatchNorm layers without a bias)
  src      where it was seen (model / batch / layer tag)
"""
import inspect
import os

import numpy as np
import torch

from egonet_amd import _lib, configs, engine, tuner

U = 2.0 ** -24      # unit roundoff of fp32

# |y - y64| <= C_BOUND[kind] * U * A, A = the same computation on |x|, |w|, |scale|, |shift|, |res|.
# Calibrated on the CPU with the fp32 emulation of tools/wino43_error_study.py (conv_direct in fp32; conv_wino with
# mats([0, 1, -1]) / mats([0, 1, -1, 2, -2])) on HRNet-like 3x3 layers fed by ``act_like`` (post-ReLU maps with x30
# spikes, filters ~ N(0, 1/(9 Cin))): Cin 16..192, 16 x 16 and 32 x 32 maps, 28 layers per kind.  Worst ratio
# measured: direct 4.3, F(2x2,3x3) 14.8, F(4x4,3x3) 373 (Cin 16: the fewest terms to average the transform error of
# a spike over).  The constants are about 4x those.  A TF32 slip (10-bit mantissas) measures 2 900 - 7 900 on the same
# layers: every constant stays below it.
C_BOUND = {0: 18.0, 1: 60.0, 3: 1500.0}
KIND_NAMES = {0: 'direct', 1: 'F(2x2,3x3)', 3: 'F(4x4,3x3)'}


def _request(key, act, entry, kinds, ticket_cap=None, inplace_res=False, alias=False, stats=False, src=''):
    return dict(key=tuple(int(v) if not isinstance(v, bool) else v for v in key), act=int(act), entry=entry,
                kinds=frozenset(kinds), ticket_cap=ticket_cap, inplace_res=bool(inplace_res), alias=bool(alias),
                stats=bool(stats), src=src)


# ---------------------------------------------------------------------------------------------------------------
# inference programs (host only)
# ---------------------------------------------------------------------------------------------------------------
def _pixshuf_config(f):
    cfg = configs.w48_config('heatmap')
    cfg['heatmapModel']['pixel_shuffle'] = True
    cfg['heatmapModel']['heatmap_size'] = [64 * f, 64 * f]
    return cfg


INFERENCE_MODELS = [
    ('w48-heatmap', lambda: configs.w48_config('heatmap'), (1, 3)),
    ('w48-coordinates', lambda: configs.w48_config('coordinates'), (1, 3, 20, 70)),    # 20, 70: not in the table
    ('ped', lambda: configs.ped_config(), (1, 3)),
    ('w48-pixshuf2', lambda: _pixshuf_config(2), (1, 3)),
    ('w48-pixshuf4', lambda: _pixshuf_config(4), (1, 3)),
    ('angle', lambda: configs.tiny_config('angleregression', input_size=(256, 256)), (1, 3)),
    ('tiny', lambda: configs.tiny_config(), (1, 3)),
]
LIFTER_BATCHES = (1, 7, 100)


def _program_requests(rec, src):
    out = []
    for kind, op in rec.ops:
        if kind != 'conv':
            continue
        # (what engine.Program._choose_and_pack passes to tuner.choose)
        out.append(_request(engine.Program._conv_key(op), op['act'], 'program', engine.Program._conv_kinds(op),
                            alias=op['res'] is not None and op['res'] is op['y'], src='%s:%s' % (src, op['tag'])))
    return out


def inference_requests():
    from egonet_amd.model.heatmapModel import hrnet
    from egonet_amd.model import FCmodel
    reqs = []
    with torch.no_grad():
        for name, mk, batches in INFERENCE_MODELS:
            cfg = mk()
            net = hrnet.get_pose_net(cfg, is_train=False).eval()
            eng = engine.HRNetEngine(net)
            iw, ih = cfg['heatmapModel']['input_size']
            for n in batches:
                rec, _, _ = eng._record(n, 3, ih, iw, None)
                reqs += _program_requests(rec, '%s/b%d' % (name, n))
            del net, eng
        lifter = FCmodel.get_fc_model(1, configs.w48_config(), 66, 96).eval()
        eng = engine.LifterEngine(lifter)
        for n in LIFTER_BATCHES:
            reqs += _program_requests(eng._record(n), 'lifter/b%d' % n)
    return reqs


# ---------------------------------------------------------------------------------------------------------------
# training tape (GPU): the requests of real steps
# ---------------------------------------------------------------------------------------------------------------
class TapeRecorder(object):
    """Context manager: records every ``tuner.choose`` call of a training step as a request.  ``_Tape._conv_launch``
    (forward and data-gradient convolutions of the HRNet tape) is wrapped only for what the tuner never sees: the
    activation, fused statistics, a residual, forward or data gradient.  A call from anywhere else (the pedestrian
    4x3 data-gradient GEMM, the lifter's row GEMMs) is a plain egn_conv2d_f32."""

    def __init__(self, src=''):
        self.src = src
        self.reqs = []
        self._launch = None

    def __enter__(self):
        from egonet_amd import train_hrnet as T
        self._T = T
        self._orig = (T._Tape._conv_launch, tuner.choose)
        orig_launch, orig_choose = self._orig
        me = self

        def named(fn, args, kw):
            call = inspect.signature(fn).bind(*args, **kw)
            call.apply_defaults()
            return call.arguments

        def conv_launch(*args, **kw):
            c = named(orig_launch, args, kw)
            if c['res'] is not None and c['res'].data_ptr() != c['y'].data_ptr():
                raise AssertionError('the tape passes a residual only as the in-place gradient add')
            me._launch = dict(act=c['act'], entry='tape', has_res=c['res'] is not None,
                              stats=c['want_stats'] and c['self'].o.fuse_bn_stats, src='dgrad' if c['dgrad'] else 'fwd')
            try:
                return orig_launch(*args, **kw)
            finally:
                me._launch = None

        def choose(*args, **kw):
            c = named(orig_choose, args, kw)
            key = tuple(c['key'])
            at = me._launch or dict(act=engine.ACT_NONE, entry='conv2d', has_res=key[11], stats=False, src='choose')
            me.reqs.append(_request(key[:11] + (at['has_res'], key[12]), at['act'], at['entry'], c['kinds'],
                                    c['ticket_cap'], c['inplace_res'], alias=c['inplace_res'], stats=at['stats'],
                                    src='%s:%s' % (me.src, at['src'])))
            return orig_choose(*args, **kw)

        T._Tape._conv_launch = conv_launch
        tuner.choose = choose
        return self

    def __exit__(self, *exc):
        self._T._Tape._conv_launch, tuner.choose = self._orig
        return False


def tape_requests(device='cuda'):
    """One ``HRNetTrainStep.step(update=False)`` of W48 'coordinates' at 3 crops, the pedestrian model at 2 and the
    pixel-shuffle head at 2; one lifter step at a ragged 30 rows."""
    g = torch.Generator().manual_seed(0)
    # (only which requests are made matters here, not what the tuner answers: no timing of shapes off the table)
    prev = os.environ.get('EGONET_AMD_AUTOTUNE')
    os.environ['EGONET_AMD_AUTOTUNE'] = '0'
    try:
        reqs = _tape_steps(device, g)
    finally:
        if prev is None:
            del os.environ['EGONET_AMD_AUTOTUNE']
        else:
            os.environ['EGONET_AMD_AUTOTUNE'] = prev
    return reqs


def hrnet_run(cfg, n, device, g, update=False, **step_kw):
    """Builds an ``HRNetTrainStep`` of ``cfg`` and its batch of ``n`` crops; returns (step object, step()): one native
    iteration per call."""
    from egonet_amd.model.heatmapModel import hrnet
    from egonet_amd.train_hrnet import HRNetTrainStep
    net = hrnet.get_pose_net(cfg, is_train=False).to(device).train()
    iw, ih = cfg['heatmapModel']['input_size']
    hw, hh = cfg['heatmapModel']['heatmap_size']
    J = cfg['heatmapModel']['num_joints']
    x = torch.randn(n, 3, ih, iw, generator=g).to(device)
    tgt = torch.rand(n, J, hh, hw, generator=g).to(device)
    jxy = (torch.rand(n, J, 2, generator=g) * iw).to(device)
    tr = HRNetTrainStep(net, lr=1e-3, w_coor=0.0 if net.head_type == 'heatmap' else 0.1, **step_kw)
    return tr, lambda: tr.step(x, tgt, None if net.pixel_shuffle else jxy, update=update)


def lifter_run(rows, device, g, update=False, leaky=False, **step_kw):
    """The same for the lifter (66 -> 96) at ``rows`` rows."""
    from egonet_amd.model import FCmodel
    from egonet_amd.train_lifter import LifterTrainStep
    cfg = configs.w48_config()
    cfg['FCModel'] = dict(cfg['FCModel'], leaky=leaky)
    lifter = FCmodel.get_fc_model(1, cfg, 66, 96).to(device).train()
    tr = LifterTrainStep(lifter, lr=1e-3, **step_kw)
    x, t = torch.randn(rows, 66, generator=g).to(device), torch.randn(rows, 96, generator=g).to(device)
    return tr, lambda: tr.step(x, t, update=update)


# The recorded training steps, ONE list for the conv sweep and the training-ops sweep (tests/train_ops_sweep.py):
# (where it is seen, make(device, g) -> (step object, step())).  W48 'coordinates' at 3 crops, the pedestrian model at
# 2, the pixel-shuffle head at 2; the lifter at a ragged 30 rows.
TAPE_STEPS = [
    ('train-w48/b3', lambda device, g: hrnet_run(configs.w48_config('coordinates'), 3, device, g)),
    ('train-ped/b2', lambda device, g: hrnet_run(configs.ped_config(), 2, device, g)),
    ('train-pixshuf/b2', lambda device, g: hrnet_run(_pixshuf_config(2), 2, device, g)),
    ('train-lifter/b30', lambda device, g: lifter_run(30, device, g)),
]


def _tape_steps(device, g):
    reqs = []
    for src, make in TAPE_STEPS:
        tr, step = make(device, g)
        with TapeRecorder(src) as rec:
            step()
        torch.cuda.synchronize()
        reqs += rec.reqs
        del tr, step
    return reqs


# ---------------------------------------------------------------------------------------------------------------
# candidates
# ---------------------------------------------------------------------------------------------------------------
def bnstats_rows(key, cfg):
    n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, nchw = key
    return _lib.lib().egn_conv2d_bnstats_rows(n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, cfg)


def pairs(reqs):
    """[(request, cfg)] without duplicate (key, act, entry, aliasing, statistics, candidate) tuples."""
    seen, out = {}, []
    for r in reqs:
        for cfg in tuner.candidates(r['key'], r['kinds'], r['ticket_cap'], r['inplace_res']):
            t = (r['key'], r['act'], r['entry'], r['alias'], r['stats'], cfg)
            if t in seen:
                seen[t]['srcs'].append(r['src'])
                continue
            p = dict(r, cfg=cfg, srcs=[r['src']])
            seen[t] = p
            out.append(p)
    return out


# ---------------------------------------------------------------------------------------------------------------
# inputs and the bound
# ---------------------------------------------------------------------------------------------------------------
def act_like(n, h, w, c, cs, gen, device='cpu'):
    """NHWC [n, h, w, cs] fp32 shaped like an activation: post-ReLU (non-negative, non-zero mean) with a few x30
    spikes per map, pad channels zero."""
    x = torch.relu(torch.randn(n, h, w, c, generator=gen) + 0.3)
    p = min(3.0 / (h * w), 1.0 / 16)
    m = torch.rand(n, h, w, c, generator=gen) < p
    x[m] = 30.0 * (0.5 + torch.rand(int(m.sum()), generator=gen))
    out = torch.zeros(n, h, w, cs)
    out[..., :c] = x
    return out.to(device)


def filt(cout, cin, kh, kw, gen):
    return torch.randn(cout, cin, kh, kw, generator=gen) / float(np.sqrt(cin * kh * kw))


def ratio(got, want, A):
    """|got - want| / (U A) elementwise (float64); an element with A = 0 must be exact."""
    err = (got.double() - want).abs()
    return torch.where(A > 0, err / (U * A.clamp_min(1e-300)), torch.where(err > 0, float('inf'), 0.0))


def bound_A(x64, w64, stride, pad, scale, shift, res, act):
    """The bound's A: the convolution and epilogue on absolute values (train_checks.conv_ref64); a sigmoid output also
    carries its own rounding (|sigmoid| <= 1), every other activation is 1-Lipschitz."""
    from train_checks import conv_ref64
    A = conv_ref64(x64.abs(), w64.abs(), stride, pad, None if scale is None else scale.abs(),
                   None if shift is None else shift.abs(), None if res is None else res.abs(), engine.ACT_NONE)
    return A + 1.0 if (act & 0xf) == engine.ACT_SIGMOID else A
