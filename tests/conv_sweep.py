"""The convolution requests the product makes, and every tile configuration the tuner could answer each with.

Helper module of tests/test_gpu_conv_sweep.py and tests/test_conv_sweep_cpu.py (imported, not a conftest).
``tuner.choose`` keeps whichever of ``tuner.candidates`` MEASURED fastest, so every one of them has to compute its
convolution correctly -- not only the ones the shipped table names.  Two sources of requests, no rule restated:
  * the product's recordings (``inference_requests``, ``tape_requests``), each with what its caller told the tuner;
  * ``edge_requests``: a hand-written list, per kernel family the smallest shapes that reach the edges of its tile
    mapping -- the planner accepts far more than HRNet records --, each with ``line`` (file under egonet_amd/csrc, the
    text of the line it is there for), ``why`` and ``family``.
The tuner's predicate does the rest (``pairs``).  ``edge_classes`` computes from egn_conv_plan_query which edges a
(request, config) pair stands on; ``FAMILY_CLASSES`` / ``NOT_REACHABLE`` say what each family admits, and the tests
require every selectable config in every admitted class.  ``refusal_requests``: one step outside each predicate.

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
import ctypes as C
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
# On the inputs of the edge list (tests/test_conv_sweep_cpu.py, the same emulations on ``draw`` of every edge request;
# the Winograd ones on the first 4 images), worst ratio: direct 11.59 (259 x 16 x 32, 16 -> 48: 6.4 M outputs, the tail
# of many more elements than a calibration layer has), F(2x2,3x3) 14.49 (1 x 16 x 16, 16 -> 48), F(4x4,3x3) 325
# (3 x 8 x 8, 32 -> 48).  All inside the unchanged constants; the direct one is above a third of its constant on the
# requests the CPU test names.
# Measured on the MI355X (256 CUs) on the edge list, worst ratio: direct 14.49 (cfg 0 - 30 alike, 259 x 16 x 16,
# 32 -> 96 with residual + ReLU), F(2x2,3x3) 31.04 (cfg 62, 259 x 16 x 32, 16 -> 48, statistics), F(4x4,3x3) 569.8
# (cfg 82, 1029 x 8 x 8, 32 -> 48, statistics); Stem 4.36, Fc 4.23, S2r 9.54, C48 12.54.
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


def draw(req):
    """The inputs of one request, on the CPU, seeded by (key, act, entry): (x NHWC [n, h, w, cs_in], filter [cout, cin,
    kh, kw], scale, shift -- coutp + 16 entries each --, residual flat in the output's layout or None).  Post-ReLU maps
    with spikes, a signed BatchNorm-like scale, a residual of both signs; ones / zeros where statistics are asked for
    (the statistics entry points take the raw convolution: the tape passes ones / zeros)."""
    import zlib
    n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, nchw = req['key']
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    coutp = (cout + 15) // 16 * 16
    g = torch.Generator().manual_seed(zlib.crc32(repr((req['key'], req['act'], req['entry'])).encode()))
    x = act_like(n, h, w, cin, cs_in, g)
    wt = filt(cout, cin, kh, kw, g)
    pad_val = 0.0 if req['entry'] == 'program' else 1.0     # fold_scale_shift zero-pads; the tape's ones do not
    if req['stats']:
        sc, sh = torch.ones(coutp + 16), torch.zeros(coutp + 16)
    else:
        sgn = torch.where(torch.rand(cout, generator=g) < 0.3, -1.0, 1.0)
        sc = torch.full((coutp + 16,), pad_val)
        sc[:cout] = sgn * (0.5 + torch.rand(cout, generator=g))
        sh = torch.zeros(coutp + 16)
        sh[:cout] = 0.5 * torch.randn(cout, generator=g)
    res = None
    if has_res:
        r = act_like(n, ho, wo, cout, cs_out, g) - 0.5 * (torch.rand(1, generator=g).item())
        r.view(-1, cs_out)[:, cout:] = 0
        if nchw:
            r = r[..., :cout].permute(0, 3, 1, 2).contiguous()
        res = r.reshape(-1)
    return x, wt, sc, sh, res


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


# ---------------------------------------------------------------------------------------------------------------
# the edge list: every family at the edges of its tile mapping
# ---------------------------------------------------------------------------------------------------------------
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'egonet_amd', 'csrc')
FAMILIES = ('Staged', 'Dma', 'C48', 'F(2x2)', 'Stem', 'F(4x4)', 'Fc', 'S2r')
NOMINAL_CUS = 256               # what the CPU tests build the ``rounds`` requests with (the GPU test: the device's)
TAPE_TICKETS = 1 << 16          # train_hrnet: the ticket words a step owns
_FAMILY_OF_KERNEL = (('conv_mfma', 'Staged'), ('conv_dma', 'Dma'), ('conv_c48', 'C48'), ('conv_wino8', 'F(2x2)'),
                     ('conv_wino9', 'F(2x2)'), ('conv_stem', 'Stem'), ('conv_wino4', 'F(4x4)'), ('conv_fc', 'Fc'),
                     ('conv_s2r', 'S2r'))
NONE, RELU, SIGMOID, LEAKY, AFTER = engine.ACT_NONE, engine.ACT_RELU, engine.ACT_SIGMOID, engine.ACT_LEAKY, \
    engine.ACT_RES_AFTER
ACT_NAMES = {NONE: 'none', RELU: 'relu', SIGMOID: 'sigmoid', LEAKY: 'leaky'}


def kernel_text(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def config_name(cfg):
    buf = C.create_string_buffer(96)
    _lib.lib().egn_conv_config_name(cfg, buf, 96)
    return buf.value.decode()


def family_of(cfg):
    """The family of a config id, from the kernel its row names (cfg 0: the cost model, over the Staged family)."""
    if cfg <= 0:
        return 'Staged'
    name = config_name(cfg)
    for frag, fam in _FAMILY_OF_KERNEL:
        if frag in name:
            return fam
    raise KeyError((cfg, name))


def selectable_configs():
    """The ids a caller can be handed by the loaded library (no probe-only, retired, ablation or stamp rows)."""
    return [c for c in range(1, _lib.lib().egn_conv_num_configs() + 1) if tuner.kind_of(c) >= 0]


def plan(key, cfg):
    """What egn_conv_plan_query answers for (key, cfg): dict(cfg, tn, TH, TW, TNB, tps, tiles, cotiles), None: refused."""
    out = (C.c_int * 12)()
    if _lib.lib().egn_conv_plan_query(*key[:11], int(key[12]), cfg, out) != 0:
        return None
    return dict(cfg=out[0], tn=out[2] * out[4] * 16, TH=out[5], TW=out[6], TNB=out[7], tps=out[8], tiles=out[10],
                cotiles=out[11])


def _key(n, h, w, cin, cout, k=3, s=1, p=1, res=False, nchw=False, cs_in=None, cs_out=None, kw=None):
    r4 = lambda c: (c + 3) // 4 * 4
    return (n, h, w, cin, cs_in or r4(cin), cout, cout if nchw else (cs_out or r4(cout)), k, kw or k, s, p, bool(res),
            bool(nchw))


def _edge(E, fam, key, act, entry, line, why, stats=False, alias=False, f43=True):
    """One edge request, with the kinds / ticket words / in-place flag its caller would pass to ``tuner.choose``:
    engine.Program._conv_kinds for a program; the rule of train_hrnet._Tape._conv_launch for the tape (Winograd kinds
    behind a plain activation, F(4x4,3x3) where the step allows it: ``f43``); a direct filter for egn_conv2d_f32."""
    plain = act in (NONE, RELU)
    if entry == 'program':
        kinds, cap = engine.Program._conv_kinds(dict(act=act)), None
    elif entry == 'tape':
        kinds, cap = (tuner.TAPE_F43 if f43 else tuner.TAPE_WINO) if plain else tuner.DIRECT, TAPE_TICKETS
    else:
        kinds, cap = tuner.DIRECT, None
    assert not alias or key[11], 'the in-place add needs a residual'
    r = _request(key, act, entry, kinds, cap, inplace_res=alias, alias=alias, stats=stats,
                 src='edge/%s:%s' % (fam, why))
    r.update(line=line, why=why, family=fam)
    E.append(r)


EPILOGUES = [(a, r) for a in (NONE, RELU, SIGMOID, LEAKY) for r in ('', '+res', '+res_after')]


def epilogue_class(act, has_res):
    return 'epi:%s%s' % (ACT_NAMES[act & 0xf], ('+res_after' if act & AFTER else '+res') if has_res else '')


def _epilogue_set(E, fam, mk, entry, line, which=EPILOGUES):
    for a, r in which:
        _edge(E, fam, mk(bool(r)), a | (AFTER if r == '+res_after' else 0), entry, line, 'epilogue %s%s' % (ACT_NAMES[a], r))


PL, CM, MF, DM = 'conv_plan.hip', 'conv_common.h', 'conv_mfma.hip', 'conv_dma.hip'
C4, WN, ST, W4, W4W, FC, S2 = 'conv_c48.hip', 'conv_wino.hip', 'conv_stem.hip', 'conv_wino4.hip', 'conv_wino4w.hip', \
    'conv_fc.hip', 'conv_s2r.hip'
L_PIX = (CM, 'sPix[tid] = (b < a.TNB && n < a.N && oy < a.Ho && ox < a.Wo) ? (n * a.Ho + oy) * a.Wo + ox : -1;')
L_HALO = (PL, 'c.HH = (th - 1) * a.stride + a.KH;')
L_NARROW = (PL, 'if (tw < 4 && tw < a.Wo) continue;')
L_SMALL = (PL, 'if (tw >= 2 * a.Wo && tw > 1) continue;')
L_OUT = (PL, 'a.Ho = (a.H + 2 * a.pad - a.KH) / a.stride + 1;')
L_TPS = (PL, 'while (tps > 1 && (lds_bytes_for(c, cf) > lds_budget || tps * EGN_CKQ * tn > cf.staging.bi * 256)) {')
L_BAL = (PL, 'c.tps = cdiv(a.taps, nst);')
L_CHUNK = (PL, 'a.nchunk = cdiv(a.Cin, EGN_CK);')
L_PADC = (CM, 'if (co + 3 >= a.Cout) v.w = 0.f;')
L_COK = (CM, 'const bool cok = co < a.CoutP;')
L_TNB = (PL, 'const int tnb = tm / (tw * th);')
L_NCHW = (CM, 'sp[r] = (b < a.TNB && on[r] < a.N && oy < a.Ho && ox < a.Wo) ? oy * a.Wo + ox : -1;')
L_TW4 = (CM, 'const bool tw4 = (a.TW & 3) == 0;')
L_AFTER = (CM, 'if (res_after) v = rv + v;')
L_INPLACE = (CM, 'const_cast<float*>(a.res ? a.res : a.y), 0, (unsigned)((size_t)a.N * a.Ho * a.Wo * a.cs_out * 4), EGN_RSRC_WORD3);')
L_C48_OUT = (C4, '(oy < a.Ho && ox < a.Wo) ? (unsigned)(((N_ * a.Ho + oy) * a.Wo + ox) * C48 + li) * 4u : EGN_OOB;')
L_C48_GRID = (C4, 'const int grid = ntiles < cus ? ntiles : cus;')
L_C48_RES = (C4, 'const unsigned ro = has_res ? voff[mt][r] : EGN_OOB;')
L_WN_STATS = (WN, 'if (voff[r] != EGN_OOB) { st1[nt] += v; st2[nt] += v * v; }')
L_WN_STATS9 = (WN, 'if (a.stats != nullptr && voff[r] != EGN_OOB) { st1[nt] += v; st2[nt] += v * v; }')
L_WN_GRID = (WN, 'const int nwork = ((ntile + 7) / 8) * 8 * nct;')
L_WN_COT = (WN, 'if (a.Cout % 48 != 0 && !(a.Cout % 32 == 0 && cot32)) return false;')
L_WN_88 = (WN, 'return !(a.TH == 8 && a.TW == 8 && (a.Ho > 8 || a.Wo > 8));')
L_ST_OUT = (ST, 'const unsigned vo = (oy < a.Ho && ox < a.Wo) ? (unsigned)(((n * a.Ho + oy) * a.Wo + ox) * 64 + li) * 4u : EGN_OOB;')
L_ST_GRID = (ST, 'const int grid = ntile < 2 * cus ? ntile : 2 * cus;')
L_ST_ACT = (ST, 'if (act == EGN_ACT_SIGMOID || act == EGN_ACT_LEAKY) v = egn_act(acc[nt][r] * sc[nt] + sh[nt], act);')
L_W4_MAP = (W4, 'case Wino4: map_ok = a.Ho % 16 == 0 && a.Wo % 32 == 0; break;')
L_W4_B = (W4, 'case Wino4b_KSplit: map_ok = a.Ho % 16 == 0 && a.Wo % 16 == 0; break;')
L_W4_C = (W4, 'case Wino4c_KSplit: map_ok = a.Ho == 8 && a.Wo == 8; break;')
L_W4_KS = (W4, 'if (w4_ksplit(k) && (a.Cin % 32 || (a.res && a.res == a.y))) return false;')
L_W4_3L = (W4, 'if (KS > 1 && !a.tickets) {')
L_W4_GRID = (W4, 'static int w4_grid(int nwork, int nck) { return egn_persistent_grid(nwork, 8 * nck); }')
L_W4_NREG = (W4, 'const int nreg = a.tiles_x * a.tiles_y * ((a.N + W4G<GEO>::NIMG - 1) / W4G<GEO>::NIMG);')
L_W4_ST = (W4, 'if (ST && KS > 1 && !a.tickets) return EGN_E_BADARG;')
L_W4_MODE = ('conv_wino4.h', 'return nct >= W4_COX_MIN_NCT && (nct == 2 || nct == 4) ? 1 : 0;')
L_W4W = (W4W, 'const int ncp = a.Cout / (2 * W4_CO);')
L_W4W_GRID = (W4W, 'const int grid = egn_persistent_grid(nwork, 8 * ncp);')
L_FC_GRID = (FC, 'const int grid = (a.Cout / 16) * ((a.N * a.H * a.W + 15) / 16);')
L_FC_PITCH = (FC, 'const int pitch = a.out_nchw ? a.Cout : a.cs_out;')
L_FC_AFTER = (FC, 'const bool res_after = (a.act & EGN_ACT_RES_AFTER) != 0;')
L_FC_ONE = (FC, 'const bool one = a.H == 1 && a.W == 1;')
L_S2_GRID = (S2, 'int grid = bpc * cus / ncg * ncg;')
L_S2_TAIL = (S2, 'if (nitem < grid) grid = (nitem + ncg - 1) / ncg * ncg;')
L_S2_ITEM = (S2, 'const int nitem = a.N * (a.Ho / S2_TH) * (a.Wo / S2_TW) * ncg;')


def edge_requests(cus=NOMINAL_CUS):
    """The hand-written list: per family, the smallest shapes that reach the edges of its tile mapping, each with the
    kernel / planner line it is there for.  ``cus``: the compute units the ``rounds`` requests are sized for."""
    E = []
    # ---- Staged / Dma: the searched tile, the direct filter, any shape ----
    F = 'Staged/Dma'
    _edge(E, F, _key(3, 19, 13, 20, 40, res=True), RELU, 'program', L_PIX, 'ragged in x, y, n, K and Cout')
    _edge(E, F, _key(2, 11, 9, 37, 70, s=2, cs_in=40, cs_out=72), RELU, 'program', L_HALO,
          'odd map at stride 2, pad channels on both sides')
    _edge(E, F, _key(2, 1, 7, 16, 16), RELU, 'program', L_NARROW, 'map one pixel high')
    _edge(E, F, _key(2, 7, 1, 16, 16), RELU, 'program', L_NARROW, 'map one pixel wide')
    _edge(E, F, _key(2, 7, 1, 16, 16, res=True), NONE, 'tape', L_NARROW, 'map one pixel wide, in-place add', alias=True)
    _edge(E, F, _key(1, 2, 2, 16, 48), RELU, 'program', L_SMALL, 'map smaller than the kernel reach')
    _edge(E, F, _key(2, 5, 6, 32, 33, p=0), NONE, 'conv2d', L_OUT, 'valid 3x3')
    _edge(E, F, _key(2, 6, 7, 20, 24, k=5, p=2), RELU, 'program', L_TPS, '5x5: 25 taps')
    _edge(E, F, _key(2, 14, 10, 3, 64, k=7, s=2, p=3), RELU, 'program', L_TPS, '7x7 s2: 49 taps, several stages')
    _edge(E, F, _key(1, 9, 9, 4, 16, k=7, p=3), NONE, 'conv2d', L_TPS, '7x7 s1, a map that takes a 16 x 16 tile: several stages on 256 x 16')
    _edge(E, F, _key(1, 12, 11, 16, 16, k=4, kw=3, p=0), NONE, 'conv2d', L_BAL, '4x3 valid: 12 taps, balanced stages on 256 x 48')
    _edge(E, F, _key(2, 9, 7, 35, 66, k=1, s=2, p=0), NONE, 'conv2d', L_HALO, '1x1 s2 with pad channels')
    _edge(E, F, _key(2, 10, 11, 20, 32, s=3), RELU, 'program', L_HALO, 'stride 3')
    _edge(E, F, _key(2, 5, 5, 1, 16), RELU, 'program', L_CHUNK, 'Cin 1 in a stride of 4')
    _edge(E, F, _key(2, 5, 5, 3, 16), RELU, 'program', L_CHUNK, 'Cin 3 in a stride of 4')
    _edge(E, F, _key(1, 4, 4, 48, 16), RELU, 'program', L_CHUNK, 'three K chunks')
    for cout, cs in ((1, 4), (5, 8), (17, 20)):
        _edge(E, F, _key(3, 5, 5, 16, cout, cs_out=cs), RELU, 'program', L_PADC, 'Cout %d in a stride of %d' % (cout, cs))
    _edge(E, F, _key(2, 4, 4, 16, 200), RELU, 'program', L_COK, 'several co-tiles, ragged last, every tile width')
    _edge(E, F, _key(5, 2, 2, 16, 16), RELU, 'program', L_TNB, '5 images on image-group tiles')
    _edge(E, F, _key(130, 1, 1, 16, 16), RELU, 'program', L_TNB, '130 images of 1 x 1 on image-group tiles')
    _edge(E, F, _key(130, 1, 1, 20, 24, k=1, p=0), NONE, 'conv2d', L_TNB, '130 rows, 1x1, on whole-tile image groups')
    _edge(E, F, _key(130, 1, 1, 20, 24, k=1, p=0, res=True), NONE, 'tape', L_INPLACE, '130 rows, 1x1, in-place add', alias=True)
    _edge(E, F, _key(2, 5, 7, 20, 18, nchw=True), NONE, 'conv2d', L_NCHW, 'NCHW output, ragged')
    _edge(E, F, _key(2, 5, 7, 20, 18, nchw=True), SIGMOID, 'program', L_NCHW, 'NCHW output, sigmoid')
    _edge(E, F, _key(3, 3, 2, 16, 5, nchw=True), NONE, 'conv2d', L_TW4, 'NCHW output on tiles narrower than 4')
    _epilogue_set(E, F, lambda res: _key(2, 5, 7, 20, 22, res=res), 'program', L_AFTER)
    _edge(E, F, _key(2, 6, 5, 20, 20, res=True), NONE, 'tape', L_INPLACE, 'in-place data-gradient add', alias=True)
    _edge(E, F, _key(2, 6, 5, 20, 20), RELU, 'tape', L_PIX, 'tape forward, frozen-layer epilogue')

    # ---- conv_c48: 48 -> 48, 3x3 s1 p1, any map ----
    F = 'C48'
    for h, w in ((1, 1), (9, 7), (17, 19)):
        _edge(E, F, _key(2, h, w, 48, 48, res=True), RELU, 'program', L_C48_OUT, '%d x %d map: partial tiles' % (h, w))
    _epilogue_set(E, F, lambda res: _key(1, 9, 7, 48, 48, res=res), 'program', L_C48_RES)
    _edge(E, F, _key(2, 9, 7, 48, 48, res=True), NONE, 'tape', L_C48_RES, 'in-place data-gradient add', alias=True)
    _edge(E, F, _key(cus + 3, 8, 16, 48, 48), RELU, 'program', L_C48_GRID, 'second persistent round, ragged tail')

    # ---- F(2x2,3x3): even maps, Cin % 16, Cout % 48 or % 32 ----
    F = 'F(2x2)'
    for n, h, w, ci, co, why in ((1, 2, 2, 16, 32, '32-channel co-tile, one chunk, map inside one tile'),
                                 (3, 6, 4, 16, 48, 'ragged image group, map smaller than 8 x 8'),
                                 (5, 8, 8, 64, 144, 'ragged image group, three co-tiles'),
                                 (2, 18, 10, 32, 96, '16 x 16 and 8 x 16 tiles, partial both ways'),
                                 (2, 24, 40, 32, 64, 'several partial tiles, 32-channel co-tiles'),
                                 (1, 4, 6, 48, 96, 'three K chunks')):
        _edge(E, F, _key(n, h, w, ci, co, res=True), RELU, 'program', L_WN_88 if h <= 8 else L_WN_COT, why)
        _edge(E, F, _key(n, h, w, ci, co), NONE, 'tape', L_WN_STATS9, why + ', statistics', stats=True)
        _edge(E, F, _key(n, h, w, ci, co, res=True), NONE, 'tape', L_WN_STATS, why + ', in-place add', alias=True,
              f43=False)
    _epilogue_set(E, F, lambda res: _key(2, 6, 4, 16, 48, res=res), 'program', L_WN_88,
                  [(a, r) for a, r in EPILOGUES if a in (NONE, RELU) and r != '+res_after'])
    _edge(E, F, _key(4 * cus + 5, 2, 2, 16, 32), NONE, 'tape', L_WN_GRID, 'second persistent round, ragged tail, statistics',
          stats=True)
    _edge(E, F, _key(4 * cus + 5, 2, 2, 16, 32, res=True), RELU, 'program', L_WN_GRID, 'second persistent round, ragged tail')

    # ---- Stem: Cin <= 4 in a stride of 4, Cout 64, 3x3 s2 p1, even maps ----
    F = 'Stem'
    _edge(E, F, _key(1, 2, 2, 3, 64, s=2), RELU, 'program', L_ST_OUT, 'one output pixel')
    _edge(E, F, _key(1, 34, 22, 3, 64, s=2), RELU, 'program', L_ST_OUT, '17 x 11 outputs: partial tiles both ways')
    _edge(E, F, _key(2, 6, 4, 1, 64, s=2), RELU, 'program', L_ST_OUT, 'Cin 1')
    _edge(E, F, _key(2, 6, 4, 4, 64, s=2), NONE, 'conv2d', L_ST_OUT, 'Cin 4: no pad channel')
    _edge(E, F, _key(2, 6, 4, 3, 64, s=2), LEAKY, 'program', L_ST_ACT, 'LeakyReLU')
    _edge(E, F, _key(2, 6, 4, 3, 64, s=2), SIGMOID, 'program', L_ST_ACT, 'sigmoid')
    _edge(E, F, _key(2, 6, 4, 3, 64, s=2), NONE, 'tape', L_ST_OUT, 'tape forward')
    _edge(E, F, _key(2 * cus + 3, 2, 2, 3, 64, s=2), RELU, 'program', L_ST_GRID, 'more tiles than 2 x CUs blocks')

    # ---- F(4x4,3x3): 70 on 16 x 32 regions, 80 / 84 / 86 on 16 x 16, 82 / 83 on 8 x 8 maps ----
    F = 'F(4x4)'

    def f43(n, h, w, ci, co, line, why, alias=False):
        _edge(E, F, _key(n, h, w, ci, co, res=True), RELU, 'program', line, why)
        _edge(E, F, _key(n, h, w, ci, co), NONE, 'tape', L_W4_ST, why + ', statistics', stats=True)
        if alias:
            _edge(E, F, _key(n, h, w, ci, co, res=True), NONE, 'tape', L_W4_KS, why + ', in-place add', alias=True)
    f43(1, 16, 32, 16, 48, L_W4_MAP, 'one 16 x 32 region, one stage', alias=True)
    f43(1, 16, 32, 48, 96, L_W4_MAP, 'one 16 x 32 region, three stages, two co-tiles')
    f43(1, 16, 16, 16, 48, L_W4_B, 'one 16 x 16 region, one stage', alias=True)
    f43(1, 16, 16, 32, 96, L_W4_KS, 'one region, one stage per K half, one wide item, two co-tiles', alias=True)
    f43(1, 16, 16, 48, 96, L_W4W, 'three stages')
    f43(1, 16, 16, 96, 96, L_W4_KS, 'three stages per K half')
    f43(1, 16, 16, 32, 144, L_W4_MODE, 'three co-tiles')
    f43(1, 16, 16, 32, 192, L_W4_MODE, 'four co-tiles: co-tiles on the XCDs')
    f43(1, 16, 16, 32, 384, L_W4_MODE, 'eight co-tiles: each XCD its share of the filter')
    for n in (1, 2, 3, 5):
        f43(n, 8, 8, 32, 48, L_W4_NREG, '%d image%s on the four-image regions' % (n, '' if n == 1 else 's'), alias=n == 3)
    f43(3, 8, 8, 16, 48, L_W4_C, 'four-image regions, one stage')
    f43(2, 8, 8, 48, 96, L_W4_C, 'four-image regions, three stages, two co-tiles')
    f43(5, 8, 8, 96, 144, L_W4_KS, 'four-image regions, three stages per K half, three co-tiles')
    _edge(E, F, _key(cus + 3, 16, 32, 16, 48), NONE, 'tape', L_W4_GRID, 'second persistent round, ragged tail, statistics',
          stats=True)
    _edge(E, F, _key(cus + 3, 16, 16, 32, 96, res=True), RELU, 'program', L_W4W_GRID, 'second persistent round, ragged tail')
    _edge(E, F, _key(cus + 3, 16, 16, 32, 96), NONE, 'tape', L_W4_GRID, 'second persistent round, ragged tail, statistics',
          stats=True)
    _edge(E, F, _key(4 * cus + 5, 8, 8, 32, 48), NONE, 'tape', L_W4_GRID, 'second persistent round of four-image regions, '
          'ragged tail, statistics', stats=True)
    _epilogue_set(E, F, lambda res: _key(1, 16, 32, 32, 96, res=res), 'program', L_W4_3L,
                  [(a, r) for a, r in EPILOGUES if a in (NONE, RELU) and r != '+res_after'])
    _epilogue_set(E, F, lambda res: _key(3, 8, 8, 32, 96, res=res), 'program', L_W4_3L,
                  [(a, r) for a, r in EPILOGUES if a in (NONE, RELU) and r != '+res_after'])

    # ---- Fc: the 1x1 row GEMM ----
    F = 'Fc'
    for rows in (1, 15, 17, 130):
        _edge(E, F, _key(rows, 1, 1, 16, 16, k=1, p=0), RELU, 'program', L_FC_GRID, '%d rows, one chunk' % rows)
    _edge(E, F, _key(17, 1, 1, 272, 32, k=1, p=0), RELU, 'program', L_FC_GRID, 'Cin 272: 17 chunks over the waves')
    _edge(E, F, _key(15, 1, 1, 64, 32, k=1, p=0, cs_in=68, cs_out=36), RELU, 'program', L_FC_PITCH, 'pad channels both sides')
    _edge(E, F, _key(17, 1, 1, 16, 32, k=1, p=0, nchw=True), NONE, 'conv2d', L_FC_ONE, 'NCHW output on a 1 x 1 map')
    _edge(E, F, _key(3, 8, 8, 32, 48, k=1, p=0), RELU, 'program', L_FC_GRID, 'rows of a 3 x 8 x 8 map')
    _edge(E, F, _key(3, 5, 3, 32, 48, k=1, p=0), RELU, 'program', L_FC_GRID, '45 rows of a 3 x 5 x 3 map')
    _edge(E, F, _key(17, 1, 1, 96, 96, k=1, p=0, res=True), LEAKY | AFTER, 'program', L_FC_AFTER, "the lifter's epilogue")
    _epilogue_set(E, F, lambda res: _key(17, 1, 1, 32, 32, k=1, p=0, res=res), 'program', L_FC_AFTER)
    _edge(E, F, _key(17, 1, 1, 32, 32, k=1, p=0, res=True), NONE, 'tape', L_FC_AFTER, 'in-place add', alias=True)

    # ---- S2r: 48 -> multiples of 48, 3x3 s2 p1 ----
    F = 'S2r'
    _edge(E, F, _key(1, 4, 16, 48, 48, s=2), RELU, 'program', L_S2_TAIL, 'one item')
    _edge(E, F, _key(1, 4, 16, 48, 48, s=2), NONE, 'tape', L_S2_TAIL, 'one item, tape forward')
    _edge(E, F, _key(3, 8, 16, 48, 96, s=2), RELU, 'program', L_S2_ITEM, 'two co-groups, six items each')
    _edge(E, F, _key(5 * cus + 3, 4, 16, 48, 48, s=2), RELU, 'program', L_S2_GRID, 'items not a multiple of the rounded grid')
    return E


# ---- the classes a (request, config) pair is in, from the planner's answer ----
def _ksplit(key, cfg):
    return tuner.ticket_words(key, cfg) > 0


def _w4_items(nreg, nct, ks):
    """csrc/conv_wino4.h: w4_item_mode, w4_item_count."""
    if nct % 8 == 0:
        return nreg * nct * ks
    if nct == 4:
        return 8 * ((nreg * ks + 8 // nct - 1) // (8 // nct))
    return (nreg + 7) // 8 * nct * ks * 8


def _grid(nwork, rnd, cus, per_cu=1):
    cap = per_cu * cus // rnd * rnd
    return nwork, (cap if cap > 0 else rnd)


def items_and_cap(req, cfg, cus, p=None):
    """(items, the launcher's grid cap) of a persistent family; None: the grid is the item count."""
    key = req['key']
    p = p or plan(key, cfg)
    fam, cout = family_of(cfg), key[5]
    if fam == 'C48':
        return p['tiles'], cus
    if fam == 'Stem':
        return p['tiles'], 2 * cus
    if fam == 'F(2x2)':
        nct = p['cotiles']
        return _grid((p['tiles'] + 7) // 8 * 8 * nct, 8 * nct, cus)
    if fam == 'F(4x4)':
        if 'conv_wino4w' in config_name(cfg):
            ncp = cout // 96
            return _grid(_w4_items(p['tiles'], ncp, 1), 8 * ncp, cus)
        nct, ks = cout // 48, 2 if _ksplit(key, cfg) else 1
        return _grid(_w4_items(p['tiles'], nct, ks), 8 * nct * ks, cus)
    if fam == 'S2r':
        ncg = cout // 48
        return _grid(p['tiles'] * ncg, ncg, cus, 5)
    return None


def edge_classes(req, cfg, cus=NOMINAL_CUS):
    """The edge classes the pair (request, config) is in: computed from egn_conv_plan_query's answer and the key."""
    key = req['key']
    n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, nchw = key
    p = plan(key, cfg)
    assert p is not None, (key, cfg)
    fam = family_of(cfg)
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    ks = 2 if _ksplit(key, cfg) else 1
    shortest = 2 if (ks == 2 or 'conv_wino4w' in config_name(cfg)) else 1
    nchunk = (cin + 15) // 16
    out = set()
    if fam == 'Fc':
        if (n * h * w) % 16:
            out.add('ragged_n')
    else:
        if wo % p['TW']:
            out.add('ragged_x')
        if ho % p['TH']:
            out.add('ragged_y')
        if p['TNB'] > 1 and n % p['TNB']:
            out.add('ragged_n')
        if ho < p['TH'] or wo < p['TW']:
            out.add('small_map')
        if ho <= p['TH'] and wo <= p['TW']:
            out.add('one_tile')                 # all four borders of the map in one tile
    if cin % 16:
        out.add('ragged_k')
    if nchunk == shortest:
        out.add('one_chunk')
    if nchunk % ks == 0 and (nchunk // ks) % 2 == 1 and nchunk // ks > 1:
        out.add('odd_stages')
    if fam in ('Staged', 'Dma') and cout % p['tn']:
        out.add('ragged_cout')
    cot = cout // 96 if 'conv_wino4w' in config_name(cfg) else p['cotiles']
    if cot > 1:
        out.add('co_tiles')
    if cs_in > cin:
        out.add('pad_cin')
    if not nchw and cs_out > cout:
        out.add('pad_cout')
    if nchw:
        out.add('nchw')
    if p['tps'] < kh * kw:
        out.add('multi_stage')
    ic = items_and_cap(req, cfg, cus, p)
    if ic is not None and ic[0] > ic[1] and ic[0] % ic[1]:
        out.add('rounds')
    ragged = out & {'ragged_x', 'ragged_y', 'ragged_n', 'small_map'}
    if req['stats'] and req['entry'] == 'tape' and cfg > 0 and bnstats_rows(key, cfg) > 0:
        out.add('stats')
        if ragged:
            out.add('stats_ragged')
    if req['alias']:
        out.add('alias')
    if ks == 2 and req['entry'] in ('program', 'tape'):
        out.add('tickets')
        if not req['alias']:
            out.add('three_launch')
    out.add(epilogue_class(req['act'], has_res))
    return out


_EPI_ALL = frozenset(epilogue_class(a | (AFTER if r == '+res_after' else 0), bool(r)) for a, r in EPILOGUES)
_EPI_PLAIN = frozenset(('epi:none', 'epi:relu', 'epi:none+res', 'epi:relu+res'))
_DIRECT_CLASSES = frozenset(('one_tile', 'ragged_x', 'ragged_y', 'ragged_n', 'small_map', 'ragged_k', 'one_chunk', 'odd_stages',
                             'ragged_cout', 'co_tiles', 'pad_cin', 'pad_cout', 'nchw', 'multi_stage', 'alias')) | _EPI_ALL
# family -> the classes its predicate admits (a config of the family that cannot be in one: NOT_REACHABLE)
FAMILY_CLASSES = {
    'Staged': _DIRECT_CLASSES,
    'Dma': _DIRECT_CLASSES,
    'C48': frozenset(('one_tile', 'ragged_x', 'ragged_y', 'small_map', 'odd_stages', 'rounds', 'alias')) | _EPI_ALL,
    'F(2x2)': frozenset(('one_tile', 'ragged_x', 'ragged_y', 'ragged_n', 'small_map', 'one_chunk', 'odd_stages', 'co_tiles', 'rounds',
                         'stats', 'stats_ragged', 'alias')) | _EPI_PLAIN,
    'Stem': frozenset(('one_tile', 'ragged_x', 'ragged_y', 'small_map', 'ragged_k', 'one_chunk', 'pad_cin', 'rounds', 'epi:none',
                       'epi:relu', 'epi:sigmoid', 'epi:leaky')),
    'F(4x4)': frozenset(('one_tile', 'ragged_n', 'one_chunk', 'odd_stages', 'co_tiles', 'rounds', 'stats', 'stats_ragged', 'alias',
                         'tickets', 'three_launch')) | _EPI_PLAIN,
    'Fc': frozenset(('ragged_n', 'one_chunk', 'odd_stages', 'co_tiles', 'pad_cin', 'pad_cout', 'nchw', 'alias')) | _EPI_ALL,
    'S2r': frozenset(('one_tile', 'odd_stages', 'co_tiles', 'rounds', 'epi:none', 'epi:relu')),
}
# (family or config id, class) -> (file, the clause that rules it out).  What a family's predicate excludes for all its
# configs is simply not in FAMILY_CLASSES; this table says why, and names the configs of a family that differ.
_ROW = {51: '{51, 8, 1, 1, 3, F::Wino, Wino8_16x16, 0, 1, Product, {}, {16, 16, 1, 16}',
        57: '{57, 4, 1, 1, 3, F::Wino, Wino8_8x16, 0, 1, Product, {}, {8, 16, 1, 16}',
        59: '{59, 8, 1, 1, 3, F::Wino, Wino9_16x16, 0, 1, Product, {}, {16, 16, 1, 16}',
        62: '{62, 4, 1, 1, 3, F::Wino, Wino9_8x16, 0, 1, Product, {}, {8, 16, 1, 16}',
        70: '{70, 12, 1, 1, 3, F::Wino4, Wino4, 0, 3, Product, {}, {16, 32, 1, 36}',
        80: '{80, 12, 1, 1, 3, F::Wino4, Wino4b, 0, 3, Product, {}, {16, 16, 1, 36}',
        84: '{84, 12, 1, 1, 3, F::Wino4, Wino4b_KSplit, 0, 3, Product, {}, {16, 16, 1, 36}',
        86: '{86, 12, 1, 1, 3, F::Wino4, Wino4w, 0, 3, Product, {}, {16, 16, 1, 36}'}
NOT_REACHABLE = {
    ('C48', 'ragged_k'): (C4, 'a.Cin == 48 && a.cs_in == 48'),
    ('F(2x2)', 'ragged_k'): (WN, 'a.Cin % EGN_CK'),
    ('F(4x4)', 'ragged_k'): (W4, 'a.Cin % 16 == 0'),
    ('Fc', 'ragged_k'): (FC, 'a.Cin % EGN_CK == 0'),
    ('S2r', 'ragged_k'): (S2, 'a.Cin == S2_CIN'),
    ('F(4x4)', 'ragged_x'): (W4, 'a.Wo % 16 == 0'),
    ('F(4x4)', 'ragged_y'): (W4, 'a.Ho % 16 == 0'),
    ('F(4x4)', 'small_map'): (W4, 'map_ok = a.Ho == 8 && a.Wo == 8'),
}
for _c in (51, 57, 59, 62, 70, 80, 84, 86):                      # one image per tile: no image group to be ragged
    NOT_REACHABLE[(_c, 'ragged_n')] = (PL, _ROW[_c])
for _c in (70, 80, 84, 86):                                      # whole regions only, so statistics never meet an edge
    NOT_REACHABLE[(_c, 'stats_ragged')] = (PL, _ROW[_c])
for _c in (70, 80, 82, 86):                                      # not a K split: no ticket words, one launch
    NOT_REACHABLE[(_c, 'tickets')] = NOT_REACHABLE[(_c, 'three_launch')] = \
        (W4, 'static bool w4_ksplit(Wino4Kernel k) { return k == Wino4b_KSplit || k == Wino4c_KSplit; }')
for _c in (83, 84):                                              # the K split zeroes y before the residual is read
    NOT_REACHABLE[(_c, 'alias')] = (W4, '(a.res && a.res == a.y)')
NOT_REACHABLE[(86, 'stats')] = (W4, 'case Wino4r: return 0;      // (the wide items / half blocks / row owners have no training build)')


# ---- refusals: one step outside each clause of a fixed-tile family's predicate ----
def refusal_requests():
    """[(cfg, key, act, (file, clause), where the refusal is made)]: 'plan' = egn_conv_plan_query refuses the key;
    'residual' = the clause reads the residual, which only egn_conv_plan_takes (tuner.usable) is told; 'launch' = the
    clause reads the activation, which no planner query and no tuner key carries: the launcher refuses."""
    R = []
    add = lambda cfgs, key, clause, act=RELU, at='plan': R.extend((c, key, act, clause, at) for c in cfgs)
    f22 = (51, 52, 56, 57, 59, 60, 61, 62)
    add(f22, _key(1, 7, 8, 16, 48), (WN, '(a.Ho & 1) || (a.Wo & 1)'))                     # odd Ho
    add(f22, _key(1, 8, 7, 16, 48), (WN, '(a.Ho & 1) || (a.Wo & 1)'))
    add(f22, _key(1, 8, 8, 16, 48, cs_in=20), (WN, 'a.cs_in != a.Cin'))
    add(f22, _key(1, 8, 8, 24, 48), (WN, 'a.Cin % EGN_CK'))
    add(f22, _key(1, 8, 8, 16, 40), (WN, 'if (a.Cout % 48 != 0 && !(a.Cout % 32 == 0 && cot32)) return false;'))
    add((52, 56, 60, 61), _key(4, 8, 10, 16, 48), (WN, 'return !(a.TH == 8 && a.TW == 8 && (a.Ho > 8 || a.Wo > 8));'))
    add((70,), _key(1, 16, 16, 16, 48), (W4, 'case Wino4: map_ok = a.Ho % 16 == 0 && a.Wo % 32 == 0; break;'))
    add((70, 80, 84, 86), _key(1, 8, 32, 32, 96), (W4, 'a.Ho % 16 == 0'))
    add((70,), _key(1, 16, 32, 24, 48), (W4, 'a.Cin % 16 == 0'))
    add((80, 82), _key(1, 16, 16, 24, 48), (W4, 'a.Cin % 16 == 0'))
    add((83, 84), _key(1, 16, 16, 48, 48), (W4, 'if (w4_ksplit(k) && (a.Cin % 32 ||'))
    add((83,), _key(1, 8, 8, 48, 48), (W4, 'if (w4_ksplit(k) && (a.Cin % 32 ||'))
    add((86,), _key(1, 16, 16, 16, 96), (W4W, 'a.Cin >= 32'))
    add((86,), _key(1, 16, 16, 32, 48), (W4W, 'a.Cout % (2 * W4_CO) == 0'))
    add((82, 83), _key(1, 16, 16, 32, 48), (W4, 'case Wino4c_KSplit: map_ok = a.Ho == 8 && a.Wo == 8; break;'))
    add((70, 80, 84, 86), _key(1, 16, 32, 32, 96, cs_in=36),('egn_internal.h', 'a.cs_in == a.Cin'))
    add((82, 83), _key(4, 8, 8, 32, 96, cs_in=36), ('egn_internal.h', 'a.cs_in == a.Cin'))
    add((70, 80, 84, 86), _key(1, 16, 32, 32, 96, s=2), ('egn_internal.h', 'a.stride == 1'))
    add((42, 44), _key(1, 8, 8, 47, 48, cs_in=48), (C4, 'a.Cin == 48'))
    add((42, 44), _key(1, 8, 8, 48, 48, s=2), (C4, 'a.stride == 1'))
    add((42, 44), _key(1, 8, 8, 48, 48, cs_out=52), (C4, 'a.cs_out == 48'))
    add((64,), _key(1, 7, 8, 3, 64, s=2), (ST, '(a.H % 2 == 0) && (a.W % 2 == 0)'))
    add((64,), _key(1, 8, 8, 5, 64, s=2, cs_in=8), (ST, 'a.Cin <= 4 && a.cs_in == 4'))
    add((64,), _key(1, 8, 8, 3, 48, s=2), (ST, 'a.Cout == 64'))
    add((64,), _key(1, 8, 8, 3, 64, s=2, res=True), (ST, 'a.res == nullptr'), at='residual')
    add((85,), _key(1, 6, 16, 48, 48, s=2), (S2, 'a.Ho % S2_TH == 0'))                  # Ho 3
    add((85,), _key(1, 5, 16, 48, 48, s=2), (S2, 'a.H % 2 == 0 && a.W % 2 == 0'))
    add((85,), _key(1, 4, 8, 48, 48, s=2), (S2, 'a.Wo % S2_TW == 0'))
    add((85,), _key(1, 4, 16, 32, 48, s=2), (S2, 'a.Cin == S2_CIN'))
    add((85,), _key(1, 4, 16, 48, 48, s=2, res=True), (S2, 'a.res == nullptr'), at='residual')
    add((85,), _key(1, 4, 16, 48, 48, s=2), (S2, '(act == EGN_ACT_NONE || act == EGN_ACT_RELU)'), act=SIGMOID, at='launch')
    add((79,), _key(2, 2, 2, 16, 16, k=1, p=0, nchw=True), (FC, '(a.out_nchw ? one : a.cs_out >= a.Cout)'))
    add((79,), _key(17, 1, 1, 24, 16, k=1, p=0), (FC, 'a.Cin % EGN_CK == 0'))
    add((79,), _key(17, 1, 1, 16, 24, k=1, p=0), (FC, 'a.Cout % 16 == 0'))
    add((79,), _key(17, 1, 1, 16, 16, k=3, p=1), (FC, 'a.KH == 1 && a.KW == 1'))
    # every family: an NCHW output takes no residual (the NCHW epilogue of conv_common.h reads none)
    add((1, 11, 21, 79), _key(17, 1, 1, 16, 16, k=1, p=0, res=True, nchw=True), ('program.hip', 'if (out_nchw && res) return EGN_E_BADARG;'),
        at='residual')
    return R
