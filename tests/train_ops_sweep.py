"""The launches of csrc/train_ops.hip that a native training step makes, and the edges of their thread mappings.

Helper module of tests/test_gpu_train_ops_sweep.py and tests/test_train_ops_sweep_cpu.py (imported, not a conftest).
Third of the family of tests/conv_sweep.py and tests/wgrad_sweep.py: BatchNorm statistics, the fused BatchNorm +
activation + dropout forward / backward, column sums, the loss criteria, the fuse layer's backward, zero insertion and
the optimizers, every launch against a float64 reference written from the kernel's header comment.

A request is a dict:
  name     the entry point (egn_*)
  s        its non-pointer arguments by name (ARGS below; float arguments rounded to fp32, as the kernel sees them)
  null     the pointer arguments that were NULL
  alias    groups of pointer arguments that held the same address (in place: y is z, dz is dy, y is a)
  srcs     where it was seen (recorded step, or the kernel line an edge request is there for)
  opt      input options of an edge request (step count before the launch, column offsets, ...)

Requests come from two places.  ``Recorder`` notes what the product's steps launch (``recorded_requests``: the steps of
conv_sweep.TAPE_STEPS plus EXTRA_RUNS with update=True); ``edge_requests`` is the hand-written list below, each entry
with the kernel line it is there for.  Entry points whose only size is an element count are replayed with the count
clamped to ``loop_clamp`` elements (every thread goes round its grid-stride loop twice, with a ragged tail): a W48
parameter vector's float64 reference stays off the CPU, what the kernel does is unchanged.

The bound, per output:  |got - want64| <= C[entry] * 2^-24 * A,  A = the same formula on absolute values.
  statistics:  mean: A = mean|x|;  biased / unbiased variance: A = mean(x^2) (x r/(r-1));  invstd: what follows from the
  variance's,  A = invstd^3 mean(x^2) / 2 + invstd.
Each constant is about 4x the worst ratio of an fp32 emulation of the entry point's formula in torch (``emulate``:
the kernel's association order where it matters -- sequential 64-term fp32 partials added in double), run on the CPU
on the inputs of ``edge_requests`` (tests/test_train_ops_sweep_cpu.py prints the ratios); never against the kernel.
The emulation's sqrt and divisions are torch's (correctly rounded); the device's sqrtf and `/` are within 1 ulp = 2 x
2^-24 relative each by the HIP math API's table, so the optimizers (one sqrtf, two divisions, the 1/rows of dz one) get
that added on top.  Summation order and fused multiply-add are free to differ: that is the 4x.

  entry                     worst emulation ratio   C
  add                       1.00                    4      (one rounding)
  sigmoid_bwd               1.37                    6
  zero_insert2, dropout_mask, step_counters, the optimizers' counter: exact (A = 0)
  fuse_bwd                  1.91                    8      (up to 64 terms, sequential)
  colsum                    4.68                    19
  bn_stats (all outputs)    6.94                    28     (unbiased variance, a column of x30 spikes)
  bn_stats_finalize         1.49                    6      (double sums of double partials; the running statistics)
  bn_act_fwd (+ _drop)      2.63                    10
  bn_bwd_sums (+ _drop)     4.24                    17
  bn_bwd_dz (+ _drop)       4.27                    17 + 2 (1.0f / rows)
  mse, elem_loss            1.97                    8      (dpred; the loss scalar accumulates in double)
  l1                        0.21                    2      (dpred is +-weight / n rounded once: 0.5, x4)
  adam                      3.13                    12 + 6 (sqrtf, two divisions)
  adam_l2                   5.33                    22 + 6 (the same; v' after the cancellation of g + wd p)
  sgd                       3.28                    13
A wrong kernel of the kinds listed in ``MUTANTS`` breaks these bounds on the same inputs (checked on the CPU).
Adam's parameter update is a quotient of two things that cancel together (g + wd p -> 0 leaves m' / sqrt(v') at its
size): its A is the first-order propagation of A_m and A_v through the quotient (``_optimizer``), 1.5 |update| where
nothing cancels.

The one-pass variance E[x^2] - m^2 from fp32 partials, relative error of the variance on 2048 rows at column offsets
of 0, 3 sigma and 30 sigma (the emulation's 64-term partials; torch's fp32 batch_norm on the same data beside it):
  0: 3.9e-8 (torch 2.1e-7)    3 sigma: 6.8e-7 (torch 1.8e-7)    30 sigma: 7.7e-5 (torch 1.6e-7)
A known departure, held to the mean(x^2) bound (28 x 2^-24 x 901 sigma^2 = 1.5e-3 sigma^2 at 30 sigma).  The kernel
itself measures 5.8e-8 / 9.7e-8 / 3.3e-6 on this matrix: at 2048 rows launch_col gives 48 row splits of 21 lanes, a lane
adds two or three rows in fp32 before the double takes over; the 64-term partials of the emulation are the kernel's worst
case (rows > 2 * 256 * 64 * lanes), which the >64-rows-per-lane edge case runs.

The ReLU gate: a pre-activation with |pre64| <= C[bn_act_fwd] 2^-24 A_pre may gate differently in fp32.  A column
holding such an element is left out of dbeta / dgamma / dz (dres: the element only); at most GATE_CAP of the columns
of a case.  Share of columns left out on the edge list (the reference alone, checked on the CPU): 0 for every case but
three: 1 of 66 columns (0.015) in the ld 68 x 37 rows ReLU cases of egn_bn_bwd_dz_f32 (their dbeta / dgamma inputs are
part of the request's seed, so the sums' cases draw other matrices), 1 of 1024 in the row-stream stride-loop case.  The
>64-rows-per-lane case runs the backward sums without a gate: 16.8 M elements at ~1.5e-6 undecided each put a tenth of
254 columns out by size alone, and its subject is the flush, not the gate.
"""
import ctypes as C
import os
import re
import zlib

import numpy as np
import torch

import conv_sweep as S
from egonet_amd import _lib

U = S.U
GATE_CAP = 0.10
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_BOUND = {
    'egn_add_f32': 4.0, 'egn_sigmoid_bwd_f32': 6.0, 'egn_zero_insert2_f32': 0.0, 'egn_dropout_mask_f32': 0.0,
    'egn_step_counters_i64': 0.0, 'egn_fuse_bwd_f32': 8.0, 'egn_colsum_f32': 19.0, 'egn_bn_stats_f32': 28.0,
    'egn_bn_stats_finalize_f32': 6.0, 'egn_bn_act_fwd_f32': 10.0, 'egn_bn_act_fwd_drop_f32': 10.0,
    'egn_bn_bwd_sums_f32': 17.0, 'egn_bn_bwd_sums_drop_f32': 17.0, 'egn_bn_bwd_dz_f32': 19.0,
    'egn_bn_bwd_dz_drop_f32': 19.0, 'egn_mse_f32': 8.0, 'egn_elem_loss_f32': 8.0, 'egn_l1_f32': 2.0,
    'egn_adam_step_dev_f32': 18.0, 'egn_adam_l2_step_dev_f32': 28.0, 'egn_sgd_step_dev_f32': 13.0,
}

# name -> arguments in ABI order (the trailing stream left out); a pointer carries its role:
#   in (read), out (written whole), io (read and written), ws (scratch)
_ARGS_TEXT = {
    'egn_add_f32': 'a:in b:in y:out n',
    'egn_colsum_f32': 'a:in rows cols ld sum:out ws:ws',
    'egn_bn_stats_f32': 'z:in rows cols ld eps mean:out invstd:out var_unbiased:out running_mean:io running_var:io '
                        'momentum ws:ws',
    'egn_bn_stats_finalize_f32': 'partials:in nrows rows cols eps mean:out invstd:out var_unbiased:out '
                                 'running_mean:io running_var:io momentum',
    'egn_bn_act_fwd_f32': 'z:in mean:in invstd:in gamma:in beta:in mask:in keep_scale relu res:in y:out rows cols ld',
    'egn_bn_act_fwd_drop_f32': 'z:in mean:in invstd:in gamma:in beta:in p seed step_dev:in layer relu res:in y:out '
                               'rows cols ld',
    'egn_bn_bwd_sums_f32': 'dy:in z:in mask:in keep_scale mean:in invstd:in gamma:in beta:in relu res:in rows cols ld '
                           'dbeta:out dgamma:out ws:ws',
    'egn_bn_bwd_sums_drop_f32': 'dy:in z:in p seed step_dev:in layer mean:in invstd:in gamma:in beta:in relu res:in '
                                'rows cols ld dbeta:out dgamma:out ws:ws',
    'egn_bn_bwd_dz_f32': 'dy:in z:in mask:in keep_scale mean:in invstd:in gamma:in beta:in relu res:in dbeta:in '
                         'dgamma:in dz:out dres:out rows cols ld',
    'egn_bn_bwd_dz_drop_f32': 'dy:in z:in p seed step_dev:in layer mean:in invstd:in gamma:in beta:in relu res:in '
                              'dbeta:in dgamma:in dz:out dres:out rows cols ld',
    'egn_dropout_mask_f32': 'mask:out n p seed step_dev:in layer',
    'egn_mse_f32': 'pred:in tgt:in rows cols ld_pred ld_tgt weight accumulate dpred:io loss:io',
    'egn_elem_loss_f32': 'pred:in tgt:in rows cols ld_pred ld_tgt crit weight accumulate dpred:io loss:io',
    'egn_l1_f32': 'pred:in tgt:in n weight dpred:out loss:io',
    'egn_sigmoid_bwd_f32': 'dy:in y:in dz:out n',
    'egn_zero_insert2_f32': 'dy:in up:out N Ho Wo H W cs',
    'egn_fuse_bwd_f32': 'dy:in y:in g:out N H W cs shift',
    'egn_step_counters_i64': 'counters:in n zero_f64:io',
    'egn_adam_step_dev_f32': 'p:io g:in m:io v:io n lr_dev:in beta1 beta2 eps step_dev:io',
    'egn_adam_l2_step_dev_f32': 'p:io g:in m:io v:io n lr_dev:in beta1 beta2 eps weight_decay step_dev:io',
    'egn_sgd_step_dev_f32': 'p:io g:in buf:io n lr_dev:in momentum weight_decay step_dev:io',
}
ARGS = {k: [tuple((a.split(':') + [None])[:2]) for a in v.split()] for k, v in _ARGS_TEXT.items()}
QUERIES = {'egn_colreduce_ws_bytes'}          # host-only: nothing launched, nothing to replay
OPTIMIZERS = ('egn_adam_step_dev_f32', 'egn_adam_l2_step_dev_f32', 'egn_sgd_step_dev_f32')


def train_ops_entries():
    """The entry points csrc/train_ops.hip defines, from its text."""
    with open(os.path.join(_ROOT, 'egonet_amd', 'csrc', 'train_ops.hip')) as fh:
        return set(re.findall(r'extern "C" \w+ (egn_\w+)\(', fh.read()))


def product_entries():
    """Those of them that the native training steps call, from the text of the three step modules."""
    called = set()
    for f in ('train_hrnet.py', 'train_lifter.py', 'train_common.py'):
        with open(os.path.join(_ROOT, 'egonet_amd', f)) as fh:
            called |= set(re.findall(r'\.(egn_\w+)\(', fh.read()))
    return (called & train_ops_entries()) - QUERIES


def grid_cap(name):
    """Blocks of 256 threads the entry point's launcher caps its grid at (grid_for: 4096; the loss kernels: 256)."""
    return 256 if name in ('egn_mse_f32', 'egn_elem_loss_f32', 'egn_l1_f32') else 4096


def loop_clamp(name):
    """The smallest count of work items that sends every thread round the stride loop twice, with a ragged tail."""
    return 2 * grid_cap(name) * 256 + 77


# ---------------------------------------------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------------------------------------------
def _addr(a):
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    if isinstance(a, C.c_void_p):
        return a.value or 0
    return C.cast(a, C.c_void_p).value or 0


class _Proxy(object):
    def __init__(self, handle, rec):
        self.__dict__['_h'], self.__dict__['_rec'] = handle, rec

    def __getattr__(self, name):
        fn = getattr(self._h, name)
        if name not in self._rec.names:
            return fn
        rec = self._rec

        def call(*args):
            rec.note(name, args)
            return fn(*args)            # forwarded as it came
        return call


class Recorder(object):
    """Context manager: while active ``_lib.lib()`` returns a proxy of the loaded handle that notes every call of an
    entry point of train_ops.hip and forwards it unchanged.  Step objects keep the handle (``self.L``): build them
    inside.  ``handle``: a stand-in for the library (the CPU test's stub)."""

    def __init__(self, handle=None, names=None, signatures=None):
        self.handle = handle
        self.names = set(names) if names is not None else train_ops_entries()
        self.sig = signatures or _lib.SIGNATURES
        self.notes = []
        self.src = ''

    def __enter__(self):
        self._prev = _lib._LIB
        real = self.handle if self.handle is not None else _lib.lib()
        self._restore = self._prev if self.handle is not None else real
        _lib._LIB = _Proxy(real, self)
        return self

    def __exit__(self, *exc):
        _lib._LIB = self._restore
        return False

    def note(self, name, args):
        types = self.sig[name][1]
        assert len(args) == len(types), (name, len(args), len(types))
        names = ARGS.get(name) or [('a%d' % i, 'in' if t is C.c_void_p else None) for i, t in enumerate(types)]
        s, null, addrs = {}, [], {}
        for (arg, role), t, v in zip(names, types, args):      # (zip drops the trailing stream)
            if role is not None:
                a = _addr(v)
                if a == 0:
                    null.append(arg)
                else:
                    addrs.setdefault(a, []).append(arg)
            elif t is C.c_float:
                s[arg] = float(np.float32(v))
            else:
                s[arg] = int(v)
        alias = tuple(sorted(tuple(g) for g in addrs.values() if len(g) > 1))
        self.notes.append(dict(name=name, s=s, null=frozenset(null), alias=alias, src=self.src, opt={}))


def req_key(r):
    return (r['name'], tuple(sorted(r['s'].items())), tuple(sorted(r['null'])), r['alias'],
            tuple(sorted(r['opt'].items())))


def merged(notes):
    """Distinct requests, each with the list of places it was seen (as conv_sweep.pairs)."""
    seen, out = {}, []
    for r in notes:
        if r['name'] in QUERIES:
            continue
        k = req_key(r)
        if k in seen:
            seen[k]['srcs'].append(r['src'])
            continue
        seen[k] = dict(r, srcs=[r['src']])
        out.append(seen[k])
    return out


def clamped(r):
    """The request with its element count clamped (entry points whose only size is that count)."""
    n = r['s'].get('n')
    if n is None or r['name'] == 'egn_step_counters_i64' or r['opt'].get('keep_n'):
        return r
    unit = 4 if r['name'] in ('egn_add_f32', 'egn_dropout_mask_f32') else 1      # float4 work items
    lim = loop_clamp(r['name']) * unit
    if n <= lim:
        return r
    return dict(r, s=dict(r['s'], n=lim), opt=dict(r['opt'], clamped_from=n))


# the training-ops sweep's own runs beside conv_sweep.TAPE_STEPS (update=True: the optimizer launches are seen)
def _w48_crit(coor_type):
    from egonet_amd import configs
    return lambda device, g: S.hrnet_run(configs.w48_config('coordinates'), 3, device, g, update=True,
                                         coor_type=coor_type)


EXTRA_RUNS = [
    ('lifter-dropout0.5/b30', lambda device, g: S.lifter_run(30, device, g, update=True, dropout=0.5)),
    ('lifter-leaky-sgd/b30', lambda device, g: S.lifter_run(30, device, g, update=True, leaky=True, optim_type='sgd',
                                                            momentum=0.9, weight_decay=1e-3)),
    ('lifter-adam-l2/b30', lambda device, g: S.lifter_run(30, device, g, update=True, weight_decay=1e-2)),
    ('train-w48-l1/b3', _w48_crit('l1')),
    ('train-w48-sl1/b3', _w48_crit('sl1')),
]


def recorded_requests(device='cuda'):
    """Every train_ops.hip launch of the recorded steps, merged."""
    g = torch.Generator().manual_seed(0)
    prev = os.environ.get('EGONET_AMD_AUTOTUNE')
    os.environ['EGONET_AMD_AUTOTUNE'] = '0'
    try:
        with Recorder() as rec:
            for src, make in S.TAPE_STEPS + EXTRA_RUNS:
                rec.src = src
                tr, step = make(device, g)        # built inside: the step object keeps the proxy
                step()
                torch.cuda.synchronize()
                del tr, step
    finally:
        if prev is None:
            del os.environ['EGONET_AMD_AUTOTUNE']
        else:
            os.environ['EGONET_AMD_AUTOTUNE'] = prev
    return rec.notes, [clamped(r) for r in merged(rec.notes)]


# ---------------------------------------------------------------------------------------------------------------
# the edge requests
# ---------------------------------------------------------------------------------------------------------------
def _req(name, why, null=(), alias=(), opt=None, **s):
    want = [a for a, role in ARGS[name] if role is None]
    assert sorted(want) == sorted(s), (name, want, sorted(s))
    fl = {a for (a, role), t in zip(ARGS[name], _lib.SIGNATURES[name][1]) if t is C.c_float}
    s = {k: (float(np.float32(v)) if k in fl else int(v)) for k, v in s.items()}
    return dict(name=name, s=s, null=frozenset(null), alias=tuple(alias), src=why, srcs=[why], opt=dict(opt or {}))


def _bn(kinds, rows, cols, ld, why, flag=1, res=False, dres=True, drop=None, opt=None):
    """Requests of the BatchNorm entry points named in ``kinds`` (colsum, stats, fwd, sums, dz) on one matrix.
    drop: None, 'mask' (explicit keep mask) or the probability of the in-kernel dropout."""
    out = []
    d = dict(rows=rows, cols=cols, ld=ld)
    nres = () if res else ('res',)
    p = drop if isinstance(drop, float) else None
    keep = 1.0 / (1.0 - 0.5) if drop == 'mask' else 1.0
    nmask = () if drop == 'mask' else ('mask',)
    dr = dict(p=p, seed=0x123456789ABCDEF, layer=3) if p is not None else None
    if 'colsum' in kinds:
        out.append(_req('egn_colsum_f32', why, opt=opt, **d))
    if 'stats' in kinds:
        out.append(_req('egn_bn_stats_f32', why, opt=opt, eps=1e-5, momentum=0.1, **d))
    bflag = flag & 0xf
    if 'fwd' in kinds:
        if dr:
            out.append(_req('egn_bn_act_fwd_drop_f32', why, null=nres, opt=opt, relu=flag, **dict(d, **dr)))
        else:
            out.append(_req('egn_bn_act_fwd_f32', why, null=nres + nmask, opt=opt, keep_scale=keep, relu=flag, **d))
    if 'sums' in kinds:
        if dr:
            out.append(_req('egn_bn_bwd_sums_drop_f32', why, null=nres, opt=opt, relu=bflag, **dict(d, **dr)))
        else:
            out.append(_req('egn_bn_bwd_sums_f32', why, null=nres + nmask, opt=opt, keep_scale=keep, relu=bflag, **d))
    if 'dz' in kinds:
        nd = nres + (() if dres else ('dres',))
        if dr:
            out.append(_req('egn_bn_bwd_dz_drop_f32', why, null=nd, opt=opt, relu=bflag, **dict(d, **dr)))
        else:
            out.append(_req('egn_bn_bwd_dz_f32', why, null=nd + nmask, opt=opt, keep_scale=keep, relu=bflag, **d))
    return out


ALL_BN = ('colsum', 'stats', 'fwd', 'sums', 'dz')
REDUCE = ('colsum', 'stats', 'sums')
STREAM = ('fwd', 'dz')


def edge_requests():
    """The hand-written list.  Sizes follow the launchers as they stand: launch_col (64 float4 groups per block,
    256 / groups row lanes, nsplit = min(512 / column blocks, rows / (2 lanes), 256)), rowstream_grid (256 groups per
    block, 256 / groups rows per step, at most 2048 steps), grid_for (4096 blocks)."""
    E = []
    # ok[k] = c < cols / c < p.cols with a false entry, idle threads (17 groups: 15 row lanes, 1 idle thread; 9 groups)
    E += _bn(ALL_BN, 37, 66, 68, 'pad columns, ld/4 = 17 does not divide 256')
    E += _bn(ALL_BN, 37, 33, 36, 'pad columns, ld/4 = 9 does not divide 256')
    # colreduce_partial: a second column block (g0 = 64) that is ragged (65 groups: the second block has 1, 256 lanes)
    E += _bn(REDUCE, 50, 258, 260, 'ld/4 = 65 > 64: second, ragged column block')
    # row-stream kernels: blockIdx.y = 1 with a single group (cgb = 1, rpi = 256)
    E += _bn(STREAM, 9, 1026, 1028, 'ld/4 = 257 > 256: second column block of one group')
    # fewer rows than row lanes
    E += _bn(ALL_BN, 2, 66, 68, 'rows < row lanes')
    E += _bn(ALL_BN, 3, 66, 68, 'rows < row lanes')
    # ld >= 256: 4 lanes, nsplit = rows / 8 = 12, rows_per = 9: split 11 starts at row 99 > 98
    E += _bn(REDUCE, 98, 256, 256, 'empty trailing row split')
    # nsplit capped at 256, 4 lanes: a lane passes 64 rows when rows > 256 * 4 * 64 (cnt >= 64 inside the loop);
    # the backward sums without a gate (module comment)
    E += _bn(REDUCE, 256 * 4 * 64 + 259, 254, 256, 'fp32 partials flushed to double inside the loop', flag=0)
    # rpi = 1 at ld 1024, gx capped at 2048: rows beyond 2048 go round the stride loop
    E += _bn(STREAM, 2048 + 77, 1024, 1024, 'row-stream grid-stride loop')
    # colreduce_final on its own: lanes with no row, exactly 8 per lane, the k = sl + 256 tail
    for nrows in (1, 33, 256, 257, 300):
        E.append(_req('egn_bn_stats_finalize_f32', 'finalize over %d partial rows' % nrows, nrows=nrows,
                      rows=8 * nrows, cols=20, eps=1e-5, momentum=0.1))
    # activation flags: forward 0, 1, 2, 0x11, 0x12, backward 0, 1, 2, each with and without res (and dres)
    for res in (False, True):
        for flag in (0, 1, 2, 0x11, 0x12):
            E += _bn(('fwd',), 37, 66, 68, 'forward flag 0x%x' % flag, flag=flag, res=res)
        for flag in (0, 1, 2):
            E += _bn(('sums',), 37, 66, 68, 'backward flag %d' % flag, flag=flag, res=res)
            for dres in (False, True):
                E += _bn(('dz',), 37, 66, 68, 'backward flag %d' % flag, flag=flag, res=res, dres=dres)
    # dropout: explicit mask, drawn in the kernel with p = 0.25 and 0.5 (the lifter's block tail: 0x11 with res)
    for drop in ('mask', 0.25, 0.5):
        E += _bn(('fwd', 'sums', 'dz'), 37, 66, 68, 'dropout %s' % drop, drop=drop)
        E += _bn(('fwd',), 37, 66, 68, 'dropout %s, residual after' % drop, flag=0x11, res=True, drop=drop)
    E += _bn(('fwd', 'sums', 'dz'), 37, 33, 36, 'dropout 0.5, pad columns, ld/4 = 9', drop=0.5)
    # conditioning of the one-pass variance: columns offset by 0, 3 sigma, 30 sigma
    E.append(_req('egn_bn_stats_f32', 'column offsets of 0, 3 and 30 sigma', opt=dict(offsets=1), rows=2048, cols=48,
                  ld=48, eps=1e-5, momentum=0.1))
    # in place, as the steps call them
    E += [dict(r, alias=(('z', 'y'),)) for r in _bn(('fwd',), 37, 66, 68, 'in place: y is z')]
    E += [dict(r, alias=(('dy', 'dz'),)) for r in _bn(('dz',), 37, 66, 68, 'in place: dz is dy')]
    # the element-count entry points the edge list would otherwise not hold: a ragged count, and in place as the tape adds
    E.append(_req('egn_add_f32', 'ragged count', n=4 * 1031))
    E.append(_req('egn_add_f32', 'in place: y is a', alias=(('a', 'y'),), n=4 * 1031))
    E.append(_req('egn_sigmoid_bwd_f32', 'ragged count', n=1031))
    E.append(_req('egn_dropout_mask_f32', 'the mask the drop kernels draw', n=37 * 68, p=0.5, seed=0x123456789ABCDEF,
                  layer=3))
    # the losses: ld_pred != ld_tgt != cols, 300 x 221 = 66 300 > 65 536 threads (the stride loop of the 256-block
    # grid), planted d = 0 and |d| = 1
    L = dict(rows=300, cols=221, ld_pred=228, ld_tgt=224, weight=0.5)
    for acc, nd in ((0, False), (1, False), (0, True)):
        nul = ('dpred',) if nd else ()
        for crit in (0, 1, 2):
            E.append(_req('egn_elem_loss_f32', 'criterion %d, accumulate %d' % (crit, acc), null=nul, crit=crit,
                          accumulate=acc, **L))
        E.append(_req('egn_mse_f32', 'accumulate %d' % acc, null=nul, accumulate=acc, **L))
    for nd in (False, True):
        E.append(_req('egn_l1_f32', 'stride loop, sign(0)', null=('dpred',) if nd else (), n=300 * 221, weight=0.5))
    # fuse backward: block sums of 1, 4, 16, 64 terms, gate on y with planted 0 and -0.0
    for shift in (0, 1, 2, 3):
        for gate in (True, False):
            E.append(_req('egn_fuse_bwd_f32', 'shift %d' % shift, null=() if gate else ('y',), N=2, H=16, W=8, cs=12,
                          shift=shift))
    # zero insertion: H = 2 Ho and 2 Ho - 1, for both axes
    for H, W in ((6, 10), (5, 9), (6, 9), (5, 10)):
        E.append(_req('egn_zero_insert2_f32', 'H %d W %d for Ho 3 Wo 5' % (H, W), N=2, Ho=3, Wo=5, H=H, W=W, cs=8))
    # the optimizers: one step from a given state; n exceeds one grid (4096 x 256) and is no multiple of 256
    n = 4096 * 256 + 77
    for step0 in (0, 1, 999):
        o = dict(step0=step0, keep_n=1)
        E.append(_req('egn_adam_step_dev_f32', 'step count %d' % step0, opt=o, n=n, beta1=0.9, beta2=0.999, eps=1e-8))
        E.append(_req('egn_adam_l2_step_dev_f32', 'step count %d' % step0, opt=o, n=n, beta1=0.9, beta2=0.999,
                      eps=1e-8, weight_decay=1e-2))
        E.append(_req('egn_sgd_step_dev_f32', 'step count %d' % step0, opt=o, n=n, momentum=0.9, weight_decay=1e-3))
        E.append(_req('egn_sgd_step_dev_f32', 'step count %d, momentum 0, no buffer' % step0, null=('buf',), opt=o,
                      n=n, momentum=0.0, weight_decay=1e-3))
    # the counters: none but the accumulator, one, one without accumulator, more than one pass of 256 threads
    for cnt, acc in ((0, True), (1, True), (1, False), (300, True)):
        E.append(_req('egn_step_counters_i64', '%d counters' % cnt, null=(() if acc else ('zero_f64',)) +
                      (() if cnt else ('counters',)), n=cnt))
    return E


# ---------------------------------------------------------------------------------------------------------------
# Philox (the in-kernel dropout's keep mask)
# ---------------------------------------------------------------------------------------------------------------
def philox4(k0, k1, c):
    """numpy Philox4x32-10 (Salmon et al.): c = uint32 [n, 4] counters -> [n, 4] draws."""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    c = c.astype(np.uint64)
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = M0 * c[:, 0], M1 * c[:, 2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(0xffffffff), p1 >> np.uint64(32), p1 & np.uint64(0xffffffff)
        c = np.stack([hi1 ^ c[:, 1] ^ np.uint64(k0), lo1, hi0 ^ c[:, 3] ^ np.uint64(k1), lo0], axis=1)
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c.astype(np.uint32)


def drop_mask(n, p, seed, layer, step):
    """Keep mask (0 / 1, float32 [n]) of n consecutive elements: counter (float4 group, layer, step), kept <=> draw >=
    p 2^32 (make_drop / egn_drop_mask4)."""
    n4 = n // 4
    ctr = np.zeros((n4, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(n4, dtype=np.uint64) & 0xffffffff
    ctr[:, 1] = np.arange(n4, dtype=np.uint64) >> 32
    ctr[:, 2], ctr[:, 3] = layer & 0xffffffff, step & 0xffffffff
    t = float(np.float32(p)) * 4294967296.0
    thresh = 0xFFFFFFFF if t >= 4294967295.0 else max(int(t), 1)
    draws = philox4(seed & 0xffffffff, seed >> 32, ctr).reshape(-1)
    return torch.from_numpy((draws >= np.uint32(thresh)).astype(np.float32))


DROP_STEP = 7       # the value the replay puts into *step_dev of the dropout kernels


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
PAD_JUNK = 3.0      # input pad columns hold this: a kernel that lets them through is seen


def _gen(r):
    return torch.Generator().manual_seed(zlib.crc32(repr(req_key(r)).encode()))


def _mat(rows, cols, ld, g, like='normal'):
    if like == 'act':
        m = S.act_like(rows, 1, 1, cols, ld, g).view(rows, ld)
    else:
        m = torch.zeros(rows, ld)
        m[:, :cols] = torch.randn(rows, cols, generator=g)
    m[:, cols:] = PAD_JUNK
    return m


def _stats64(z64, eps):
    m = z64.mean(0)
    var = (z64 * z64).mean(0) - m * m
    return m, (var + eps).rsqrt()


def inputs(r):
    """name -> CPU tensor for every non-NULL pointer argument that is read (in / io), from a seed derived from the
    request.  Activations: conv_sweep.act_like; gamma in [0.5, 1.5]; the rest random normal."""
    name, s, g = r['name'], r['s'], _gen(r)
    has = lambda a: a not in r['null']
    x = {}
    if name in ('egn_add_f32', 'egn_sigmoid_bwd_f32'):
        n = s['n']
        if name == 'egn_add_f32':
            x['a'], x['b'] = torch.randn(n, generator=g), torch.randn(n, generator=g)
        else:
            x['dy'], x['y'] = torch.randn(n, generator=g), torch.sigmoid(2 * torch.randn(n, generator=g))
    elif name == 'egn_colsum_f32':
        x['a'] = _mat(s['rows'], s['cols'], s['ld'], g, 'act')
    elif name == 'egn_bn_stats_f32':
        z = _mat(s['rows'], s['cols'], s['ld'], g, 'act')
        if r['opt'].get('offsets'):         # unit-variance columns at 0, 3 sigma, 30 sigma
            z[:, :s['cols']] = torch.randn(s['rows'], s['cols'], generator=g) + \
                torch.tensor([0.0, 3.0, 30.0]).repeat(s['cols'] // 3 + 1)[:s['cols']]
        x['z'] = z
        if has('running_mean'):
            x['running_mean'] = torch.randn(s['cols'], generator=g)
        if has('running_var'):
            x['running_var'] = torch.rand(s['cols'], generator=g) + 0.5
    elif name == 'egn_bn_stats_finalize_f32':
        # the partials are the reference's: float64 block sums of a random z, [nrows][2][cols]
        z = S.act_like(s['rows'], 1, 1, s['cols'], s['cols'], g).view(s['rows'], s['cols']).double()
        blk = (torch.arange(s['rows']) * s['nrows']) // s['rows']
        part = torch.zeros(s['nrows'], 2, s['cols'], dtype=torch.float64)
        part[:, 0].index_add_(0, blk, z)
        part[:, 1].index_add_(0, blk, z * z)
        x['partials'] = part
        if has('running_mean'):
            x['running_mean'] = torch.randn(s['cols'], generator=g)
        if has('running_var'):
            x['running_var'] = torch.rand(s['cols'], generator=g) + 0.5
    elif name.startswith('egn_bn_'):
        rows, cols, ld = s['rows'], s['cols'], s['ld']
        x['z'] = _mat(rows, cols, ld, g, 'act')
        m, istd = _stats64(x['z'][:, :cols].double(), 1e-5)
        x['mean'], x['invstd'] = m.float(), istd.float()
        x['gamma'] = torch.rand(cols, generator=g) + 0.5
        x['beta'] = 0.5 * torch.randn(cols, generator=g)
        if has('res'):
            x['res'] = _mat(rows, cols, ld, g)
        if 'keep_scale' in s and has('mask'):
            x['mask'] = (torch.rand(rows, ld, generator=g) < 0.5).float()
        if 'p' in s and has('step_dev'):
            x['step_dev'] = torch.tensor([DROP_STEP], dtype=torch.int32)
        if 'bwd' in name:
            x['dy'] = _mat(rows, cols, ld, g)
        if 'bwd_dz' in name:        # the sums the first backward launch leaves: the reference's, rounded to fp32
            sums = reference(dict(r, name=name.replace('dz', 'sums')), x, sums_only=True)
            x['dbeta'], x['dgamma'] = sums['dbeta'][0].float(), sums['dgamma'][0].float()
    elif name == 'egn_dropout_mask_f32':
        x['step_dev'] = torch.tensor([DROP_STEP], dtype=torch.int32)
    elif name in ('egn_mse_f32', 'egn_elem_loss_f32', 'egn_l1_f32'):
        if name == 'egn_l1_f32':
            rows, cols, ldp, ldt = 1, s['n'], s['n'], s['n']
        else:
            rows, cols, ldp, ldt = s['rows'], s['cols'], s['ld_pred'], s['ld_tgt']
        p, t = _mat(rows, cols, ldp, g), _mat(rows, cols, ldt, g)
        p[:, :cols] *= 1.5                       # |d| on both sides of 1
        for k, (pv, tv) in enumerate(((0.25, 0.25), (1.5, 0.5), (-0.5, 0.5), (0.0, 0.0), (-3.0, -2.0))):
            if k < cols:                         # planted: d = 0 exactly, |d| = 1 exactly
                p[rows // 2, k], t[rows // 2, k] = pv, tv
        x['pred'], x['tgt'] = p, t
        x['loss'] = torch.tensor([0.75], dtype=torch.float64)       # the launch adds to what is there
        if has('dpred') and name != 'egn_l1_f32':
            d = _mat(rows, cols, ldp, g)
            if not s['accumulate']:
                d[:] = float('nan')              # written, not added to: every element has to be
            d[:, cols:] = float('nan')           # pad columns of dpred are not the kernel's: they stay as they are
            x['dpred'] = d
    elif name == 'egn_zero_insert2_f32':
        x['dy'] = torch.randn(s['N'], s['Ho'], s['Wo'], s['cs'], generator=g)
    elif name == 'egn_fuse_bwd_f32':
        x['dy'] = torch.randn(s['N'], s['H'], s['W'], s['cs'], generator=g)
        if has('y'):
            y = torch.relu(torch.randn(s['N'], s['H'], s['W'], s['cs'], generator=g))
            y.view(-1)[1::7] = -0.0              # outputs of exactly 0 and -0.0 (and the ReLU's own zeros)
            y.view(-1)[2::11] = 0.0
            x['y'] = y
    elif name in OPTIMIZERS:
        n, step0 = s['n'], r['opt'].get('step0', 3)
        x['p'] = 0.1 * torch.randn(n, generator=g)
        mag = 10.0 ** (9.0 * torch.rand(n, generator=g) - 6.0)           # 1e-6 .. 1e3
        grad = mag * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        grad[torch.rand(n, generator=g) < 0.05] = 0.0                    # exact zeros among them
        x['g'] = grad
        fresh = step0 == 0
        for a in ('m', 'v', 'buf'):
            if a in dict(ARGS[name]) and has(a):
                st = torch.randn(n, generator=g) * 0.01
                x[a] = torch.zeros(n) if fresh else (st * st if a == 'v' else st)
        x['lr_dev'] = torch.tensor([r['opt'].get('lr', 1e-3)], dtype=torch.float32)
        x['step_dev'] = torch.tensor([step0], dtype=torch.int32)
    elif name == 'egn_step_counters_i64':
        if has('counters'):
            x['counters'] = torch.randint(0, 1 << 40, (s['n'],), generator=g, dtype=torch.int64)   # the counters' values
        if has('zero_f64'):
            x['zero_f64'] = torch.tensor([3.5], dtype=torch.float64)
    else:
        raise KeyError('no inputs for %s' % name)
    for grp in r['alias']:                       # one address: one content (the first member that is read)
        src = next((a for a in grp if a in x), None)
        for a in grp:
            if a in x and src is not None:
                x[a] = x[src]
    return x


# ---------------------------------------------------------------------------------------------------------------
# the references (float64 on the fp32 inputs) and the fp32 emulations: one formula, two precisions
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ('dz_no_row_terms', 'invstd_unbiased', 'bias_correction_t_minus_1', 'weight_decay_after_moments',
           'sgd_first_step_momentum', 'smooth_l1_threshold_half', 'l1_grad_at_zero', 'leaky_slope_0.1',
           'res_before_activation', 'no_keep_scale_in_backward')


def _colsum(t, dt):
    """Column sums: exact order in float64; in fp32 sequential partials of 64 rows added in double (the kernel's)."""
    if dt == torch.float64:
        return t.sum(0)
    rows, cols = t.shape
    pad = (-rows) % 64
    if pad:
        t = torch.cat([t, t.new_zeros(pad, cols)])
    t = t.view(-1, 64, cols)
    acc = torch.zeros_like(t[:, 0])
    for k in range(64):
        acc = acc + t[:, k]
    return acc.double().sum(0)


def _out(want, A, view=None, pad=None, keep=None):
    return (want, A, dict(view=view, pad=pad, keep=keep))


def _f32(v):
    return float(np.float32(v))


def _bn_family(r, x, dt, mut, sums_only=False):
    name, s = r['name'], r['s']
    rows, cols, ld = s['rows'], s['cols'], s['ld']
    view = (rows, ld, cols)
    V = lambda t: t.to(dt).view(rows, ld)[:, :cols]
    z = V(x['z'])
    vec = lambda a: x[a].to(dt)[:cols]
    mean, istd, gm, bt = vec('mean'), vec('invstd'), vec('gamma'), vec('beta')
    flag = s['relu']
    act, after = flag & 0xf, bool(flag & 0x10)
    if mut == 'res_before_activation':
        after = False
    slope = 0.1 if mut == 'leaky_slope_0.1' else 0.01
    res = V(x['res']) if 'res' in x else None
    mask, keep = None, 1.0
    if 'mask' in x:
        mask, keep = V(x['mask']), s['keep_scale']
    elif s.get('p', 0) > 0:
        mask = V(drop_mask(rows * ld, s['p'], s['seed'], s['layer'], int(x['step_dev'][0])).to(z.device))
        keep = _f32(np.float32(1) / (np.float32(1) - np.float32(s['p'])))
    xhat = (z - mean) * istd
    A_xhat = (z.abs() + mean.abs()) * istd.abs()
    pre = gm * xhat + bt
    A_pre = gm.abs() * A_xhat + bt.abs()
    if res is not None and not after:
        pre, A_pre = pre + res, A_pre + res.abs()
    out = {}
    if 'fwd' in name:
        o = pre
        if act == 2:
            o = torch.where(o > 0, o, slope * o)
        elif act:
            o = o.clamp_min(0)
        A = A_pre
        if mask is not None:
            o, A = o * (mask * keep), A * (mask * keep)
        if res is not None and after:
            o, A = res + o, res.abs() + A
        out['y'] = _out(o, A, view, 'zero')
        if mask is not None:
            out['_kept'] = float(mask.double().mean())
        return out
    # backward: the gate reads gamma xhat + beta + res whatever the flag (flags 0, 1, 2 only)
    d = V(x['dy'])
    A_d = d.abs()
    if mask is not None:
        k = 1.0 if mut == 'no_keep_scale_in_backward' else keep
        d, A_d = d * (mask * k), A_d * (mask * keep)
    undecided = None
    if act:
        closed = ~(pre > 0)
        d = torch.where(closed, slope * d if act == 2 else torch.zeros_like(d), d)
        A_d = torch.where(closed, slope * A_d if act == 2 else torch.zeros_like(A_d), A_d)
        if dt == torch.float64:
            undecided = pre.abs() <= C_BOUND['egn_bn_act_fwd_f32'] * U * A_pre
    colkeep = None
    if undecided is not None:
        colkeep = ~undecided.any(0)
        out['_left_out'] = float((~colkeep).double().mean())
    if 'sums' in name or sums_only:
        out['dbeta'] = _out(_colsum(d, dt), A_d.sum(0), keep=colkeep)
        out['dgamma'] = _out(_colsum(d * xhat, dt), (A_d * A_xhat).sum(0), keep=colkeep)
        return out
    db, dg = vec('dbeta'), vec('dgamma')
    if dt == torch.float32:
        inv = torch.tensor(1.0, dtype=dt) / rows
        dz = gm * istd * (d - db * inv - xhat * dg * inv)
    elif mut == 'dz_no_row_terms':
        dz = gm * istd * d
    else:
        dz = gm * istd * (d - db / rows - xhat * dg / rows)
    A_dz = gm.abs() * istd.abs() * (A_d + db.abs() / rows + A_xhat * dg.abs() / rows)
    out['dz'] = _out(dz, A_dz, view, 'zero', None if colkeep is None else colkeep[None, :].expand(rows, cols))
    if 'dres' not in r['null']:
        out['dres'] = _out(d, A_d, view, 'zero', None if undecided is None else ~undecided)
    return out


def _stats_out(r, x, t0, t1, mut, dt):
    """mean / invstd / unbiased variance / running statistics from the column sums (double in the kernel)."""
    s = r['s']
    rows, eps, mom = s['rows'], s['eps'], s['momentum']
    t0, t1 = t0.double(), t1.double()
    m = t0 / rows
    msq = t1 / rows
    var = (msq - m * m).clamp_min(0)
    vu = var * rows / (rows - 1) if rows > 1 else var
    istd = ((vu if mut == 'invstd_unbiased' else var) + eps).rsqrt()
    A_m = x['_absmean']
    A_v = msq * (rows / (rows - 1.0) if rows > 1 else 1.0)
    cast = (lambda t: t.float()) if dt == torch.float32 else (lambda t: t)
    out = {'mean': _out(cast(m), A_m), 'invstd': _out(cast(istd), 0.5 * istd ** 3 * msq + istd)}
    if 'var_unbiased' not in r['null']:
        out['var_unbiased'] = _out(cast(vu), A_v)
    if 'running_mean' in x:
        rm = x['running_mean'].to(dt)
        out['running_mean'] = _out((1 - mom) * rm + mom * cast(m).to(dt), rm.abs().double() + mom * A_m)
    if 'running_var' in x:
        rv = x['running_var'].to(dt)
        out['running_var'] = _out((1 - mom) * rv + mom * cast(vu).to(dt), rv.abs().double() + mom * A_v)
    out['_rel_var'] = (var, msq)
    return out


def _loss_family(r, x, dt, mut):
    name, s = r['name'], r['s']
    if name == 'egn_l1_f32':
        rows, cols, ldp, ldt, crit, acc = 1, s['n'], s['n'], s['n'], 1, 0
    else:
        rows, cols, ldp, ldt, acc = s['rows'], s['cols'], s['ld_pred'], s['ld_tgt'], s['accumulate']
        crit = s.get('crit', 0)
    w = s['weight']
    p = x['pred'].to(dt).view(rows, ldp)[:, :cols]
    t = x['tgt'].to(dt).view(rows, ldt)[:, :cols]
    d = (p - t).double()                  # the kernel subtracts in fp32 and goes on in double
    Ad = p.abs().double() + t.abs().double()
    inv = w / float(rows * cols)
    thr = 0.5 if mut == 'smooth_l1_threshold_half' else 1.0
    if crit == 0:
        v, gd, Av, Ag = d * d, 2 * d, Ad * Ad, 2 * Ad
    elif crit == 1:
        v, gd, Av, Ag = d.abs(), torch.sign(d), Ad, torch.ones_like(Ad)
        if mut == 'l1_grad_at_zero':
            gd = torch.where(d >= 0, 1.0, -1.0).to(d.dtype)
    else:
        small = d.abs() < thr
        v = torch.where(small, 0.5 * d * d, d.abs() - 0.5)
        gd = torch.where(small, d, torch.sign(d))
        Av, Ag = torch.where(Ad < 1, 0.5 * Ad * Ad, Ad + 0.5), Ad.clamp_max(1.0)
    loss0 = x['loss'].double()
    out = {'loss': _out(loss0 + v.sum() * inv, loss0.abs() + Av.sum() * abs(inv))}
    if 'dpred' not in r['null']:
        gf = gd * inv
        Agf = Ag * abs(inv)
        if dt == torch.float32:
            gf = gf.float()
        if acc:
            d0 = x['dpred'].to(dt).view(rows, ldp)[:, :cols]
            gf, Agf = d0 + gf.to(dt), d0.abs().double() + Agf
        out['dpred'] = _out(gf, Agf, (rows, ldp, cols), 'untouched')
    return out


def _optimizer(r, x, dt, mut):
    name, s = r['name'], r['s']
    t = int(x['step_dev'][0]) + 1                    # the counter is incremented before the update
    lr = float(x['lr_dev'][0])
    p, g = x['p'].to(dt), x['g'].to(dt)
    dev = x['p'].device
    out = {'step_dev': _out(torch.tensor([t], dtype=torch.float64, device=dev),
                            torch.zeros(1, dtype=torch.float64, device=dev))}
    wd = s.get('weight_decay', 0.0)
    if name == 'egn_sgd_step_dev_f32':
        mom = s['momentum']
        gi, A_g = g + wd * p, g.abs() + wd * p.abs()
        if mom != 0:
            buf = x['buf'].to(dt)
            first = t <= 1
            if first:
                gi2 = mom * gi if mut == 'sgd_first_step_momentum' else gi
                A_b = A_g
            else:
                gi2, A_b = mom * buf + gi, mom * buf.abs() + A_g
            out['buf'] = _out(gi2, A_b.double())
            gi, A_g = gi2, A_b
        out['p'] = _out(p - lr * gi, (p.abs() + lr * A_g).double())
        return out
    b1, b2, eps = s['beta1'], s['beta2'], s['eps']
    m, v = x['m'].to(dt), x['v'].to(dt)
    gi, A_g = g, g.abs()
    if wd and mut != 'weight_decay_after_moments':
        gi, A_g = g + wd * p, g.abs() + wd * p.abs()
    if dt == torch.float32:
        one = torch.tensor(1.0, dtype=dt)
        mi = b1 * m + (one - b1) * gi
        vi = b2 * v + (one - b2) * gi * gi
    else:
        mi = b1 * m + (_f32(np.float32(1) - np.float32(b1))) * gi          # 1.f - b1 is exact in fp32
        vi = b2 * v + (_f32(np.float32(1) - np.float32(b2))) * gi * gi
    tt = t - 1 if mut == 'bias_correction_t_minus_1' else t
    step_size = lr / (1.0 - b1 ** tt) if tt > 0 else float('inf')
    bc2 = (1.0 - b2 ** tt) ** 0.5 if tt > 0 else 0.0
    if dt == torch.float32:
        step_size, bc2 = _f32(step_size), _f32(bc2)
    den = vi.sqrt() / bc2 + eps
    upd = step_size * (mi / den)
    if wd and mut == 'weight_decay_after_moments':
        upd = upd + lr * wd * p
    A_m = (b1 * m.abs() + (1 - b1) * A_g).double()
    A_v = (b2 * v.abs() + (1 - b2) * A_g * A_g).double()
    out['m'] = _out(mi, A_m)
    out['v'] = _out(vi, A_v)
    # The quotient's formula on absolute values hides the cancellation of g + wd p (and of b1 m + (1 - b1) g) in
    # front of a division by nearly the same quantity: A is the first-order propagation of A_m and A_v through
    # m' / (sqrt(v') / bc2 + eps) instead -- 1.5 |update| where nothing cancels.
    den64, rt = den.double(), vi.double().sqrt()
    A_q = A_m / den64 + torch.where(rt > 0, mi.double().abs() * A_v / (2 * rt.clamp_min(1e-300) * bc2 * den64 ** 2),
                                    torch.zeros_like(rt))
    out['p'] = _out(p - upd, p.abs().double() + abs(step_size) * A_q)
    return out


def _compute(r, x, dt, mut=None, sums_only=False):
    name, s = r['name'], r['s']
    if name == 'egn_add_f32':
        a, b = x['a'].to(dt), x['b'].to(dt)
        return {'y': _out(a + b, (a.abs() + b.abs()).double())}
    if name == 'egn_sigmoid_bwd_f32':
        dy, y = x['dy'].to(dt), x['y'].to(dt)
        return {'dz': _out(dy * y * (1 - y), (dy.abs() * y.abs() * (1 + y.abs())).double())}
    if name == 'egn_colsum_f32':
        a = x['a'].to(dt).view(s['rows'], s['ld'])[:, :s['cols']]
        got = _colsum(a, dt)
        return {'sum': _out(got.float() if dt == torch.float32 else got, a.abs().double().sum(0))}
    if name == 'egn_bn_stats_f32':
        z = x['z'].to(dt).view(s['rows'], s['ld'])[:, :s['cols']]
        return _stats_out(r, dict(x, _absmean=z.abs().double().mean(0)), _colsum(z, dt), _colsum(z * z, dt), mut, dt)
    if name == 'egn_bn_stats_finalize_f32':
        part = x['partials'].view(s['nrows'], 2, s['cols'])
        return _stats_out(r, dict(x, _absmean=part[:, 0].abs().sum(0) / s['rows']), part[:, 0].sum(0),
                          part[:, 1].sum(0), mut, dt)
    if name.startswith('egn_bn_'):
        return _bn_family(r, x, dt, mut, sums_only)
    if name == 'egn_dropout_mask_f32':
        m = drop_mask(s['n'], s['p'], s['seed'], s['layer'], int(x['step_dev'][0])).double()
        return {'mask': _out(m.to(x['step_dev'].device), torch.zeros_like(m).to(x['step_dev'].device)),
                '_kept': float(m.mean())}
    if name in ('egn_mse_f32', 'egn_elem_loss_f32', 'egn_l1_f32'):
        return _loss_family(r, x, dt, mut)
    if name == 'egn_zero_insert2_f32':
        dy = x['dy'].double()
        up = dy.new_zeros(s['N'], s['H'], s['W'], s['cs'])
        up[:, 0:2 * s['Ho']:2, 0:2 * s['Wo']:2] = dy
        return {'up': _out(up, torch.zeros_like(up))}
    if name == 'egn_fuse_bwd_f32':
        k = 1 << s['shift']
        d = x['dy'].to(dt)
        if 'y' in x:
            d = torch.where(x['y'] > 0, d, torch.zeros_like(d))
        N, H, W, cs = d.shape
        blk = d.view(N, H // k, k, W // k, k, cs).permute(0, 1, 3, 5, 2, 4).reshape(N, H // k, W // k, cs, k * k)
        if dt == torch.float64:
            tot = blk.sum(-1)
        else:
            tot = torch.zeros_like(blk[..., 0])
            for i in range(k * k):
                tot = tot + blk[..., i]
        return {'g': _out(tot, blk.abs().double().sum(-1))}
    if name in OPTIMIZERS:
        return _optimizer(r, x, dt, mut)
    if name == 'egn_step_counters_i64':
        out = {}
        if 'counters' in x:
            out['counters'] = _out(x['counters'] + 1, torch.zeros_like(x['counters'], dtype=torch.float64))
        if 'zero_f64' in x:
            out['zero_f64'] = _out(torch.zeros_like(x['zero_f64']), torch.zeros_like(x['zero_f64']))
        return out
    raise KeyError('no reference for %s' % name)


def reference(r, x, mut=None, sums_only=False):
    """name -> (want float64, A, how to look at it) per output; keys with '_' are figures about the case."""
    return _compute(r, x, torch.float64, mut, sums_only)


def emulate(r, x):
    """The same formulas in fp32, in the kernel's association order where it matters."""
    return _compute(r, x, torch.float32)


def worst_ratios(got, ref, exact_ints=True):
    """out name -> worst |got - want| / (2^-24 A) over what is compared (columns / elements left out excluded)."""
    res = {}
    for k, (want, A, how) in ((k, v) for k, v in ref.items() if not k.startswith('_')):
        g = got[k][0] if isinstance(got[k], tuple) else got[k]
        if want.dtype in (torch.int64, torch.int32):
            res[k] = 0.0 if torch.equal(g.to(want.dtype).reshape(want.shape), want) else float('inf')
            continue
        q = S.ratio(g.reshape(want.shape), want.double(), A.double().expand_as(want))
        if how['keep'] is not None:
            q = torch.where(how['keep'], q, torch.zeros_like(q))
        res[k] = float(q.max()) if q.numel() else 0.0
    return res
