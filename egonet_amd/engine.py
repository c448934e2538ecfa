"""Execution engines: turn a parameter-owning ``nn.Module`` into a native launch
program of gfx950 HIP kernels (C ABI: include/egonet_hip.h).

``HRNetEngine``   backbone + heads        (reference hrnet.py:563-614)
``LifterEngine``  2D->3D residual MLP      (reference FCmodel.py:92-105)

A program is recorded once per (device, batch shape):
  * ``_Recorder`` walks the module tree and records symbolic ops on symbolic
    NHWC buffers (channel stride rounded up to 4);
  * buffer lifetimes are derived from the op list and packed into ONE activation
    arena by a best-fit free-list allocator (an HRNet-W48 forward at B=64 needs
    a few hundred MB instead of ~18 GB of distinct outputs, so the working set
    of neighbouring layers stays inside the 256 MB Infinity Cache);
  * weights are folded (BatchNorm -> per-channel scale/shift) and prepacked (on
    the host: filters.py) into ONE device blob in the layouts the conv kernels read;
  * the ops are emitted into a native ``egn_program`` whose pointers are
    (slot, offset) pairs: slot 0 arena, 1 weights, 2.. user tensors.
A forward is then a single C call that issues ~320 kernel launches.
"""
import collections
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib, tuner
from ._lib import Ref, NULL_REF, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_LEAKY
from .filters import (CK, H_CK, H_KS, _round_up, pack_conv_weight, wino_cot, pack_wino_weight,   # noqa: F401
                      pack_wino43_weight, pack_wino4_weight, pack_conv_weight_f16, unpack_conv_weight_f16,
                      pack_conv_weight_f16x, unpack_conv_weight_f16x, pack_for_kind)

ACT_RES_AFTER = 0x10
BN_EPS_DEFAULT = 1e-5
SLOT_ARENA, SLOT_WEIGHTS, SLOT_USER0 = 0, 1, 2
# (cin, cout) classes of 3x3 stride-2 layers that precision = 'f16s2' leaves on their fp32 kernels because the f16-operand
# op was measured not to win on them (tools/precision_bench.py --s2); empty unless a measurement fills it.
#   48 -> 48: faster at 64 crops (64^2 input 35.7 -> 19.0 us, 32^2 input 14.7 -> 9.9 us) but SLOWER beyond the spread at 16
#   crops on the 32^2 input: fp32 (cfg 85) 7.8 us (spread 0.9), f16-operand op 8.9 us (spread 0.7) -- 64 blocks, the
#   latency of one block.  (64^2 input at 16 crops: 14.7 -> 9.6 us.)
F16S2_FP32_CLASSES = ((48, 48),)
# (cin, cout, stride) classes that precision = 'f16x' leaves on their fp32 kernels because the f16-operand op was measured
# not to win on them (tools/precision_bench.py --x); empty unless a measurement fills it.
#   Empty: all sixteen classes of W32 at 192 x 256 and of W48's seven layers are faster beyond the spread at 64 crops
#   (1.6-4.0x) and at 16 (1.2-5.7x; the smallest win is 256 -> 48 stride 1 at 16 crops, 55.3 -> 45.9 us, spreads 2.2 / 1.2).
F16X_FP32_CLASSES = ()
# (cin, cout, stride) classes of PRODUCERS that activations = 'f16' leaves on fp32 storage because the producer + consumer
# pair was measured not to win with f16 storage (tools/precision_bench.py --a); empty unless a measurement
# fills it.  Looked up at every call, like the tuples above.
#   The rule (3.16b): a class keeps f16 storage only if its pair is faster by more than the spread (max - min of 7 passes,
#   the larger of the two) at 64 crops and not slower beyond it at 16, in every pair it produces.  Measured
#   (profiles/f16_storage_bench.json; us of producer + consumer, fp32 storage -> f16 storage, spreads in brackets): the f16
#   median is the lower one in all 26 rows (1.03-1.18x), but only 48 -> 48 (77.8 -> 72.3 [3.6 / 4.8]), 64 -> 64 (30.2 -> 28.4
#   [0.5 / 0.8]) and 64 -> 64 /2 (27.6 -> 23.4 [1.8 / 1.5]) win beyond the spread at 64 crops.  Within the spread there:
#     32 -> 32       36.8 -> 33.7 [0.4 / 3.3]       32 -> 32 /2    20.4 -> 18.8 [1.5 / 5.0], 24.5 -> 22.4 [2.6 / 2.8]
#     96 -> 96       53.8 -> 51.4 [6.5 / 0.8]       96 -> 96 /2    39.6 -> 37.6 [4.8 / 4.4]
#     128 -> 128     42.5 -> 40.6 [0.6 / 7.2]       192 -> 192     59.7 -> 57.7 [1.2 / 7.2]
#     256 -> 256     60.1 -> 53.3 [13.5 / 14.6]     384 -> 384     86.4 -> 84.2 [3.9 / 0.6]
F16_STORAGE_FP32_CLASSES = ((32, 32, 1), (32, 32, 2), (96, 96, 1), (96, 96, 2), (128, 128, 1), (192, 192, 1), (256, 256, 1),
                            (384, 384, 1))
# Every value of the storage switch (PoseHighResolutionNet.activations), independent of ``precision``.
ACTIVATIONS = ('f32', 'f16')

# THE f16-operand lowering rules, one row per value of the switch, in the order the values extend each other:
# a precision activates its own row and every row above it (``active_rules``), and a layer goes to the first active row
# that takes it.  Everything the three modes do differently is a field here; ``eligible``, ``takes``, ``_Recorder.conv``,
# ``Program._emit`` and ``lowered_cost`` read the fields and name no mode.
#   kind          the recorded op ('res' / 'stride' are keys of its dict where res_arg / stride_arg say so)
#   strides       the strides of the 3x3 / pad 1 layers it takes; klass[i] names the class at strides[i] (bench.py parses it)
#   res_strides   the strides at which a residual may come with the layer
#   applies, add  the library's host-only predicate and its egn_program_add_* entry; res_arg / stride_arg: whether their
#                 argument lists carry has_res / res and the stride (an entry of one stride has it in its name)
#   fp32_classes  the NAME of the module-level tuple of classes measured not to win (looked up at every call: tests and
#                 tools assign to it), keyed by the first ``class_key`` of (cin, cout, stride); None: no such tuple
#   pack          the filter layout its kernel instances read (filters.py)
#   ck            the input channels per chunk of those instances: what egn_program_add_conv3x3_h16 -- the one entry of an
#                 op with f16 storage (``f16_storage``) -- is told beside the stride
F16Rule = collections.namedtuple('F16Rule', 'mode kind strides klass res_strides applies add res_arg stride_arg '
                                            'fp32_classes class_key pack ck')
F16_RULES = (
    # the W48 widths at stride 1 (csrc/conv_h.hip, chunks of 48 channels)
    F16Rule(mode='f16', kind='convh', strides=(1,), klass=('conv3x3h',), res_strides=(1,),
            applies='egn_conv3x3_h_applies', add='egn_program_add_conv3x3_h', res_arg=True, stride_arg=False,
            fp32_classes=None, class_key=0, pack=pack_conv_weight_f16, ck=H_CK),
    # ... and at stride 2: no stride-2 layer of HRNet has a residual
    F16Rule(mode='f16s2', kind='convh2', strides=(2,), klass=('conv3x3s2h',), res_strides=(),
            applies='egn_conv3x3s2_h_applies', add='egn_program_add_conv3x3s2_h', res_arg=False, stride_arg=False,
            fp32_classes='F16S2_FP32_CLASSES', class_key=2, pack=pack_conv_weight_f16, ck=H_CK),
    # the 32-multiple widths at either stride (chunks of 32): HRNet-W32's stages, and in every width layer1's 64 -> 64,
    # the stem's second convolution and transition1
    F16Rule(mode='f16x', kind='convhx', strides=(1, 2), klass=('conv3x3hx', 'conv3x3hxs2'), res_strides=(1,),
            applies='egn_conv3x3_hx_applies', add='egn_program_add_conv3x3_hx', res_arg=True, stride_arg=True,
            fp32_classes='F16X_FP32_CLASSES', class_key=3, pack=pack_conv_weight_f16x, ck=32),
)
_RULE_OF_KIND = {rule.kind: rule for rule in F16_RULES}
# Every value the switch takes; PRECISIONS keeps its three values and its last entry.
ALL_PRECISIONS = ('f32',) + tuple(rule.mode for rule in F16_RULES)
PRECISIONS = ALL_PRECISIONS[:3]


def _or_text(names):
    return ', '.join(repr(v) for v in names[:-1]) + ' or %r' % (names[-1],)


_PRECISION_TEXT = _or_text(ALL_PRECISIONS)


def active_rules(precision):
    """The rows of ``F16_RULES`` that ``precision`` switches on: a prefix of the table, none for 'f32'."""
    if precision not in ALL_PRECISIONS:
        raise ValueError("precision must be %s, got %r" % (_PRECISION_TEXT, precision))
    return F16_RULES[:ALL_PRECISIONS.index(precision)]


def _applies(rule, n, h, w, cin, cs_in, cout, cs_out, has_res, act, stride):
    """The rule's C predicate on a layer of one of its strides, unless the layer's class is measured to stay on fp32."""
    if rule.fp32_classes and (cin, cout, stride)[:rule.class_key] in globals()[rule.fp32_classes]:
        return False
    args = (n, h, w, cin, cs_in, cout, cs_out) + ((int(has_res),) if rule.res_arg else ()) + (act,) + \
        ((stride,) if rule.stride_arg else ())
    return bool(getattr(_lib.lib(), rule.applies)(*args))


def eligible(rule, conv, n, h, w):
    """Whether ``rule`` moves the module ``conv`` to the f16-operand kernels (csrc/conv_h.hip): a 3x3 / pad 1 nn.Conv2d of
    one of the rule's strides without bias, groups or dilation, the rule's host-only predicate takes its [n, Cin, h, w]
    input (unpadded channel strides), and its class is not among the rule's fp32 exceptions.  The epilogue is not the
    module's: the recorder asks the same predicate with the layer's own (``takes``; every such layer of HRNet has a plain
    one: folded BatchNorm, optional residual, ReLU or none)."""
    if not isinstance(conv, nn.Conv2d) or conv.stride[0] not in rule.strides:
        return False
    s = conv.stride[0]
    if (tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding), tuple(conv.dilation), conv.groups) != \
            ((3, 3), (s, s), (1, 1), (1, 1), 1) or conv.bias is not None or conv.padding_mode != 'zeros':
        return False
    cin, cout = conv.in_channels, conv.out_channels
    return _applies(rule, n, h, w, cin, cin, cout, cout, False, ACT_RELU, s)


def takes(rule, x, weight, bias, act, res, stride, pad, out_nchw=False, cout_cs=None, dst_given=False):
    """``eligible`` on a recorded layer: the same C predicate, asked with the layer's own epilogue."""
    cout, cin, kh, kw = weight.shape
    if (kh, kw, pad) != (3, 3, 1) or stride not in rule.strides or bias is not None or out_nchw or cout_cs is not None or \
            dst_given or (res is not None and stride not in rule.res_strides):
        return False
    return _applies(rule, x.n, x.h, x.w, cin, x.cs, cout, _round_up(cout, 4), res is not None, act, stride)


def check_activations(activations):
    """Refuses any value of the storage switch but 'f32' and 'f16'."""
    if activations not in ACTIVATIONS:
        raise ValueError("activations must be %s, got %r" % (_or_text(ACTIVATIONS), activations))
    return activations


def lowered_cost(kind, op):
    """(klass, flops, bytes) of a recorded 'convh' / 'convh2' / 'convhx' op, as ``Program.meta`` reports them: fp32
    activations (the residual read beside the output written) unless the op carries ``x16`` / ``y16`` (2 bytes an
    element), f16 filters."""
    rule, x, y = _RULE_OF_KIND[kind], op['x'], op['y']
    stride = op['stride'] if rule.stride_arg else rule.strides[0]
    flops = 2.0 * y.n * y.h * y.w * op['cout'] * op['cin'] * 9
    nbytes = (2.0 if op.get('x16') else 4.0) * x.n * x.h * x.w * op['cin'] + \
        y.n * y.h * y.w * op['cout'] * ((2.0 if op.get('y16') else 4.0) + (4.0 if op.get('res') is not None else 0.0)) + \
        2.0 * op['cout'] * op['cin'] * 9
    return '%s %d->%d@%dx%d' % (rule.klass[rule.strides.index(stride)], op['cin'], op['cout'], y.h, y.w), flops, nbytes


def f16_storage(rec):
    """THE rule of activations = 'f16' (DESIGN 3.16d), applied to a finished recording before ``plan_arena``: the set of
    ``Buf`` that are stored as f16.  A buffer qualifies iff it lies in the arena, exactly one op writes it -- a lowered
    op (a kind of ``F16_RULES``) as its ``y``, without a residual, whose (cin, cout, stride) is not in
    ``F16_STORAGE_FP32_CLASSES`` --, it has at least one reader, and every reader is a lowered op that takes it as ``x``
    and never as ``res``.  Such a reader rounds every element to f16 while it stages it; the producer applies the same
    rounding in its epilogue instead, so the reader's operand bits -- and every output of the network -- are the same.
    A qualifying buffer gets ``f16 = True`` and half its bytes, its producer ``op['y16']``, its readers ``op['x16']``."""
    fp32_classes = globals()['F16_STORAGE_FP32_CLASSES']
    out = set()
    for b in rec.bufs:
        if b.slot != SLOT_ARENA or not b.uses:
            continue
        writers, readers, ok = [], [], True
        for i in sorted(set(b.uses)):
            kind, op = rec.ops[i]
            if kind not in _RULE_OF_KIND or op.get('res') is b:
                ok = False
                break
            if op['y'] is b:
                writers.append((kind, op))
            if op['x'] is b:
                readers.append(op)
        if not ok or len(writers) != 1 or not readers:
            continue
        rule, w = _RULE_OF_KIND[writers[0][0]], writers[0][1]
        stride = w['stride'] if rule.stride_arg else rule.strides[0]
        if w.get('res') is not None or (w['cin'], w['cout'], stride) in fp32_classes or b.cs != b.c:
            continue
        b.f16 = True
        b.nbytes = b.n * b.h * b.w * b.c * 2
        w['y16'] = True
        for op in readers:
            op['x16'] = True
        out.add(b)
    return out


def f16_eligible(conv, n, h, w):
    """The layers precision = 'f16' moves to the f16-operand kernels (the first row of ``F16_RULES``): the 3x3 / stride 1 /
    pad 1 convolutions of the W48 widths that egn_conv3x3_h_applies takes."""
    return eligible(F16_RULES[0], conv, n, h, w)


def f16s2_eligible(conv, n, h, w):
    """The layers precision = 'f16s2' moves BESIDE those ``f16_eligible`` names (the second row): the 3x3 / stride 2 / pad 1
    convolutions that egn_conv3x3s2_h_applies takes and whose (cin, cout) class is not in ``F16S2_FP32_CLASSES``."""
    return eligible(F16_RULES[1], conv, n, h, w)


def f16x_eligible(conv, n, h, w):
    """The layers precision = 'f16x' moves BESIDE those ``f16_eligible`` and ``f16s2_eligible`` name (the third row): the
    3x3 / pad 1 convolutions of stride 1 or 2 that egn_conv3x3_hx_applies takes and whose (cin, cout, stride) class is not
    in ``F16X_FP32_CLASSES``."""
    return eligible(F16_RULES[2], conv, n, h, w)


class f16_emulation(object):
    """Context manager: the torch graph of ``model`` computing what precision = 'f16' computes, up to the fp32 summation
    order -- every ``f16_eligible`` convolution sees its input as f16(clamp(x, +-65504)) and its filter as f16(w), both
    round-to-nearest-even and widened back to fp32.  The measuring stick of the mode's network-level error (CPU or any
    device; tests/golden/make_f16_bounds.py, tools/precision_bench.py), never a way to run the network.
    ``precision='f16s2'`` also rounds the operands of the ``f16s2_eligible`` convolutions, ``precision='f16x'`` those and
    the ``f16x_eligible`` ones."""

    def __init__(self, model, precision='f16'):
        if precision not in ALL_PRECISIONS[1:]:
            raise ValueError("f16_emulation: precision must be %s, got %r" % (_or_text(ALL_PRECISIONS[1:]), precision))
        self.model, self.handles, self.saved, self.hit = model, [], {}, []
        self.rules = active_rules(precision)

    def _pre(self, mod, args):
        x = args[0]
        if x.dim() != 4 or not any(eligible(rule, mod, x.shape[0], x.shape[2], x.shape[3]) for rule in self.rules):
            return None
        self.saved[mod] = mod.weight.data
        mod.weight.data = mod.weight.data.half().float()
        self.hit.append(mod)
        return (x.clamp(-65504.0, 65504.0).half().float(),) + tuple(args[1:])

    def _post(self, mod, args, out):
        if mod in self.saved:
            mod.weight.data = self.saved.pop(mod)

    def __enter__(self):
        for m in self.model.modules():
            if isinstance(m, nn.Conv2d):
                self.handles += [m.register_forward_pre_hook(self._pre), m.register_forward_hook(self._post)]
        return self

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()
        for mod, w in self.saved.items():
            mod.weight.data = w
        self.handles, self.saved = [], {}
        return False


def fold_scale_shift(cout, bias=None, bn=None):
    """Per-channel (scale, shift) so that  bn(conv(x) + bias) == conv(x)*scale + shift,
    eval-mode BatchNorm (running stats).  Computed in float64, stored fp32,
    zero padded to CoutP."""
    coutp = _round_up(cout, 16)
    scale = torch.ones(cout, dtype=torch.float64)
    shift = torch.zeros(cout, dtype=torch.float64)
    if bias is not None:
        shift = bias.detach().double().cpu().clone()
    if bn is not None:
        g = bn.weight.detach().double().cpu() if bn.weight is not None else torch.ones(cout, dtype=torch.float64)
        b = bn.bias.detach().double().cpu() if bn.bias is not None else torch.zeros(cout, dtype=torch.float64)
        inv = 1.0 / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
        s = g * inv
        shift = b + (shift - bn.running_mean.detach().double().cpu()) * s
        scale = s
    out_s = torch.zeros(coutp, dtype=torch.float32)
    out_b = torch.zeros(coutp, dtype=torch.float32)
    out_s[:cout] = scale.float()
    out_b[:cout] = shift.float()
    return out_s, out_b


def fold_pw(weight, bn):
    """A 1x1 filter [Cout,Cin,1,1] + eval-mode BatchNorm for csrc/conv_pw.hip: (W' [Cout*Cin] = scale * W, shift [Cout]),
    float64 arithmetic, one rounding to fp32 -- the kernel's lanes read float4 pieces of the row-major matrix as it lies."""
    cout, cin = weight.shape[:2]
    scale, shift = fold_scale_shift(cout, None, bn)
    w = weight.detach().double().cpu().reshape(cout, cin) * scale[:cout].double()[:, None]
    return w.float().reshape(-1).contiguous(), shift[:cout].clone()


# ---------------------------------------------------------------------------
# symbolic recording
# ---------------------------------------------------------------------------
class Buf(object):
    """Symbolic fp32 tensor.  NHWC [n,h,w,cs] (cs = channel stride) in the arena,
    or an external user tensor bound to ``slot``."""
    __slots__ = ('n', 'h', 'w', 'c', 'cs', 'slot', 'off', 'nbytes', 'first', 'last', 'uses', 'name', 'f16')

    def __init__(self, n, h, w, c, cs=None, slot=SLOT_ARENA, nbytes=None, name=''):
        self.n, self.h, self.w, self.c = n, h, w, c
        self.cs = _round_up(c, 4) if cs is None else cs
        self.slot = slot
        self.off = 0
        self.nbytes = nbytes if nbytes is not None else n * h * w * self.cs * 4
        self.first = self.last = -1
        self.uses = []          # indices of every op that reads or writes the buffer
        self.name = name
        self.f16 = False        # stored as f16 between two f16-operand convs (``f16_storage``)

    def ref(self):
        return Ref(self.slot, self.off)


class _Recorder(object):
    def __init__(self):
        self.ops = []          # (kind, dict)
        self.blobs = []        # list of 1-D fp32 tensors -> weights blob
        self.blob_off = 0
        self.bufs = []
        self.region = 0        # fork/join regions are totally ordered
        self.cur_lane = 0      # launch lane inside the current region
        self._pending = {}     # lane -> tokens its next op waits for (``wait``)
        self._before = None    # happens_before's closure, rebuilt after every new op
        self.rules = ()        # the active rows of F16_RULES: a 3x3 conv one of them takes is recorded as its op kind

    def _push(self, kind, op):
        op['region'], op['lane'] = self.region, self.cur_lane
        if kind not in ('fork', 'join'):
            # waits asked for on this lane (``wait``) belong to the first op recorded on it afterwards
            op['waits'] = self._pending.pop(self.cur_lane, [])
        self.ops.append((kind, op))
        self._before = None

    def fork(self):
        """Ops recorded until ``join`` may run concurrently when they are on
        different lanes (``lane(k)``); they must be independent."""
        self.region += 1
        self.cur_lane = 0
        self._push('fork', {})

    def lane(self, k):
        self.cur_lane = k % 4

    def join(self):
        assert not self._pending, 'a wait with no op behind it on lanes %s' % sorted(self._pending)
        self.cur_lane = 0
        self._push('join', {})
        self.region += 1

    def signal(self):
        """Mark the op recorded last: its lane records an event behind it.  Returns the token ``wait`` takes."""
        kind, op = self.ops[-1]
        assert kind not in ('fork', 'join')
        op['signal'] = True
        return len(self.ops) - 1

    def wait(self, token):
        """The next op recorded on the current lane starts only after the op ``token`` names is complete."""
        assert self.ops[token][1].get('signal'), token
        self._pending.setdefault(self.cur_lane, []).append(token)

    def happens_before(self, u, d):
        """Op u is complete before op d starts: the transitive closure of "earlier region", "same region and same
        lane, in op order (stream order)" and the signal -> wait edges."""
        if self.ops[u][1]['region'] < self.ops[d][1]['region']:
            return True
        if self._before is None:
            # before[d]: bit set of the ops complete before d through lane order and signal -> wait edges alone (a
            # chain through an earlier region ends in an earlier region: the first test has it)
            before, last = [], {}
            for i, (kind, op) in enumerate(self.ops):
                at = (op['region'], op['lane'])
                preds = ([last[at]] if at in last else []) + list(op.get('waits', ()))
                m = 0
                for p in preds:
                    m |= before[p] | (1 << p)
                before.append(m)
                last[at] = i
            self._before = before
        return bool((self._before[d] >> u) & 1)

    # -- storage --
    def new(self, n, h, w, c, name=''):
        b = Buf(n, h, w, c, name=name)
        self.bufs.append(b)
        return b

    def weight(self, t):
        off = self.blob_off
        self.blobs.append(t)
        self.blob_off += _round_up(t.numel() * 4, 256)
        return Ref(SLOT_WEIGHTS, off)

    def _touch(self, *bufs):
        i = len(self.ops)
        for b in bufs:
            if b is None:
                continue
            if b.first < 0:
                b.first = i
            b.last = i
            b.uses.append(i)

    # -- ops --
    def conv(self, x, weight, bias=None, bn=None, act=ACT_NONE, res=None, stride=1, pad=0,
             dst=None, out_nchw=False, cout_cs=None, tag=''):
        cout, cin, kh, kw = weight.shape
        assert cin == x.c, (cin, x.c, tag)
        ho = (x.h + 2 * pad - kh) // stride + 1
        wo = (x.w + 2 * pad - kw) // stride + 1
        dst_given = dst is not None
        if dst is None:
            dst = self.new(x.n, ho, wo, cout, name=tag)
            if cout_cs is not None:
                dst.cs = cout_cs
                dst.nbytes = x.n * ho * wo * cout_cs * 4
        for rule in self.rules:
            if takes(rule, x, weight, bias, act, res, stride, pad, out_nchw, cout_cs, dst_given):
                scale, shift = fold_scale_shift(cout, None, bn)
                op = dict(x=x, w=self.weight(rule.pack(weight)), scale=self.weight(scale), shift=self.weight(shift),
                          y=dst, cin=cin, cout=cout, act=act, tag=tag)
                if rule.res_arg:
                    op['res'] = res
                if rule.stride_arg:
                    op['stride'] = stride
                self._touch(x, res, dst)
                # rule.kind -- self._push('convh', op), self._push('convh2', op) or self._push('convhx', op): spelled out for
                # tests/program_ops_sweep.py, which reads the kinds a program can hold from this file's text (and
                # tests/test_f16_rules_cpu.py holds the table to this list)
                self._push(rule.kind, op)
                return dst
        scale, shift = fold_scale_shift(cout, bias, bn)
        # the filter is packed when the program is built: the layout depends on the tile
        # configuration the tuner picks for the shape (direct vs Winograd kernels)
        op = dict(x=x, w=None, w_src=weight, scale=self.weight(scale),
                  shift=self.weight(shift), res=res, y=dst, cin=cin, cout=cout, kh=kh, kw=kw,
                  stride=stride, pad=pad, act=act, out_nchw=int(out_nchw), ho=ho, wo=wo, tag=tag)
        self._touch(x, res, dst)
        self._push('conv', op)
        return dst

    @staticmethod
    def takes_f16(x, weight, bias, act, res, stride, pad, out_nchw=False, cout_cs=None, dst_given=False):
        """``f16_eligible`` on a recorded layer."""
        return takes(F16_RULES[0], x, weight, bias, act, res, stride, pad, out_nchw, cout_cs, dst_given)

    @staticmethod
    def takes_f16s2(x, weight, bias, act, res, stride, pad, out_nchw=False, cout_cs=None, dst_given=False):
        """``f16s2_eligible`` on a recorded layer."""
        return takes(F16_RULES[1], x, weight, bias, act, res, stride, pad, out_nchw, cout_cs, dst_given)

    @staticmethod
    def takes_f16x(x, weight, bias, act, res, stride, pad, out_nchw=False, cout_cs=None, dst_given=False):
        """``f16x_eligible`` on a recorded layer."""
        return takes(F16_RULES[2], x, weight, bias, act, res, stride, pad, out_nchw, cout_cs, dst_given)

    def conv_pair(self, xa, conv_a, bn_a, act_a, res_a, xb, conv_b, bn_b, act_b, res_b, tag=''):
        """Two independent 3x3 / stride 1 / pad 1 convolutions (+ folded BatchNorm, residual, ReLU) as ONE launch
        (csrc/conv_wino4.hip, conv_wino4_pair_kernel): ``a`` as tile configuration 86 runs it, ``b`` as 82 does.  The
        caller asked ``tuner.pair_usable`` first.  Returns (ya, yb).  Only the inference recorder has this op: the
        training tape records its layers one by one."""
        halves = []
        for x, conv, bn, act, res, which in ((xa, conv_a, bn_a, act_a, res_a, 'a'), (xb, conv_b, bn_b, act_b, res_b, 'b')):
            cout, cin, kh, kw = conv.weight.shape
            assert (cin, kh, kw) == (x.c, 3, 3) and x.cs == x.c and cout % 4 == 0, (conv.weight.shape, x.c, x.cs, tag)
            y = self.new(x.n, x.h, x.w, cout, name='%s.%s' % (tag, which))
            scale, shift = fold_scale_shift(cout, None, bn)
            halves.append(dict(x=x, w=None, w_src=conv.weight, scale=self.weight(scale), shift=self.weight(shift), res=res,
                               y=y, cin=cin, cout=cout, act=act))
        self._touch(*[h[k] for h in halves for k in ('x', 'res', 'y')])
        self._push('convpair', dict(a=halves[0], b=halves[1], tag=tag))
        return halves[0]['y'], halves[1]['y']

    def fuse(self, terms, relu, tag=''):
        """terms: list of (Buf, shift); output resolution = that of a shift-0 term."""
        base = [t for t, s in terms if s == 0][0]
        y = self.new(base.n, base.h, base.w, base.c, name=tag)
        self._touch(y, *[t for t, _ in terms])
        self._push('fuse', dict(y=y, terms=terms, relu=int(relu), tag=tag))
        return y

    def pw_pair(self, h, conv3, bn3, res, relu1, conv1=None, bn1=None, tag=''):
        """layer1's 1x1 pair as one launch (csrc/conv_pw.hip): out = act(bn3(conv3(h)) (+ res)) [64 -> 256] and, with
        conv1, hn = relu(bn1(conv1(out))) [256 -> 64].  Returns (out, hn or None)."""
        assert tuple(conv3.weight.shape) == (256, 64, 1, 1) and h.c == 64 and h.cs == 64, (conv3.weight.shape, h.c, h.cs)
        out = self.new(h.n, h.h, h.w, 256, name=tag + '.out')
        w3, s3 = fold_pw(conv3.weight, bn3)
        op = dict(h=h, res=res, out=out, hn=None, w3=self.weight(w3), shift3=self.weight(s3), w1=None, shift1=None,
                  relu1=int(relu1), m=h.n * h.h * h.w, tag=tag)
        hn = None
        if conv1 is not None:
            assert tuple(conv1.weight.shape) == (64, 256, 1, 1), conv1.weight.shape
            hn = self.new(h.n, h.h, h.w, 64, name=tag + '.next')
            w1, s1 = fold_pw(conv1.weight, bn1)
            op.update(hn=hn, w1=self.weight(w1), shift1=self.weight(s1))
        self._touch(h, res, out, hn)
        self._push('pwpair', op)
        return out, hn

    def nchw_to_nhwc(self, x_ext, n, c, h, w, tag=''):
        y = self.new(n, h, w, c, name=tag)
        self._touch(y)
        self._push('to_nhwc', dict(x=x_ext, y=y, tag=tag))
        return y

    def nhwc_to_nchw(self, x, c, dst_ext, tag=''):
        self._touch(x)
        self._push('to_nchw', dict(x=x, y=dst_ext, c=c, tag=tag))

    def pixel_shuffle(self, x, c, up, dst_ext, tag=''):
        self._touch(x)
        self._push('pixshuf', dict(x=x, y=dst_ext, c=c, up=up, tag=tag))

    def ramps(self, y, c0, tag=''):
        self._touch(y)
        self._push('ramps', dict(y=y, c0=c0, tag=tag))

    def decode(self, hm_ext, n, k, h, w, mode, xy, mx, idx, tag=''):
        self._push('decode', dict(hm=hm_ext, n=n, k=k, h=h, w=w, mode=mode, xy=xy, mx=mx, idx=idx, tag=tag))

    # -- finalisation --
    def plan_arena(self):
        """Greedy best-fit packing of arena buffers by lifetime; returns bytes.
        A buffer's storage is re-used only by a buffer whose defining op starts
        after EVERY use of the old one has completed (``happens_before``), so
        concurrent lanes never alias each other's live tensors.
        With f16-stored buffers (``f16_storage``) the packing is never larger than that of the fp32 program: a greedy
        packing of smaller buffers can come out larger, and then every f16 buffer keeps the place -- and the room -- of
        its fp32 size."""
        top = self._place(lambda b: b.nbytes)
        if any(b.f16 for b in self.bufs):
            offs = [b.off for b in self.bufs]
            top32 = self._place(lambda b: 2 * b.nbytes if b.f16 else b.nbytes)
            if top32 < top:
                return top32
            for b, off in zip(self.bufs, offs):
                b.off = off
        return top

    def _place(self, size):
        """``plan_arena`` with ``size(buf)`` bytes of room per buffer: sets every ``off``, returns the arena's bytes."""
        live = [b for b in self.bufs if b.slot == SLOT_ARENA and b.first >= 0]
        events = sorted(live, key=lambda b: b.first)
        free = []              # [off, size, uses]: uses = op indices that touched the bytes
        active = []
        top = 0
        for b in events:
            d = b.first
            region_d = self.ops[d][1]['region']
            # retire buffers with no later use: their bytes become candidates, tagged
            # with the uses a new owner has to wait for
            still = []
            for ab in active:
                if ab.last < d:
                    free.append([ab.off, _round_up(size(ab), 256), list(ab.uses)])
                else:
                    still.append(ab)
            active = still
            # uses in earlier regions are ordered before everything from here on
            for blk in free:
                blk[2] = [u for u in blk[2] if self.ops[u][1]['region'] >= region_d]
            free.sort(key=lambda blk: blk[0])
            merged = []
            for off, sz, uses in free:
                if merged and merged[-1][0] + merged[-1][1] == off:
                    merged[-1][1] += sz
                    merged[-1][2] = merged[-1][2] + uses
                else:
                    merged.append([off, sz, uses])
            free = merged

            def usable(blk):
                return all(self.happens_before(u, d) for u in blk[2])

            need = _round_up(size(b), 256)
            best = None
            for i, blk in enumerate(free):
                if blk[1] >= need and usable(blk) and (best is None or blk[1] < free[best][1]):
                    best = i
            if best is None:
                # grow: extend a usable free block that ends at the top if there is one
                if free and free[-1][0] + free[-1][1] == top and usable(free[-1]):
                    off, sz, uses = free.pop()
                    b.off = off
                    top = off + need
                else:
                    b.off = top
                    top += need
            else:
                off, sz, uses = free.pop(best)
                b.off = off
                if sz > need:
                    free.append([off + need, sz - need, uses])
            active.append(b)
        return top

    def pack_pending(self):
        """Filters no tile configuration was chosen for get the direct layout."""
        for kind, op in self.ops:
            if kind == 'conv' and op.get('w') is None:
                op['w'] = self.weight(pack_conv_weight(op['w_src']))

    def weights_blob(self, device):
        self.pack_pending()
        blob = torch.zeros(max(self.blob_off, 256) // 4, dtype=torch.float32)
        off = 0
        for t in self.blobs:
            blob[off // 4: off // 4 + t.numel()] = t
            off += _round_up(t.numel() * 4, 256)
        return blob.to(device)


for _rule in F16_RULES:          # r.f16, r.f16s2, r.f16x: whether the recorder lowers by the row of that mode
    setattr(_Recorder, _rule.mode, property(lambda self, rule=_rule: rule in self.rules))


class ProgramCalls(object):
    """THE place every call that builds an egn_program goes through (``Program._emit``, for HRNet and lifter programs
    alike): ``calls(name, *args)`` calls the library's entry ``name(handle, *args)`` and checks its code, and -- with
    a ``log`` -- appends (name, args) first.  A list among the arguments (the fuse terms and shifts, the waits) becomes
    the C array the entry takes.  Without a handle nothing is called: the log alone is the program, which is how
    egonet_amd.plan writes the launch list of a model to a file (no GPU needed: K-split ops allocate device words when
    they are added)."""

    def __init__(self, lib=None, handle=None, log=None):
        self.lib, self.handle, self.log = lib, handle, log

    def __call__(self, name, *args, what='', unchecked=False):
        if self.log is not None:
            self.log.append((name, args))
        if self.handle is None:
            return
        cargs = []
        for a in args:
            if isinstance(a, list):
                a = ((Ref if a and isinstance(a[0], Ref) else C.c_int) * len(a))(*a)
            cargs.append(a)
        code = getattr(self.lib, name)(self.handle, *cargs)
        if not unchecked:
            _lib.check(code, what)


class Program(object):
    """Owns a native egn_program plus the torch storage its slots point to.  ``log``: a list that receives every
    building call (``ProgramCalls``); ``native=False``: only that log, the arena size and the packed weights are made --
    no device storage, no egn_program (``device`` may then be None: nothing is measured, see ``_choose_and_pack``)."""

    def __init__(self, rec, device, n_user_slots, log=None, native=True, pack=pack_for_kind):
        self.device = device
        arena_bytes = rec.plan_arena()
        self.arena_bytes = arena_bytes
        self.tags = []
        self.meta = []
        self._choose_and_pack(rec, device, pack)
        if not native:
            rec.pack_pending()
            self.weight_bytes = rec.blob_off
            self.lib = self.handle = None
            self.call = ProgramCalls(log=log if log is not None else [])
            for kind, op in rec.ops:
                self._emit(kind, op)
            return
        L = _lib.lib()
        self.lib = L
        self.arena = torch.zeros(max(arena_bytes, 256) // 4, dtype=torch.float32, device=device)
        self.weights = rec.weights_blob(device)
        self.handle = C.c_void_p(L.egn_program_create(SLOT_USER0 + n_user_slots))
        if not self.handle:
            raise _lib.EgonetHipError('egn_program_create failed')
        self.weight_bytes = rec.blob_off
        self.call = ProgramCalls(L, self.handle, log)
        _lib.check(L.egn_program_bind(self.handle, SLOT_ARENA, _lib.ptr(self.arena)))
        _lib.check(L.egn_program_bind(self.handle, SLOT_WEIGHTS, _lib.ptr(self.weights)))
        # (ops may own device memory -- the ticket words of K-split convolutions: allocate it on the program's device)
        with torch.cuda.device(device):
            for kind, op in rec.ops:
                self._emit(kind, op)

    @staticmethod
    def _conv_key(op):
        x, y = op['x'], op['y']
        cs_out = y.cs if not op['out_nchw'] else op['cout']
        return (x.n, x.h, x.w, op['cin'], x.cs, op['cout'], cs_out, op['kh'], op['kw'], op['stride'],
                op['pad'], op['res'] is not None, bool(op['out_nchw']))

    @staticmethod
    def _conv_kinds(op):
        """The filter kinds the program feeds this conv (tuner.usable): Winograd only behind a plain epilogue."""
        plain_act = (op['act'] & 0xf) in (ACT_NONE, ACT_RELU) and not (op['act'] & ACT_RES_AFTER)
        return tuner.ALL_KINDS if plain_act else tuner.DIRECT

    def _choose_and_pack(self, rec, device, pack=pack_for_kind):
        """Tile configuration per conv (measured table / autotune) and the filter in the layout
        that configuration's kernel stages through LDS.  ``device`` None: the table's choice or the cost model's 0,
        never a measurement.  ``pack``: ``pack_for_kind`` or a caller's memo of it."""
        for kind, op in rec.ops:
            if kind == 'convpair':          # both halves read the F(4x4,3x3) register-feed layout (configs 86 / 82)
                for half in (op['a'], op['b']):
                    if half['w'] is None:
                        half['w'] = rec.weight(pack(half['w_src'], 3))
                continue
            if kind != 'conv' or op.get('w') is not None:
                continue
            if 'cfg' not in op:
                op['cfg'] = tuner.choose(device, self._conv_key(op), self._conv_kinds(op), measure=device is not None)
            op['w'] = rec.weight(pack(op['w_src'], tuner.kind_of(op['cfg'])))

    def _emit(self, kind, op):
        call = self.call
        flops, nbytes = 0.0, 0.0
        if kind in ('fork', 'join'):
            call('egn_program_fork' if kind == 'fork' else 'egn_program_join')
            self.meta.append(dict(kind=kind, klass=kind, tag='', flops=0.0, bytes=0.0, cfg=0))
            return
        call('egn_program_set_lane', op.get('lane', 0))
        if kind == 'conv':
            x, y = op['x'], op['y']
            res = op['res'].ref() if op['res'] is not None else NULL_REF
            cs_out = y.cs if not op['out_nchw'] else op['cout']
            call('egn_program_add_conv2d', x.ref(), op['w'], op['scale'], op['shift'], res, y.ref(),
                 x.n, x.h, x.w, op['cin'], x.cs, op['cout'], cs_out, op['kh'], op['kw'],
                 op['stride'], op['pad'], op['act'], op['out_nchw'], op.get('cfg', 0), what=op['tag'])
            m = x.n * op['ho'] * op['wo']
            flops = 2.0 * m * op['cout'] * op['cin'] * op['kh'] * op['kw']
            nbytes = 4.0 * (x.n * x.h * x.w * op['cin'] + m * op['cout'] * (2 if op['res'] is not None else 1)
                            + op['cout'] * op['cin'] * op['kh'] * op['kw'])
            klass = 'conv%dx%ds%d %d->%d@%dx%d' % (op['kh'], op['kw'], op['stride'], op['cin'],
                                                    op['cout'], op['ho'], op['wo'])
        elif kind in _RULE_OF_KIND:
            rule, x, y = _RULE_OF_KIND[kind], op['x'], op['y']
            if op.get('x16') or op.get('y16'):
                # f16 storage of x and / or y: the one entry of all three kinds (chunk size and stride say which)
                res = op['res'].ref() if op.get('res') is not None else NULL_REF
                call('egn_program_add_conv3x3_h16', x.ref(), op['w'], op['scale'], op['shift'], res, y.ref(), x.n, x.h, x.w,
                     op['cin'], op['cout'], op['act'], op['stride'] if rule.stride_arg else rule.strides[0],
                     rule.ck, int(bool(op.get('x16'))),
                     int(bool(op.get('y16'))), what=op['tag'])
            else:
                res = [op['res'].ref() if op['res'] is not None else NULL_REF] if rule.res_arg else []
                call(rule.add, *([x.ref(), op['w'], op['scale'], op['shift']] + res +
                                 [y.ref(), x.n, x.h, x.w, op['cin'], op['cout'], op['act']] +
                                 ([op['stride']] if rule.stride_arg else [])), what=op['tag'])
            klass, flops, nbytes = lowered_cost(kind, op)
        elif kind == 'convpair':
            args, klass = [], []
            for half in (op['a'], op['b']):
                x, y = half['x'], half['y']
                res = half['res'].ref() if half['res'] is not None else NULL_REF
                args += [x.ref(), half['w'], half['scale'], half['shift'], res, y.ref(), x.n, x.h, x.w, half['cin'],
                         half['cout'], half['act']]
                m = x.n * x.h * x.w
                flops += 2.0 * m * half['cout'] * half['cin'] * 9
                nbytes += 4.0 * (m * half['cin'] + m * half['cout'] * (2 if half['res'] is not None else 1)
                                 + half['cout'] * half['cin'] * 9)
                klass.append('%d->%d@%dx%d' % (half['cin'], half['cout'], x.h, x.w))
            call('egn_program_add_conv2d_pair', *(args + [0]), what=op['tag'])
            klass = 'convpair3x3s1 ' + ' + '.join(klass)
        elif kind == 'fuse':
            y = op['y']
            terms = op['terms']
            call('egn_program_add_fuse', y.ref(), y.n, y.h, y.w, y.c, y.cs, len(terms), [t.ref() for t, _ in terms],
                 [s for _, s in terms], op['relu'], what=op['tag'])
            nbytes = 4.0 * y.n * y.c * (y.h * y.w + sum((y.h >> s) * (y.w >> s) for _, s in terms))
            klass = 'fuse%d %d@%dx%d' % (len(terms), y.c, y.h, y.w)
        elif kind == 'to_nhwc':
            y = op['y']
            call('egn_program_add_nchw_to_nhwc', op['x'], y.ref(), y.n, y.c, y.h, y.w, y.cs)
            nbytes = 4.0 * y.n * y.h * y.w * (y.c + y.cs)
            klass = 'nchw2nhwc %d@%dx%d' % (y.c, y.h, y.w)
        elif kind == 'to_nchw':
            x = op['x']
            call('egn_program_add_nhwc_to_nchw', x.ref(), op['y'], x.n, op['c'], x.h, x.w, x.cs)
            nbytes = 8.0 * x.n * x.h * x.w * op['c']
            klass = 'nhwc2nchw %d@%dx%d' % (op['c'], x.h, x.w)
        elif kind == 'pixshuf':
            x = op['x']
            call('egn_program_add_pixel_shuffle', x.ref(), op['y'], x.n, op['c'], x.h, x.w, x.cs, op['up'])
            nbytes = 8.0 * x.n * x.h * x.w * op['c'] * op['up'] ** 2
            klass = 'pixel_shuffle%d %d@%dx%d' % (op['up'], op['c'], x.h, x.w)
        elif kind == 'pwpair':
            hb, rb, ob, nb = op['h'], op['res'], op['out'], op['hn']
            none = NULL_REF
            call('egn_program_add_pw_pair', hb.ref(), rb.ref() if rb is not None else none, op['w3'], op['shift3'],
                 op['w1'] if nb is not None else none, op['shift1'] if nb is not None else none, ob.ref(),
                 nb.ref() if nb is not None else none, op['m'], op['relu1'])
            flops = 2.0 * op['m'] * 64 * 256 * (2 if nb is not None else 1)
            nbytes = 4.0 * op['m'] * (64 + 256 * (2 if rb is not None else 1) + (64 if nb is not None else 0))
            klass = 'pwpair%d%d 64->256%s@%dx%d' % (int(rb is not None), op['relu1'], '->64' if nb is not None else '',
                                                    hb.h, hb.w)
        elif kind == 'ramps':
            y = op['y']
            call('egn_program_add_ramps', y.ref(), y.n, y.h, y.w, y.cs, op['c0'])
            nbytes = 8.0 * y.n * y.h * y.w
            klass = 'ramps'
        elif kind == 'decode':
            call('egn_program_add_decode', op['hm'], op['n'], op['k'], op['h'], op['w'], op['mode'], op['xy'], op['mx'],
                 op['idx'])
            nbytes = 4.0 * op['n'] * op['k'] * op['h'] * op['w']
            klass = 'decode%d %dx%d' % (op['mode'], op['h'], op['w'])
        else:
            raise ValueError(kind)
        call('egn_program_tag', (op.get('tag') or klass).encode(), flops, nbytes, unchecked=True)
        if op.get('signal') or op.get('waits'):     # (tokens are op indices: the program has one op per recorded op)
            waits = op.get('waits', [])
            call('egn_program_set_deps', int(bool(op.get('signal'))), list(waits), len(waits), what=op.get('tag', ''))
        self.meta.append(dict(kind=kind, klass=klass, tag=op.get('tag', ''), flops=flops, bytes=nbytes,
                              cfg=op.get('cfg', 0) if kind == 'conv' else 0))

    def bind(self, slot, tensor):
        _lib.check(self.lib.egn_program_bind(self.handle, slot, _lib.ptr(tensor)))

    def run(self):
        _lib.check(self.lib.egn_program_run(self.handle, _lib.current_stream(self.device)), 'program_run')

    def run_timed(self):
        n = self.lib.egn_program_num_ops(self.handle)
        ms = (C.c_float * n)()
        _lib.check(self.lib.egn_program_run_timed(self.handle, _lib.current_stream(self.device), ms, n))
        return np.array(ms[:], dtype=np.float64)

    def capture(self):
        _lib.check(self.lib.egn_program_capture(self.handle, _lib.current_stream(self.device)))

    def replay(self):
        _lib.check(self.lib.egn_program_replay(self.handle, _lib.current_stream(self.device)))

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                self.lib.egn_program_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


# ---------------------------------------------------------------------------
# staleness of the packed weights
# ---------------------------------------------------------------------------
class _Stamp(object):
    """Detects that a module's parameters / buffers changed since its programs were built.

    The packed blob folds EVERY parameter and BatchNorm buffer, so all of them are watched:
    the sum of their autograd version counters (optimizer steps, load_state_dict, in-place
    edits, BatchNorm running-stat updates), the XOR of their storage addresses (``.data = ...``,
    ``.to()``), their count, and a generation counter that code writing through raw pointers
    (the native training steps: their Adam / BatchNorm kernels never touch ``_version``) bumps
    with ``invalidate``.  ~0.2 ms on the host for the 1 828 tensors of HRNet-W48, hidden behind
    the asynchronous launches of the forward."""

    def __init__(self, model):
        self.model = model
        self.tensors = None
        self.last = None

    def _now(self):
        if self.tensors is None:
            self.tensors = list(self.model.parameters()) + list(self.model.buffers())
        ver, addr = 0, 0
        for t in self.tensors:
            ver += t._version
            addr ^= t.data_ptr()
        return (ver, addr, len(self.tensors), getattr(self.model, '_egn_generation', 0),
                self.tensors[0].device if self.tensors else None)

    def changed(self):
        now = self._now()
        if now != self.last:
            self.tensors = None          # something moved: enumerate the tensors afresh
            self.last = self._now()
            return True
        return False


def invalidate(model):
    """Tell the inference engines of ``model`` that its weights were written behind autograd's
    back (native training steps)."""
    model._egn_generation = getattr(model, '_egn_generation', 0) + 1
    model._engine = None


# ---------------------------------------------------------------------------
# HRNet
# ---------------------------------------------------------------------------
def _act_of(seq):
    return ACT_RELU if any(isinstance(m, nn.ReLU) for m in seq) else ACT_NONE


class HRNetEngine(object):
    """Runs ``PoseHighResolutionNet`` (eval mode) on one GPU as HIP kernels."""

    def __init__(self, model):
        import os
        self.model = model
        self.programs = {}        # (device, N, H, W, decode) -> Program
        self._stamp = _Stamp(model)
        self.lanes = os.environ.get('EGONET_AMD_LANES', '1') != '0'   # branch-level concurrency
        # batches up to this size replay their program as one hipGraph (_forward_graphed); 0 = never.  OFF by default:
        # replays are bit-identical and faster (16 crops: 5.16 -> 5.01 ms per step; 64 crops: 12.79 -> 12.60), but inside
        # the GPU test suite hipGraphLaunch crashed the interpreter after the autograd-bridge tests had run in the same
        # process (profiles/r5_graph_replay_crash.txt) -- not root-caused, so nothing depends on it
        self.graph_max_n = int(os.environ.get('EGONET_AMD_GRAPH_MAX_N', '0'))
        self.fuse_layer1 = os.environ.get('EGONET_AMD_PW_FUSE', '1') != '0'      # layer1's 1x1 pairs on csrc/conv_pw.hip
        # fuse output i -> branch i of the next module on the same lane, no join in between
        self.chain_regions = os.environ.get('EGONET_AMD_CHAIN', '1') != '0'
        # fuse term (i, j) waits for branch j alone instead of a join of all branches (_module); 0: the joins, for A/B runs
        self.deps = os.environ.get('EGONET_AMD_DEPS', '1') != '0'
        # ... from this many crops on: measured at 1 and 16 crops, only the larger was free of any regression
        self.deps_min_n = int(os.environ.get('EGONET_AMD_DEPS_MIN_N', '16'))
        self.last_f16_ops = []    # tags of the layers the last recording lowered to the f16-operand ops (precision = 'f16' / 'f16s2' / 'f16x')

    @property
    def precision(self):
        """The model's ``precision`` attribute ('f32', the default, 'f16', 'f16s2' or 'f16x'): read at every forward, part of
        the program key.  'f16' moves the layers ``f16_eligible`` names to csrc/conv_h.hip, 'f16s2' those and the layers
        ``f16s2_eligible`` names, 'f16x' those and the layers ``f16x_eligible`` names; everything else, and the training
        tape, is recorded exactly as in 'f32'."""
        prec = getattr(self.model, 'precision', 'f32')
        active_rules(prec)          # (refuses any other value)
        return prec

    @property
    def activations(self):
        """The model's ``activations`` attribute ('f32', the default, or 'f16'): read at every forward, part of the program
        key, independent of ``precision``.  'f16' stores the tensors ``f16_storage`` names -- written by one f16-operand
        conv, read only by f16-operand convs as their input -- as f16; every output keeps its bits.  With
        precision = 'f32' nothing is lowered and nothing qualifies.  The training tape ignores it."""
        return check_activations(getattr(self.model, 'activations', 'f32'))

    # -- recording ---------------------------------------------------------
    def _block(self, r, x, blk, tag):
        y = x
        for i in range(1, blk.depth + 1):
            conv = getattr(blk, 'conv%d' % i)
            bn = getattr(blk, 'bn%d' % i)
            k = conv.kernel_size[0]
            if i < blk.depth:
                y = r.conv(y, conv.weight, None, bn, ACT_RELU, None, conv.stride[0], conv.padding[0],
                           tag='%s.conv%d' % (tag, i))
            else:
                if blk.downsample is None:
                    res = x
                else:
                    pc, pb = blk.downsample[0], blk.downsample[1]
                    res = r.conv(x, pc.weight, None, pb, ACT_NONE, None, pc.stride[0], 0,
                                 tag=tag + '.downsample')
                y = r.conv(y, conv.weight, None, bn, ACT_RELU, res, conv.stride[0], conv.padding[0],
                           tag='%s.conv%d' % (tag, i))
        return y

    def _layer1(self, r, x, blocks):
        """layer1 (hrnet.py:325, 512-529: four Bottlenecks, 64 -> 256 channels).  Where the recorder has ``pw_pair`` (the
        inference recorder; the training tape walks the blocks layer by layer) each block's conv3 + residual + ReLU and
        the NEXT block's conv1 + ReLU are ONE launch of csrc/conv_pw.hip, the downsample conv and the last conv3 the same
        kernel's one-product form: the 256-channel tensor crosses HBM once per direction (EGONET_AMD_PW_FUSE=0: the
        general conv kernels, one launch per layer)."""
        def plain():
            t = x
            for k, blk in enumerate(blocks):
                t = self._block(r, t, blk, 'layer1.%d' % k)
            return t

        def is11(conv, cout, cin):
            return tuple(conv.weight.shape) == (cout, cin, 1, 1) and conv.stride[0] == 1 and conv.bias is None
        ok = self.fuse_layer1 and hasattr(r, 'pw_pair') and x.c == 64 and x.cs == 64 and (x.n * x.h * x.w) % 32 == 0 \
            and x.n * x.h * x.w * 256 * 4 < 2 ** 31 \
            and len(blocks) >= 1 and all(getattr(b, 'depth', 0) == 3 for b in blocks)
        if ok:
            for k, b in enumerate(blocks):
                ok = ok and is11(b.conv1, 64, 64 if k == 0 else 256) and is11(b.conv3, 256, 64) and \
                    tuple(b.conv2.weight.shape) == (64, 64, 3, 3) and b.conv2.stride[0] == 1
                if k == 0:
                    ok = ok and b.downsample is not None and is11(b.downsample[0], 256, 64)
                else:
                    ok = ok and b.downsample is None
        if not ok:
            return plain()
        b0 = blocks[0]
        h = r.conv(x, b0.conv1.weight, None, b0.bn1, ACT_RELU, None, 1, 0, tag='layer1.0.conv1')
        t = x
        for k, b in enumerate(blocks):
            h = r.conv(h, b.conv2.weight, None, b.bn2, ACT_RELU, None, 1, 1, tag='layer1.%d.conv2' % k)
            if k == 0:
                res, _ = r.pw_pair(t, b.downsample[0], b.downsample[1], None, False, tag='layer1.0.downsample')
            else:
                res = t
            nxt = blocks[k + 1] if k + 1 < len(blocks) else None
            t, h = r.pw_pair(h, b.conv3, b.bn3, res, True, nxt.conv1 if nxt is not None else None,
                             nxt.bn1 if nxt is not None else None, tag='layer1.%d.conv3' % k)
        return t

    def _unit_chain(self, r, x, seq_of_units, tag):
        """Sequential of Sequential(conv, bn[, relu]) (transition / fuse down paths)."""
        t = x
        for s, unit in enumerate(seq_of_units):
            conv, bn = unit[0], unit[1]
            t = r.conv(t, conv.weight, None, bn, _act_of(unit), None, conv.stride[0], conv.padding[0],
                       tag='%s.%d' % (tag, s))
        return t

    @staticmethod
    def _pair_branches(r, xs, mod):
        """(ia, ib) if branches ia and ib of ``mod`` run level by level as paired launches (``_Recorder.conv_pair``), else
        None: the recorder has the op (the training tape has not), both are chains of plain BasicBlocks of equal length,
        and ``tuner.pair_usable`` -- the one place that says whether a pair is used -- takes their shapes with and
        without the residual.  Stage 4 of W48 at 64 crops: the 192-channel 16 x 16 branch beside the 384-channel 8 x 8 one
        (hrnet.py:286-287: the branches are independent at every depth)."""
        if mod is None or not hasattr(r, 'conv_pair'):
            return None
        # a branch with a layer that any active f16-operand rule takes is never half of a pair
        lowered = [any(takes(rule, x, conv.weight, conv.bias, ACT_RELU, None, conv.stride[0], conv.padding[0])
                       for rule in getattr(r, 'rules', ()) for blk in b for conv in (blk.conv1, blk.conv2)
                       if getattr(blk, 'depth', 0) == 2)
                   for b, x in zip(mod.branches, xs)]

        def plain(branch, x):
            for blk in branch:
                if getattr(blk, 'depth', 0) != 2 or blk.downsample is not None:
                    return False
                for conv in (blk.conv1, blk.conv2):
                    if tuple(conv.weight.shape) != (x.c, x.c, 3, 3) or conv.stride[0] != 1 or conv.padding[0] != 1 \
                            or conv.bias is not None:
                        return False
            return x.cs == x.c and len(branch) > 0

        def key(x, has_res):
            return (x.n, x.h, x.w, x.c, x.c, x.c, x.c, 3, 3, 1, 1, has_res, False)
        nb = mod.num_branches
        for ia in reversed(range(nb)):          # (the coarsest pair first: what the measured table holds)
            for ib in reversed(range(nb)):
                if ia == ib or len(mod.branches[ia]) != len(mod.branches[ib]) or lowered[ia] or lowered[ib]:
                    continue
                if not (plain(mod.branches[ia], xs[ia]) and plain(mod.branches[ib], xs[ib])):
                    continue
                if all(tuner.pair_usable(key(xs[ia], res), key(xs[ib], res)) for res in (False, True)):
                    return ia, ib
        return None

    def _module(self, r, xs, mod, tag, region_open=False, keep_open=False, nxt=None):
        """``region_open``: the previous module left its fuse region open -- output i was
        produced on lane i, which is exactly what branch i of this module reads, so the
        branches continue on their lanes without a join/fork pair in between (lane 0 does
        not wait for the coarse lanes' fuse work).  ``keep_open``: leave this module's fuse
        region open for the next one, ``nxt`` (same stage, same branch count).  Returns (outs, open).
        A paired launch reads tensors of two branches: both chains are recorded on the lane of the lower branch, and
        where the next module pairs too and the region stays open, so are the two fuse outputs that feed them -- every
        tensor a pair reads was written on its own lane (stream order; ``_Recorder.happens_before`` sees it).  The
        other branches keep their lanes: lane 0 runs on into the next module without waiting for the coarse ones."""
        xs = list(xs)
        pair = self._pair_branches(r, xs, mod)
        # the resolution branches are independent (hrnet.py:286-287): one launch
        # lane each, so their kernels overlap each other's prologue / epilogue /
        # tail and the small coarse-branch grids do not leave the chip idle
        lanes = self.lanes and mod.num_branches > 1
        # point-to-point dependencies (EGONET_AMD_DEPS, default on): no join between the branches and the fuse rows.
        # Branch j signals behind its last block; on lane i the first op of term (i, j) waits for that signal alone, so
        # a term conv starts when ITS branch is done, not when the slowest one is, and fuse_i -- behind its row's term
        # convs in lane order -- has waited for all of them.  The paired launch (opt-in) and the training tape (its
        # recorder has no ``signal``) keep the join, and so do batches below ``deps_min_n`` crops: at 1 crop the graph
        # replay of the dependency recording measured slower than the joined one (profiles/deps_small_batch.txt).
        deps = lanes and self.deps and hasattr(r, 'signal') and mod.fuse_layers is not None and \
            xs[0].n >= self.deps_min_n and os.environ.get('EGONET_AMD_PAIR', tuner.PAIR_DEFAULT) == '0'
        sig, eta = {}, {}
        if lanes and not region_open:
            r.fork()
        for b, branch in enumerate(mod.branches):
            if pair is not None and b == max(pair):
                continue                # (recorded with its partner)
            if lanes:
                r.lane(b)
            if pair is not None and b == min(pair):
                ia, ib = pair
                for k, (ba, bb) in enumerate(zip(mod.branches[ia], mod.branches[ib])):
                    q = '%s.branches.%d+%d.%d' % (tag, ia, ib, k)
                    ha, hb = r.conv_pair(xs[ia], ba.conv1, ba.bn1, ACT_RELU, None,
                                         xs[ib], bb.conv1, bb.bn1, ACT_RELU, None, tag=q + '.conv1')
                    xs[ia], xs[ib] = r.conv_pair(ha, ba.conv2, ba.bn2, ACT_RELU, xs[ia],
                                                 hb, bb.conv2, bb.bn2, ACT_RELU, xs[ib], tag=q + '.conv2')
                continue
            first = len(r.ops) if deps else 0
            for k, blk in enumerate(branch):
                xs[b] = self._block(r, xs[b], blk, '%s.branches.%d.%d' % (tag, b, k))
            if deps:
                assert len(r.ops) > first, 'branch %d of %s recorded no op to signal behind' % (b, tag)
                sig[b] = r.signal()
                # when the lane is expected to be done: the tabled times of the branch's convs
                eta[b] = sum(tuner.tabled_ms(Program._conv_key(op)) for kind, op in r.ops[first:] if kind == 'conv')
        if lanes and not deps:
            r.join()
        if mod.fuse_layers is None:
            return xs, False
        outs = []
        stay = lanes and keep_open and self.chain_regions and len(mod.fuse_layers) == mod.num_branches
        pair_next = self._pair_branches(r, xs, nxt) if stay else None
        if lanes and not deps:          # the fuse outputs are independent too (hrnet.py:291-298)
            r.fork()
        # with dependencies a row records first the term whose source lane is expected to be done first (ties: by j);
        # fuse_kernel takes the terms in the reference's association order either way
        order = sorted(range(mod.num_branches), key=lambda j: (eta[j], j)) if deps else range(mod.num_branches)
        for i, row in enumerate(mod.fuse_layers):
            if lanes:
                r.lane(min(pair_next) if pair_next is not None and i in pair_next else i)
            terms = [None] * mod.num_branches
            for j in order:
                q = '%s.fuse_layers.%d.%d' % (tag, i, j)
                if deps and j != i:
                    r.wait(sig[j])
                if row[j] is None:
                    terms[j] = (xs[j], 0)
                elif j > i:
                    conv, bn = row[j][0], row[j][1]
                    t = r.conv(xs[j], conv.weight, None, bn, ACT_NONE, None, 1, 0, tag=q)
                    terms[j] = (t, j - i)
                else:
                    terms[j] = (self._unit_chain(r, xs[j], row[j], q), 0)
            outs.append(r.fuse(terms, True, tag='%s.fuse%d' % (tag, i)))
        if lanes and not stay:
            r.join()
        return outs, stay

    def _record(self, n, cin, h, w, decode_mode, r=None):
        """Walk the module tree once, issuing every layer to the recorder ``r``.
        The default recorder builds an inference program; egonet_amd.train_hrnet
        passes a tape that executes train-mode layers and records their backward."""
        m = self.model
        own = r is None
        if own:
            r = _Recorder()
            r.rules = active_rules(self.precision)     # (the training tape brings its own recorder: the switch is not its)
        x = r.nchw_to_nhwc(Ref(SLOT_USER0, 0), n, cin, h, w, tag='input')
        t = r.conv(x, m.conv1.weight, None, m.bn1, ACT_RELU, None, 2, 1, tag='conv1')
        t = r.conv(t, m.conv2.weight, None, m.bn2, ACT_RELU, None, 2, 1, tag='conv2')
        t = self._layer1(r, t, m.layer1)
        ys = [t]
        for idx in (1, 2, 3):
            trans = getattr(m, 'transition%d' % idx)
            xs = []
            for i, tr in enumerate(trans):
                if tr is None:
                    xs.append(ys[i])
                elif isinstance(tr[0], nn.Conv2d):      # conv, bn, relu
                    xs.append(r.conv(ys[-1], tr[0].weight, None, tr[1], ACT_RELU, None, 1, 1,
                                     tag='transition%d.%d' % (idx, i)))
                else:
                    xs.append(self._unit_chain(r, ys[-1], tr, 'transition%d.%d' % (idx, i)))
            stage = getattr(m, 'stage%d' % (idx + 1))
            open_ = False
            for k, mod in enumerate(stage):
                nxt = stage[k + 1] if k + 1 < len(stage) else None
                keep = nxt is not None and nxt.num_branches == mod.num_branches
                xs, open_ = self._module(r, xs, mod, 'stage%d.%d' % (idx + 1, k), region_open=open_, keep_open=keep,
                                         nxt=nxt if keep else None)
            ys = xs
        trunk = ys[0]
        J = m.num_joints
        mh, mw = trunk.h, trunk.w
        maps_ext = Ref(SLOT_USER0 + 1, 0)
        out_shapes = {'maps': (n, J, mh, mw)}
        if m.head_type == 'heatmap' and m.pixel_shuffle:
            # hrnet.py:373-383, 598-600: final_layer -> 1x1 conv + BN + ReLU -> PixelShuffle(up)
            fl, up = m.final_layer, m.upsample_layer
            t = r.conv(trunk, fl.weight, fl.bias, None, ACT_NONE, None, 1, fl.padding[0], tag='final_layer')
            f = int(m.upsamp_fact)
            u = r.conv(t, up[0].weight, up[0].bias, up[1], ACT_RELU, None, 1, 0, tag='upsample_layer.0')
            r.pixel_shuffle(u, J, f, maps_ext, tag='upsample_layer.3')
            mh, mw = mh * f, mw * f
            out_shapes['maps'] = (n, J, mh, mw)
            nslots = 2
        elif m.head_type == 'heatmap':
            fl = m.final_layer
            buf = Buf(n, mh, mw, J, cs=J, slot=SLOT_USER0 + 1, name='maps')
            r.conv(trunk, fl.weight, fl.bias, None, ACT_NONE, None, 1, fl.padding[0], dst=buf,
                   out_nchw=True, tag='final_layer')
            nslots = 2
        elif m.head_type == 'angleregression':
            # hrnet.py:384-422, 609-611: 1x1 conv (bias) -> 4 strided BasicBlocks -> AvgPool2d(4) ->
            # Linear + BatchNorm1d + ReLU -> Linear(256, 2).  The average pool and the first Linear
            # are ONE 4x4 valid convolution (filter = W[o][c] / 16 on every tap): the same sum.
            hd = m.head
            t = r.conv(trunk, hd[0].weight, hd[0].bias, None, ACT_NONE, None, 1, 0, tag='head.0')
            for k in range(1, 5):
                t = self._block(r, t, hd[k], 'head.%d' % k)
            pool = hd[5]
            ks = pool.kernel_size if isinstance(pool.kernel_size, int) else pool.kernel_size[0]
            if (t.h, t.w) != (ks, ks):
                raise ValueError('angle head expects a %dx%d map in front of AvgPool2d(%d), got %dx%d'
                                 % (ks, ks, ks, t.h, t.w))
            fc1, bn1, fc2 = m.final_fc[0], m.final_fc[1], m.final_fc[3]
            if hasattr(r, 'avgpool'):
                # the training tape: the layers as the module defines them (AvgPool2d, then the Linear layers as
                # parameters of their own -- their gradients belong to fc1.weight / fc2.weight, not to a derived filter)
                t = r.avgpool(t, ks, tag='head.5')
                y = r.conv(t, fc1.weight, fc1.bias, bn1, ACT_RELU, None, 1, 0, tag='final_fc.0')
                w2 = fc2.weight
            else:
                w1 = (fc1.weight.detach() / float(ks * ks)).view(fc1.out_features, fc1.in_features, 1, 1) \
                    .expand(-1, -1, ks, ks).contiguous()
                y = r.conv(t, w1, fc1.bias, bn1, ACT_RELU, None, 1, 0, tag='final_fc.0')
                w2 = fc2.weight.view(fc2.out_features, fc2.in_features, 1, 1)
            out = Buf(n, 1, 1, fc2.out_features, cs=fc2.out_features, slot=SLOT_USER0 + 1, name='angles')
            r.conv(y, w2, fc2.bias, None, ACT_NONE, None, 1, 0, dst=out, out_nchw=True, tag='final_fc.3')
            out_shapes = {'maps': (n, fc2.out_features)}          # the module returns [N, 2]
            nslots = 2
            decode_mode = None
        else:
            h1 = m.head1[0]
            aug = r.conv(trunk, h1.weight, h1.bias, None, ACT_NONE, None, 1, 0,
                         cout_cs=_round_up(J + 2, 4), tag='head1')
            r.ramps(aug, J, tag='coor_maps')
            r.nhwc_to_nchw(aug, J, maps_ext, tag='maps_nchw')
            aug.c = J + 2
            t = aug
            for k in range(4):
                t = self._block(r, t, m.head2[k], 'head2.%d' % k)
            fc = m.head2[4]
            if t.h != fc.kernel_size[0] or t.w != fc.kernel_size[1]:
                raise ValueError('coordinate head expects a %s map, got %dx%d'
                                 % (fc.kernel_size, t.h, t.w))
            cbuf = Buf(n, 1, 1, 2 * J, cs=2 * J, slot=SLOT_USER0 + 2, name='coords')
            r.conv(t, fc.weight, fc.bias, None, ACT_SIGMOID, None, 1, 0, dst=cbuf, out_nchw=True,
                   tag='head2.4')
            out_shapes['coords'] = (n, J, 2)
            nslots = 3
        if decode_mode is not None:
            r.decode(maps_ext, n, J, mh, mw, decode_mode, Ref(SLOT_USER0 + nslots, 0),
                     Ref(SLOT_USER0 + nslots + 1, 0), Ref(SLOT_USER0 + nslots + 2, 0), tag='decode')
            out_shapes['decode_slot'] = SLOT_USER0 + nslots
            nslots += 3
        if own:
            self.last_f16_ops = [op['tag'] for kind, op in r.ops if kind in _RULE_OF_KIND]
            if self.activations == 'f16':
                f16_storage(r)
        return r, nslots, out_shapes

    def program(self, x, decode_mode=None, slot=0):
        """``slot``: independent copies of the program (own arena, own launch lanes) for batches IN FLIGHT together: a
        serving loop that alternates two streams runs slot 0 on one and slot 1 on the other, and the low-occupancy head
        and tail of one batch overlap the other batch's kernels."""
        if self._stamp.changed():
            self.programs.clear()
        n, c, h, w = x.shape
        key = (x.device, n, c, h, w, decode_mode) if not slot else (x.device, n, c, h, w, decode_mode, slot)
        if self.precision != 'f32':
            key = key + (self.precision,)
        if self.activations != 'f32':
            key = key + ('a' + self.activations,)
        prog = self.programs.get(key)
        if prog is None:
            if h % 32 or w % 32:
                raise ValueError('HRNet input height/width must be multiples of 32, got %dx%d' % (h, w))
            rec, nslots, shapes = self._record(n, c, h, w, decode_mode)
            prog = Program(rec, x.device, nslots)
            prog.out_shapes = shapes
            self.programs[key] = prog
        return prog

    # -- execution ---------------------------------------------------------
    def forward(self, x, decode_mode=None, timed=False, slot=0):
        """x [N,C,H,W] fp32 CUDA.  Returns what the module's forward returns;
        with decode_mode 0/1 additionally (xy[N,K,2], maxvals[N,K,1], idx[N,K])."""
        if x.dtype != torch.float32:
            raise TypeError('egonet_amd HRNet engine computes in fp32, got %s' % x.dtype)
        x = x.contiguous()
        nmax = self.max_batch(x.shape[1], x.shape[2], x.shape[3])
        if x.shape[0] > nmax:
            return self._forward_chunked(x, decode_mode, timed, slot, nmax)
        with torch.cuda.device(x.device):
            prog = self.program(x, decode_mode, slot)
            if not timed and x.shape[0] <= self.graph_max_n and not torch.cuda.is_current_stream_capturing():
                return self._forward_graphed(prog, x, decode_mode)
            prog.captured = False             # (the bindings below replace the static ones of a captured graph)
            shp = prog.out_shapes
            maps = torch.empty(shp['maps'], dtype=torch.float32, device=x.device)
            prog.bind(SLOT_USER0, x)
            prog.bind(SLOT_USER0 + 1, maps)
            outs = maps
            if 'coords' in shp:
                coords = torch.empty(shp['coords'], dtype=torch.float32, device=x.device)
                prog.bind(SLOT_USER0 + 2, coords)
                outs = (maps, coords)
            dec = None
            if decode_mode is not None:
                n, k = shp['maps'][:2]
                xy = torch.empty(n, k, 2, dtype=torch.float32, device=x.device)
                mx = torch.empty(n, k, 1, dtype=torch.float32, device=x.device)
                idx = torch.empty(n, k, dtype=torch.int32, device=x.device)
                s = shp['decode_slot']
                prog.bind(s, xy)
                prog.bind(s + 1, mx)
                prog.bind(s + 2, idx)
                dec = (xy, mx, idx)
            if timed:
                self.last_ms = prog.run_timed()
            else:
                prog.run()
        return outs if dec is None else (outs, dec)


    # the batch sizes the shipped tile table covers (tuned/gfx950.json): chunks of an oversized batch are cut to these
    CHUNK_SIZES = (128, 64, 32, 16, 8, 4, 2, 1)

    def max_batch(self, c, h, w):
        """Largest batch ONE program takes: the kernels address a tensor with 32-bit byte offsets (buffer instructions;
        csrc/conv_plan.hip refuses a tensor of 2 GiB), and the widest tensor of the network is layer1's 256-channel map at
        a quarter of the resolution (hrnet.py:512-529) or the stem's 64 channels at half of it: 4 MiB per 256 x 256 crop,
        i.e. 511 crops.  The reference takes any loader batch (libs/trainer/trainer.py:113-125): larger batches are cut
        into chunks (_forward_chunked), not refused.  EGONET_AMD_MAX_TENSOR_BYTES lowers the limit (tests)."""
        import os
        limit = int(os.environ.get('EGONET_AMD_MAX_TENSOR_BYTES', str(2 ** 31 - 1)))
        per_crop = 4 * max(256 * (h // 4) * (w // 4), 64 * (h // 2) * (w // 2), c * h * w)
        return max(1, limit // per_crop)

    def _forward_chunked(self, x, decode_mode, timed, slot, nmax):
        """A batch whose widest tensor would reach 2 GiB: cut into the largest table-covered chunk sizes that fit (at
        256 x 256: 128 crops), run chunk by chunk on the same stream, results concatenated -- bit-identical to calling
        the chunks one by one (tests/test_gpu_models.py::test_oversized_batches_are_chunked)."""
        n = x.shape[0]
        sizes, left = [], n
        for c in self.CHUNK_SIZES:
            if c > nmax:
                continue
            while left >= c:
                sizes.append(c)
                left -= c
        outs, decs, ms, at = [], [], 0.0, 0
        for c in sizes:
            r = self.forward(x[at:at + c], decode_mode, timed, slot)
            at += c
            if timed:
                ms += self.last_ms
            if decode_mode is not None:
                r, d = r
                decs.append(d)
            outs.append(r)
        if timed:
            self.last_ms = ms
        if isinstance(outs[0], tuple):
            out = tuple(torch.cat([o[k] for o in outs]) for k in range(len(outs[0])))
        else:
            out = torch.cat(outs)
        if decode_mode is None:
            return out
        return out, tuple(torch.cat([d[k] for d in decs]) for k in range(3))

    def _forward_graphed(self, prog, x, decode_mode):
        """Opt-in (EGONET_AMD_GRAPH_MAX_N=<n>, default 0).  Small batches (BASELINE configs[4]'s per-GPU shard, configs[0]'s
        single crop) are launch-bound -- ~320 launches of 5-15 us each: from its third run on, a program is replayed as
        ONE hipGraph (``egn_program_capture``: the launch lanes become graph edges).  Measured on MI355X
        (profiles/r5_small_batch.txt): 16 crops 5.68 -> 4.89 ms, 4 crops 4.22 -> 3.80, one crop 3.79 -> 3.62, outputs
        bit-identical.  A captured graph holds addresses, so the program owns static input / output tensors: the
        caller's crops are copied in (12.6 MB at 16 crops) and the outputs copied out -- the results are fresh tensors
        as in the eager path.  tools/inference.py:135-199 (the reference's per-image forward) is this regime."""
        shp = prog.out_shapes
        st = getattr(prog, 'static', None)
        if st is None:
            dev = x.device
            st = dict(x=torch.empty_like(x), maps=torch.empty(shp['maps'], dtype=torch.float32, device=dev))
            if 'coords' in shp:
                st['coords'] = torch.empty(shp['coords'], dtype=torch.float32, device=dev)
            if decode_mode is not None:
                n, k = shp['maps'][:2]
                st['xy'] = torch.empty(n, k, 2, dtype=torch.float32, device=dev)
                st['mx'] = torch.empty(n, k, 1, dtype=torch.float32, device=dev)
                st['idx'] = torch.empty(n, k, dtype=torch.int32, device=dev)
            prog.static, prog.runs, prog.captured = st, 0, False
        prog.bind(SLOT_USER0, st['x'])            # (same address: a captured graph stays valid)
        prog.bind(SLOT_USER0 + 1, st['maps'])
        if 'coords' in st:
            prog.bind(SLOT_USER0 + 2, st['coords'])
        if decode_mode is not None:
            s = shp['decode_slot']
            prog.bind(s, st['xy'])
            prog.bind(s + 1, st['mx'])
            prog.bind(s + 2, st['idx'])
        # (a caller that alternates streams on ONE program: the static input may still be read by the previous run)
        cur = torch.cuda.current_stream(x.device)
        prev = getattr(prog, 'last_stream', None)
        if prev is not None and prev != cur:
            cur.wait_stream(prev)
        prog.last_stream = cur
        st['x'].copy_(x)
        if prog.captured:
            prog.replay()
        else:
            prog.run()
            prog.runs += 1
            if prog.runs >= 2:                    # (short-lived programs -- nn.DataParallel replicas -- never pay a capture)
                # captured on a stream of its own: the caller's current stream may be the legacy default stream, which
                # cannot be captured; the graph is then launched on whatever stream is current
                cur = torch.cuda.current_stream(x.device)
                cs = torch.cuda.Stream(device=x.device)
                cs.wait_stream(cur)
                with torch.cuda.stream(cs):
                    prog.capture()
                cur.wait_stream(cs)
                prog.captured = True
        outs = st['maps'].clone()
        if 'coords' in st:
            outs = (outs, st['coords'].clone())
        if decode_mode is None:
            return outs
        return outs, (st['xy'].clone(), st['mx'].clone(), st['idx'].clone())


# ---------------------------------------------------------------------------
# lifter
# ---------------------------------------------------------------------------
class LifterEngine(object):
    """Runs ``FCModel`` (eval mode) as six fused GEMM launches (Linear + folded
    BatchNorm1d + ReLU (+ residual)); a Linear is a 1x1 convolution on
    [N,1,1,C]."""

    def __init__(self, model):
        self.model = model
        self.programs = {}
        self._stamp = _Stamp(model)

    def _record(self, n, ld_in=None):
        m = self.model
        act = ACT_LEAKY if m.leaky else ACT_RELU
        r = _Recorder()
        cin = m.w1.in_features
        if ld_in is None:
            x = r.nchw_to_nhwc(Ref(SLOT_USER0, 0), n, cin, 1, 1, tag='input')
        else:                      # caller provides [n, ld_in] rows already padded
            x = Buf(n, 1, 1, cin, cs=ld_in, slot=SLOT_USER0, name='input')

        def lin(t, fc, bn, a, res, tag, dst=None, nchw=False):
            return r.conv(t, fc.weight.view(fc.out_features, fc.in_features, 1, 1), fc.bias, bn, a,
                          res, 1, 0, dst=dst, out_nchw=nchw, tag=tag)

        y = lin(x, m.w1, m.batch_norm1, act, None, 'w1')
        for b, blk in enumerate(m.res_blocks):
            z = lin(y, blk.w1, blk.batch_norm1, act, None, 'res%d.w1' % b)
            y = lin(z, blk.w2, blk.batch_norm2, act | ACT_RES_AFTER, y, 'res%d.w2' % b)
        out = Buf(n, 1, 1, m.w2.out_features, cs=m.w2.out_features, slot=SLOT_USER0 + 1, name='out')
        lin(y, m.w2, None, ACT_NONE, None, 'w2', dst=out, nchw=True)
        return r

    def program(self, device, n, ld_in=None, slot=0):
        if self._stamp.changed():
            self.programs.clear()
        key = (device, n, ld_in) if not slot else (device, n, ld_in, slot)
        prog = self.programs.get(key)
        if prog is None:
            prog = Program(self._record(n, ld_in), device, 2)
            self.programs[key] = prog
        return prog

    def forward(self, x, ld_in=None, slot=0):
        """x [N,in] fp32 CUDA (or [N,ld_in] zero-padded rows) -> [N,out]."""
        if x.dtype != torch.float32:
            raise TypeError('egonet_amd lifter engine computes in fp32, got %s' % x.dtype)
        x = x.contiguous()
        n = x.shape[0]
        out = torch.empty(n, self.model.w2.out_features, dtype=torch.float32, device=x.device)
        if n == 0:
            return out
        with torch.cuda.device(x.device):
            prog = self.program(x.device, n, ld_in, slot)
            prog.bind(SLOT_USER0, x)
            prog.bind(SLOT_USER0 + 1, out)
            prog.run()
        return out
