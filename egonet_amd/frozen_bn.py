"""Frozen layers on the native HRNet tape (``train_hrnet._Tape``): which buffers need a gradient, BatchNorm in eval
mode inside a model that trains, and the launches a backward is expected to make.

Reference: ``nn.BatchNorm2d.forward`` with ``training == False`` (the frozen-BN fine-tune: ``model.train();
model.layer1.eval()`` under libs/trainer/trainer.py:183-209) normalises with ``running_mean`` / ``running_var``, writes
neither and leaves ``num_batches_tracked`` alone; ``freeze_layers`` (hrnet.py:675-690) sets ``requires_grad = False``.

The rule for "needs a gradient" (DESIGN.md section 3.22): a tape buffer needs one if the op that produced it has a
trainable parameter (conv weight, bias, BatchNorm gamma / beta) or any of its inputs needs one; the input images never
do.  An op whose output needs none registers no backward closure and keeps nothing for one.

The form a BatchNorm layer takes on the tape, per layer (``bn_form``):
  BATCH   train mode: batch statistics, running-statistics update, the two-reduction backward -- today's launches;
  FUSED   eval mode, gamma and beta frozen: the conv with the folded scale / shift (+ residual + ReLU) in its epilogue is
          the whole forward; backward = egn_bn_frozen_bwd_f32, one pass, no reduction;
  AFFINE  eval mode, gamma or beta trainable: raw conv -> egn_bn_act_fwd_f32 with mean = running_mean and the folded
          1/sigma; backward = egn_bn_bwd_sums_f32 (dbeta, dgamma) + egn_bn_bwd_dz_f32 with ZERO sum vectors, which is
          gamma * istd * dpre, the derivative with constant statistics.
"""
import os

import torch

from . import _lib
from .engine import Buf, _round_up

BATCH, FUSED, AFFINE = 'batch', 'fused', 'affine'


def prune_enabled():
    """EGONET_AMD_PRUNE_BACKWARD=0: every op registers its backward as before (A/B runs, the bit-equality test)."""
    return os.environ.get('EGONET_AMD_PRUNE_BACKWARD', '1') != '0'


def trainable(*params):
    return any(p is not None and p.requires_grad for p in params)


def bn_form(bn):
    if bn.training:
        return BATCH
    if not bn.track_running_stats or bn.running_mean is None or bn.running_var is None:
        raise NotImplementedError('BatchNorm in eval mode without running statistics (track_running_stats=False) on '
                                  'the native tape: it would normalise with batch statistics it must not track')
    return AFFINE if trainable(bn.weight, bn.bias) else FUSED


def op_needs_grad(no_grad, inputs, *params):
    """THE rule: the op has a trainable parameter, or one of its input Bufs needs a gradient."""
    return trainable(*params) or any(b is not None and id(b) not in no_grad for b in inputs)


def bn_modules_under(model, prefixes):
    """The BatchNorm modules whose qualified name starts with one of ``prefixes`` (``is_freezed``'s rule)."""
    return [m for name, m in model.named_modules()
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and any(name.startswith(p) for p in prefixes)]


class FoldTable(object):
    """scale / shift vectors of the eval-mode BatchNorm layers of a model, folded on the device: from the second step
    on ONE launch at the start of the step (``egn_bn_fold_batch_f32`` over a device descriptor table, rebuilt when a
    pointer moved -- like ``PackedFilters`` / ``StepCounters``); the first step folds layer by layer while it discovers
    them.  Every step folds again: a trainable conv bias in front of a frozen BatchNorm changes the shift."""

    _DESC = [('gamma', '<u8'), ('beta', '<u8'), ('mean', '<u8'), ('var', '<u8'), ('bias', '<u8'), ('scale', '<u8'),
             ('shift', '<u8'), ('eps', '<f8'), ('cout', '<i4'), ('coutp', '<i4')]

    def __init__(self, device):
        self.dev = device
        self.L = _lib.lib()
        self.entries = {}          # (id(bn), form) -> (bn, bias, scale, shift | None)
        self.table = None
        self.ptrs = None
        self.keep = []             # one-layer tables of the first step: alive until its finalize

    @staticmethod
    def _row(bn, bias, form, scale, shift):
        fused = form == FUSED
        return (bn.weight.data_ptr() if fused else 0, bn.bias.data_ptr() if fused else 0, bn.running_mean.data_ptr(),
                bn.running_var.data_ptr(), bias.data_ptr() if (fused and bias is not None) else 0, scale.data_ptr(),
                shift.data_ptr() if fused else 0, float(bn.eps), bn.num_features, scale.numel())

    def _rows(self):
        return [self._row(bn, bias, form, sc, sh) for (_, form), (bn, bias, sc, sh) in self.entries.items()]

    def _upload(self, rows):
        import numpy as np
        desc = np.zeros(len(rows), dtype=np.dtype(self._DESC, align=True))
        assert desc.dtype.itemsize == self.L.egn_bn_fold_desc_bytes(), (desc.dtype.itemsize,
                                                                        self.L.egn_bn_fold_desc_bytes())
        for i, r in enumerate(rows):
            desc[i] = r
        return torch.from_numpy(desc.view(np.uint8)).to(self.dev)

    def get(self, bn, bias, form, stream):
        """(scale, shift) of a FUSED layer, (1/sigma, None) of an AFFINE one: zero-padded [CoutP] device vectors."""
        key = (id(bn), form)
        ent = self.entries.get(key)
        if ent is not None and ent[1] is not bias:
            ent = None
        if ent is not None and self.table is not None:
            return ent[2], ent[3]
        if ent is None:
            coutp = _round_up(bn.num_features, 16)
            scale = torch.zeros(coutp, dtype=torch.float32, device=self.dev)
            shift = torch.zeros(coutp, dtype=torch.float32, device=self.dev) if form == FUSED else None
            ent = self.entries[key] = (bn, bias, scale, shift)
            self.table = None
        one = self._upload([self._row(bn, bias, form, ent[2], ent[3])])
        _lib.check(self.L.egn_bn_fold_batch_f32(_lib.ptr(one), 1, stream), 'bn fold')
        self.keep.append(one)
        return ent[2], ent[3]

    def finalize(self):
        self.keep = []
        if self.table is not None or not self.entries:
            return
        rows = self._rows()
        self.table = self._upload(rows)
        self.ptrs = rows

    def fold_all(self, stream):
        """One launch for every layer seen so far; False before the table exists or after a pointer moved."""
        if self.table is None:
            return False
        if self._rows() != self.ptrs:
            self.table = None
            return False
        _lib.check(self.L.egn_bn_fold_batch_f32(_lib.ptr(self.table), len(self.ptrs), stream), 'bn fold')
        return True


def frozen_bwd(L, dy, y, scale, relu, dz, dres, rows, cols, ld, stream):
    _lib.check(L.egn_bn_frozen_bwd_f32(_lib.ptr(dy), _lib.ptr(y) if relu else None, _lib.ptr(scale), relu, _lib.ptr(dz),
                                       _lib.ptr(dres), rows, cols, ld, stream), 'bn_frozen_bwd')


def new_counts():
    return {'dgrad': 0, 'wgrad': 0, 'bn_bwd': 0}


class PlanTape(object):
    """The recorder interface of the training tape WITHOUT a device: walks the model as ``_Tape`` does, applies the same
    rule and counts what the backward of a step whose every output receives a gradient launches
    (``planned_backward_launches``).  Needs no GPU and no library."""

    def __init__(self, prune):
        self.prune = prune
        self.no_grad = set()
        self.keep = []
        self.counts = new_counts()
        self.bns = []

    def fork(self):
        pass

    join = fork

    def lane(self, k):
        pass

    def new(self, n, h, w, c, cs=None, name=''):
        b = Buf(n, h, w, c, cs=cs, name=name)
        self.keep.append(b)
        return b

    def nchw_to_nhwc(self, x_ext, n, c, h, w, tag=''):
        y = self.new(n, h, w, c, name=tag)
        self.no_grad.add(id(y))
        return y

    def nhwc_to_nchw(self, x, c, dst_ext, tag=''):
        pass

    def pixel_shuffle(self, x, c, up, dst_ext, tag=''):
        pass

    def ramps(self, y, c0, tag=''):
        pass

    def _dead(self, y, inputs, *params):
        if self.prune and not op_needs_grad(self.no_grad, inputs, *params):
            self.no_grad.add(id(y))
            return True
        return False

    def avgpool(self, x, k, tag=''):
        y = self.new(x.n, x.h // k, x.w // k, x.c, cs=x.cs, name=tag)
        self._dead(y, (x,))
        return y

    def fuse(self, terms, relu, tag=''):
        base = [t for t, s in terms if s == 0][0]
        y = self.new(base.n, base.h, base.w, base.c, cs=base.cs, name=tag)
        self._dead(y, [t for t, _ in terms])
        return y

    def conv(self, x, weight, bias=None, bn=None, act=0, res=None, stride=1, pad=0, dst=None, out_nchw=False,
             cout_cs=None, tag=''):
        if weight.dim() == 2:
            cout, kh, kw = weight.shape[0], 1, 1
        else:
            cout, _, kh, kw = weight.shape
        ho = (x.h + 2 * pad - kh) // stride + 1
        wo = (x.w + 2 * pad - kw) // stride + 1
        y = self.new(x.n, ho, wo, cout, cs=cout_cs, name=tag)
        form = None if bn is None else bn_form(bn)
        if form == BATCH:
            self.bns.append(bn)
        if self._dead(y, (x, res), weight, bias, *(() if bn is None else (bn.weight, bn.bias))):
            return y
        if bn is not None:
            self.counts['bn_bwd'] += 1 if form == FUSED else 2
        if weight.requires_grad:
            self.counts['wgrad'] += 1
        if id(x) not in self.no_grad:
            self.counts['dgrad'] += 1
        return y


def planned_backward_launches(model, h, w, n=2, prune=None):
    """``last_backward_launches`` of a native step (or bridge backward) of ``model`` on [n, C, h, w] crops in which every
    output receives a gradient, from the model alone (no GPU): {'dgrad': data-gradient convolutions, 'wgrad':
    weight-gradient launches, 'bn_bwd': BatchNorm backward entry-point calls (2 per layer on the reduction forms, 1 per
    fused frozen layer)}."""
    from .engine import HRNetEngine
    tape = PlanTape(prune_enabled() if prune is None else prune)
    HRNetEngine(model)._record(n, model.conv1.weight.shape[1], h, w, None, r=tape)
    return tape.counts
