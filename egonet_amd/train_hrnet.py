"""Native training step of the HRNet heat-map / coordinate model on MI355X
(BASELINE config 4).

Reference hot loop, ``libs/trainer/trainer.py:183-209``::

    optim.zero_grad(); prediction = model(data); loss = loss_func(prediction, target, weights, meta)
    loss.backward(); optim.step()

with ``model`` = PoseHighResolutionNet in train mode (BatchNorm on batch
statistics), ``loss_func`` = JointsCompositeLoss(['mse','l1',None], weights
1.0 / 0.1) (libs/loss/function.py:61-202, KITTI_train_IGRs.yml:86-89) and
Adam(lr 1e-3) (libs/optimizer/optimizer.py:8-40).

``HRNetTrainStep.step`` runs all of that as HIP launches through the C ABI;
torch autograd / MIOpen are not involved:

* forward: the SAME module walk the inference engine records
  (``engine.HRNetEngine._record``) is issued to a tape that executes each layer
  in train mode -- raw conv on the fp32-MFMA kernel (weights packed on the
  device every step), batch statistics + running-stat update, fused
  BatchNorm(+residual)+ReLU -- and remembers what its backward needs;
* backward: the tape is replayed in reverse: fused BatchNorm/ReLU backward
  (two-pass column reductions), weight gradients on the split-K MFMA kernel
  (csrc/conv_wgrad.hip), data gradients on the forward conv kernel with the
  180-degree-rotated, channel-swapped filter (stride 2: over the zero-inserted
  gradient), multi-resolution fuse backward (gated block sums);
* loss: 0.5 * MSE over the maps + 0.1 * L1 over the coordinates, gradients
  written by the loss kernels;
* Adam: ONE launch over the flat parameter buffer (``FlatParams``): parameters,
  gradients and both moments each live in one contiguous allocation, the
  module's ``nn.Parameter``s are views of it (state_dict / HC.pth unchanged).
  The flat gradient is also what a data-parallel job all-reduces (one RCCL
  call per bucket, ``egonet_amd.parallel``).
"""
import collections
import ctypes as C
import os

import torch

from . import _lib, filters, frozen_bn, optim, train_state, tuner
from .engine import invalidate
from ._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID
from .engine import Buf, HRNetEngine, _round_up
from .train_common import (FlatParams, PackedFilters, StepCounters, _gc_paused, begin_grad_sync, finish_step,
                           fork_wgrad, join_wgrad, timing_begin, timing_end, wgrad_side_stream)


class _Tape(object):
    """Recorder interface of ``engine._Recorder`` that EXECUTES train-mode layers."""

    def __init__(self, owner, images):
        self.o = owner
        self.L = owner.L
        self.dev = images.device
        self.images = images
        self.st = _lib.current_stream(self.dev)
        self.data = {}            # id(Buf) -> 1-D fp32 tensor
        self.grad = {}            # id(Buf) -> [tensor, owned]
        self.keep = []            # Bufs (ids stay unique while the tape lives)
        self.side = owner.wgrad_stream      # weight gradients run here, beside the backward chain
        self.side_st = None if self.side is None else C.c_void_p(self.side.cuda_stream)
        self.side_keep = []       # tensors the side stream reads: alive until it is joined
        self.back = []            # backward closures, forward order
        self.named = {}           # tag -> Buf
        self.user = {}            # tag -> NCHW copy for the caller
        self.no_grad = set()      # ids of Bufs that need no gradient: the input, and (pruning) what frozen_bn's rule finds
        self.prune = owner.prune_backward
        self.counts = frozen_bn.new_counts()      # backward launches issued: the owner's last_backward_launches
        self.bns = []             # BatchNorm layers in train mode: their num_batches_tracked moves
        self.maps_user = None

    # -- recorder plumbing (concurrency hints are ignored: one stream) ------
    def fork(self):
        pass

    def join(self):
        pass

    def lane(self, k):
        pass

    def decode(self, *a, **k):
        raise NotImplementedError('decode is not part of the training step')

    def _empty(self, numel):
        return torch.empty(numel, dtype=torch.float32, device=self.dev)

    def new(self, n, h, w, c, cs=None, name=''):
        b = Buf(n, h, w, c, cs=cs, name=name)
        self.keep.append(b)
        self.data[id(b)] = self._empty(n * h * w * b.cs)
        return b

    def _accum(self, buf, g, owned=True):
        if id(buf) in self.no_grad:
            return
        cur = self.grad.get(id(buf))
        if cur is None:
            self.grad[id(buf)] = [g, owned]
            return
        if not cur[1]:                              # shared tensor: do not add in place
            out = self._empty(g.numel())
            _lib.check(self.L.egn_add_f32(_lib.ptr(cur[0]), _lib.ptr(g), _lib.ptr(out), g.numel(), self.st), 'add')
            self.grad[id(buf)] = [out, True]
        else:
            _lib.check(self.L.egn_add_f32(_lib.ptr(cur[0]), _lib.ptr(g), _lib.ptr(cur[0]), g.numel(), self.st), 'add')

    def _take_grad(self, buf):
        cur = self.grad.pop(id(buf), None)
        return None if cur is None else cur[0]

    # -- launches -----------------------------------------------------------
    def _conv_launch(self, x, wp, shift, y, n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, act,
                     weight=None, dgrad=0, want_stats=False, res=None, f43_ok=True, scale=None):
        """``wp``: the direct-packed filter (None: packed here from ``weight``).  With ``weight`` (+ ``dgrad``) given, the tuner may pick a
        Winograd configuration for 3x3 stride-1 layers (forward and data gradient alike: the data
        gradient is a stride-1 convolution with the rotated filter); the transformed filter then comes
        from the step's PackedFilters like the direct one.  ``scale``: the folded BatchNorm scale of a frozen layer (with its
        ``shift``, ``res`` and ``act`` the inference epilogue); None: ones, a raw convolution."""
        key = (n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, scale is not None and res is not None, False)
        if scale is None:
            scale = self.o.ones
        can_wino = weight is not None and act in (ACT_NONE, ACT_RELU) and self.o.allow_wino
        # [round 5] F(4x4,3x3) (csrc/conv_wino4.hip, filter kind 3) in the tape: the filter is transformed on the device
        # with all the others (PackedFilters), BatchNorm statistics come from conv_wino4s_kernel's item end, the K-split
        # configurations get the owner's ticket words (one stream: launches that share them are ordered)
        can_f43 = can_wino and f43_ok and self.o.allow_f43 in (('all',) if dgrad else ('all', 'fwd'))
        kinds = tuner.TAPE_F43 if can_f43 else tuner.TAPE_WINO if can_wino else tuner.DIRECT
        cfg = tuner.choose(self.dev, key, kinds, ticket_cap=self.o.tickets.numel(),
                           inplace_res=res is not None and res.data_ptr() == y.data_ptr())
        kind = tuner.kind_of(cfg)
        if wp is None or kind != filters.DIRECT:
            wp = self.o.packs.get(weight, dgrad, self.st, kind)
        stats = None
        if want_stats and self.o.fuse_bn_stats and cfg > 0:
            # BatchNorm batch statistics in the conv epilogue (per-tile partial sums, csrc/conv_wino.hip):
            # saves the separate reduction pass over z where the tile configuration supports it
            nrows = self.L.egn_conv2d_bnstats_rows(n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, cfg)
            if nrows > 0:
                stats = (torch.empty(nrows * 2 * cout, dtype=torch.float64, device=self.dev), nrows)
        e0 = timing_begin(self.o.timing, self.dev)     # bench.py: hipEvents around every forward / data-gradient conv
        if kind == filters.WINO4:
            _lib.check(self.L.egn_conv2d_ex_f32(_lib.ptr(x), _lib.ptr(wp), _lib.ptr(scale), _lib.ptr(shift),
                                                _lib.ptr(res), _lib.ptr(y), n, h, w, cin, cs_in, cout, cs_out, kh, kw,
                                                stride, pad, act, cfg, None if stats is None else _lib.ptr(stats[0]),
                                                0 if stats is None else stats[1],
                                                _lib.ptr(self.o.tickets) if tuner.ticket_words(key, cfg) > 0 else None,
                                                self.o.tickets.numel(), self.st), 'conv (F(4x4,3x3))')
        elif stats is not None:
            _lib.check(self.L.egn_conv2d_bnstats_f32(_lib.ptr(x), _lib.ptr(wp), _lib.ptr(self.o.ones), _lib.ptr(shift),
                                                     _lib.ptr(y), n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride,
                                                     pad, cfg, _lib.ptr(stats[0]), stats[1], self.st), 'conv+stats')
        else:
            _lib.check(self.L.egn_conv2d_f32(_lib.ptr(x), _lib.ptr(wp), _lib.ptr(scale), _lib.ptr(shift),
                                             _lib.ptr(res), _lib.ptr(y), n, h, w, cin, cs_in, cout, cs_out, kh, kw,
                                             stride, pad, act, 0, cfg, self.st), 'conv')
        if e0 is not None:
            ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
            timing_end(self.o.timing, self.dev, e0, cfg, 2.0 * n * ho * wo * cout * cin * kh * kw,
                       stats is not None and kind == filters.WINO4)
        return stats

    def _wgrad(self, x, xd, dy, cs_out, weight, stride, pad):
        cout, cin, kh, kw = weight.shape
        L = self.L
        need = L.egn_conv2d_wgrad_ws_bytes(x.n, x.h, x.w, cin, x.cs, cout, cs_out, kh, kw, stride, pad)
        if need < 0:
            raise NotImplementedError('weight gradient of a %dx%d convolution' % (kh, kw))
        ws = self.o.wgrad_ws(need)
        self.counts['wgrad'] += 1
        st = self.st
        if self.side is not None:
            fork_wgrad(self.side, self.dev, self.side_keep, (xd, dy))
            st = self.side_st
        _lib.check(L.egn_conv2d_wgrad_f32(_lib.ptr(xd), _lib.ptr(dy), _lib.ptr(self.o.grad_of(self.o.param_of(weight))),
                                          x.n, x.h, x.w, cin, x.cs,
                                          cout, cs_out, kh, kw, stride, pad, _lib.ptr(ws), ws.numel() * 4, st),
                   'wgrad')

    def release(self):
        """Break the tape <-> backward-closure reference cycles so that every tensor of the iteration is
        freed by reference counting when the step returns (left to the cyclic garbage collector they
        linger for a few iterations, the caching allocator has to hipMalloc fresh blocks meanwhile and
        single steps take 2x as long)."""
        self.back = []
        self.data = {}
        self.grad = {}
        self.keep = []
        self.named = {}
        self.side_keep = []

    def join_side(self):
        join_wgrad(self.side, self.dev, self.side_keep)

    def _accum_dgrad(self, x, dy, ho, wo, cs_out, weight, stride, pad):
        """grad(x) += data gradient of the conv.  Where x already has a gradient tensor of its own (the
        residual path of a block reaches x first) the conv adds it in its epilogue and writes in place
        (every element is read and written by the same lane) instead of a separate add pass."""
        if id(x) in self.no_grad:
            return
        cur = self.grad.get(id(x))
        into = cur[0] if (cur is not None and cur[1] and weight.shape[2] == weight.shape[3] and self.o.fuse_grad_add) else None
        g = self._dgrad(dy, ho, wo, cs_out, weight, stride, pad, x, into=into)
        if into is None:
            self._accum(x, g)

    def _dgrad(self, dy, ho, wo, cs_out, weight, stride, pad, x, into=None):
        cout, cin, kh, kw = weight.shape
        L = self.L
        self.counts['dgrad'] += 1
        if kh != kw:
            # the Pedestrian model's final 4x3 'valid' conv over the whole 4x3 map (hrnet.py:457-460):
            # one output pixel, so dx[n, (ky,kx), ci] = sum_co dy[n, co] * W[co, ci, ky, kx] is a GEMM
            # whose output rows are the NHWC map itself
            if not (pad == 0 and stride == 1 and x.h == kh and x.w == kw and ho == 1 and wo == 1):
                raise NotImplementedError('data gradient of a non-square %dx%d convolution that does not '
                                          'cover its whole input' % (kh, kw))
            wt = torch.zeros(kh * kw, x.cs, cout, dtype=torch.float32, device=self.dev)
            wt[:, :cin] = weight.detach().permute(2, 3, 1, 0).reshape(kh * kw, cin, cout)
            wt = wt.view(kh * kw * x.cs, cout, 1, 1)
            rows = kh * kw * x.cs
            wq = torch.empty(L.egn_packed_weight_floats(rows, cout, 1, 1, 0), dtype=torch.float32, device=self.dev)
            _lib.check(L.egn_pack_conv_weight_f32(_lib.ptr(wt), rows, cout, 1, 1, 0, _lib.ptr(wq), self.st), 'pack')
            dx = self._empty(x.n * rows)
            shift = self.o.zeros if self.o.zeros.numel() >= rows + 16 else torch.zeros(rows + 16, device=self.dev)
            ones = self.o.ones if self.o.ones.numel() >= rows + 16 else torch.ones(rows + 16, device=self.dev)
            cfg = tuner.choose(self.dev, (x.n, 1, 1, cout, cs_out, rows, rows, 1, 1, 1, 0, False, False))
            _lib.check(L.egn_conv2d_f32(_lib.ptr(dy), _lib.ptr(wq), _lib.ptr(ones), _lib.ptr(shift), None, _lib.ptr(dx),
                                        x.n, 1, 1, cout, cs_out, rows, rows, 1, 1, 1, 0, ACT_NONE, 0, cfg, self.st),
                       'conv')
            return dx
        if stride == 2:
            up = self._empty(x.n * x.h * x.w * cs_out)
            _lib.check(L.egn_zero_insert2_f32(_lib.ptr(dy), _lib.ptr(up), x.n, ho, wo, x.h, x.w, cs_out, self.st),
                       'zero_insert')
            src, sh, sw = up, x.h, x.w
        elif stride == 1:
            src, sh, sw = dy, ho, wo
        else:
            raise NotImplementedError('stride %d' % stride)
        # a stride-2 conv's data gradient is a stride-1 conv over the zero-inserted dy: Winograd applies too
        dx = into if into is not None else self._empty(x.n * x.h * x.w * x.cs)
        # (F(4x4,3x3) only for the stride-1 layers: over a zero-inserted gradient its per-launch error measured
        # 2.0-2.5e-5 of the largest element at 32 crops -- above the 2e-5 the float64 launch checks allow -- against
        # <= 1.4e-5 on the stride-1 layers; tests/test_gpu_bench_size.py, profiles/r5_train32_dgrad_errors.txt)
        self._conv_launch(src, None, self.o.zeros, dx, x.n, sh, sw, cout, cs_out, cin, x.cs, kh, kw, 1, kh - 1 - pad,
                          ACT_NONE, weight=weight, dgrad=1, res=into, f43_ok=(stride == 1))
        return dx

    def _dead(self, y, inputs, *params):
        """Pruning: the output ``y`` of an op without a trainable parameter among ``params`` and without an input that
        needs a gradient needs none either (frozen_bn.op_needs_grad) -- the caller registers no backward for it."""
        if self.prune and not frozen_bn.op_needs_grad(self.no_grad, inputs, *params):
            self.no_grad.add(id(y))
            return True
        return False

    # -- ops (engine._Recorder interface) -----------------------------------
    def nchw_to_nhwc(self, x_ext, n, c, h, w, tag=''):
        y = self.new(n, h, w, c, name=tag)
        _lib.check(self.L.egn_nchw_to_nhwc_f32(_lib.ptr(self.images), _lib.ptr(self.data[id(y)]), n, c, h, w, y.cs,
                                               self.st), 'to_nhwc')
        self.no_grad.add(id(y))
        return y

    def nhwc_to_nchw(self, x, c, dst_ext, tag=''):
        self.maps_user = torch.empty(x.n, c, x.h, x.w, dtype=torch.float32, device=self.dev)
        _lib.check(self.L.egn_nhwc_to_nchw_f32(_lib.ptr(self.data[id(x)]), _lib.ptr(self.maps_user), x.n, c, x.h, x.w,
                                               x.cs, self.st), 'to_nchw')

    def pixel_shuffle(self, x, c, up, dst_ext, tag=''):
        """nn.PixelShuffle(up) of the heat-map upsampler (hrnet.py:373-383, 598-600) into an NCHW user tensor
        (``user[tag]``); ``named[tag]`` is the pre-shuffle Buf, where the gradient of the maps arrives (the step's
        fused loss, egn_pixshuf_loss_f32, or the autograd bridge's unshuffle writes it there)."""
        u = torch.empty(x.n, c, x.h * up, x.w * up, dtype=torch.float32, device=self.dev)
        _lib.check(self.L.egn_pixel_shuffle_nhwc_to_nchw_f32(_lib.ptr(self.data[id(x)]), _lib.ptr(u), x.n, c, x.h, x.w,
                                                             x.cs, up, self.st), 'pixel_shuffle')
        self.user[tag] = u
        self.named[tag] = x

    def avgpool(self, x, k, tag=''):
        """AvgPool2d(k) (the angle head's, hrnet.py:384-422) on csrc/heads.hip."""
        L = self.L
        y = self.new(x.n, x.h // k, x.w // k, x.c, cs=x.cs, name=tag)
        xd, yd = self.data[id(x)], self.data[id(y)]
        _lib.check(L.egn_avgpool_fwd_f32(_lib.ptr(xd), _lib.ptr(yd), x.n, x.h, x.w, x.cs, k, self.st), 'avgpool')
        self.named[tag] = y
        if self._dead(y, (x,)):
            return y

        def backward():
            dy = self._take_grad(y)
            if dy is None or id(x) in self.no_grad:
                return
            dx = self._empty(xd.numel())
            _lib.check(L.egn_avgpool_bwd_f32(_lib.ptr(dy), _lib.ptr(dx), x.n, x.h, x.w, x.cs, k, 0, self.st),
                       'avgpool_bwd')
            self._accum(x, dx)
        self.back.append(backward)
        return y

    def ramps(self, y, c0, tag=''):
        _lib.check(self.L.egn_fill_coord_ramps_f32(_lib.ptr(self.data[id(y)]), y.n, y.h, y.w, y.cs, c0, self.st),
                   'ramps')

    def conv(self, x, weight, bias=None, bn=None, act=ACT_NONE, res=None, stride=1, pad=0,
             dst=None, out_nchw=False, cout_cs=None, tag=''):
        L = self.L
        param = weight
        if weight.dim() == 2:            # nn.Linear (the angle head's final_fc): a 1x1 convolution on a 1x1 map
            weight = self.o.linear4(weight)
        cout, cin, kh, kw = weight.shape
        assert cin == x.c, (cin, x.c, tag)
        ho = (x.h + 2 * pad - kh) // stride + 1
        wo = (x.w + 2 * pad - kw) // stride + 1
        # user-facing outputs (dst / out_nchw of the inference recording) are computed
        # into an internal NHWC tensor like every other layer -- the backward needs the
        # padded layout -- and copied out in the caller's NCHW format afterwards
        xd = self.data[id(x)]
        wp = None                        # packed by _conv_launch in the layout its tile configuration reads
        rows = x.n * ho * wo
        form = None if bn is None else frozen_bn.bn_form(bn)
        if form == frozen_bn.FUSED:
            return self._conv_frozen(x, xd, param, weight, bias, bn, act, res, stride, pad, ho, wo, cout_cs, tag)
        z = self.new(x.n, ho, wo, cout, cs=cout_cs, name=tag)
        zd = self.data[id(z)]
        if bn is None:
            shift = self.o.zeros
            if bias is not None:
                shift = torch.zeros(_round_up(cout, 16), dtype=torch.float32, device=self.dev)
                shift[:cout].copy_(bias.detach())
            self._conv_launch(xd, wp, shift, zd, x.n, x.h, x.w, cin, x.cs, cout, z.cs, kh, kw, stride, pad, act,
                              weight=weight)
            if dst is not None or out_nchw:
                u = torch.empty(x.n, cout, ho, wo, dtype=torch.float32, device=self.dev)
                _lib.check(L.egn_nhwc_to_nchw_f32(_lib.ptr(zd), _lib.ptr(u), x.n, cout, ho, wo, z.cs, self.st), 'to_nchw')
                self.user[tag] = u
            self.named[tag] = z
            if self._dead(z, (x,), param, bias):
                return z

            def backward():
                dy = self._take_grad(z)
                if dy is None:
                    return
                if act == ACT_SIGMOID:
                    dz = self._empty(dy.numel())
                    _lib.check(L.egn_sigmoid_bwd_f32(_lib.ptr(dy), _lib.ptr(zd), _lib.ptr(dz), dy.numel(), self.st),
                               'sigmoid_bwd')
                    dy = dz
                elif act != ACT_NONE:
                    raise NotImplementedError('activation %d without BatchNorm' % act)
                if bias is not None and bias.requires_grad:
                    _lib.check(L.egn_colsum_f32(_lib.ptr(dy), rows, cout, z.cs, _lib.ptr(self.o.grad_of(bias)),
                                                _lib.ptr(self.o.col_ws), self.st), 'bias grad')
                if param.requires_grad:
                    self._wgrad(x, xd, dy, z.cs, weight, stride, pad)
                self._accum_dgrad(x, dy, ho, wo, z.cs, weight, stride, pad)
            backward.params = [param] + ([bias] if bias is not None else [])     # gradients final after it
            self.back.append(backward)
            return z

        shift = self.o.zeros
        if bias is not None:
            # a bias in front of BatchNorm (the pixel-shuffle upsampler's 1x1 conv, the angle head's first Linear):
            # it goes into the conv epilogue, so the batch statistics -- and running_mean -- include it like the
            # reference's; the statistics then come from the separate reduction over z
            shift = torch.zeros(_round_up(cout, 16), dtype=torch.float32, device=self.dev)
            shift[:cout].copy_(bias.detach())
        frozen = form == frozen_bn.AFFINE      # eval mode, gamma / beta trainable: the running statistics, nothing written
        stats = self._conv_launch(xd, wp, shift, zd, x.n, x.h, x.w, cin, x.cs, cout, z.cs, kh, kw, stride, pad,
                                  ACT_NONE, weight=weight, want_stats=bias is None and not frozen)
        mom = 0.1 if bn.momentum is None else bn.momentum
        if not frozen:
            mean, istd = self._empty(cout), self._empty(cout)
            self.bns.append(bn)
        if frozen:                 # no statistics launch, no finalise: the running mean and the folded 1/sigma
            mean, istd = bn.running_mean, self.o.folds.get(bn, None, form, self.st)[0]
        elif stats is not None:      # the conv epilogue wrote per-tile partial sums: only the finalise stage is left
            _lib.check(L.egn_bn_stats_finalize_f32(_lib.ptr(stats[0]), stats[1], rows, cout, bn.eps, _lib.ptr(mean),
                                                   _lib.ptr(istd), None, _lib.ptr(bn.running_mean),
                                                   _lib.ptr(bn.running_var), mom, self.st), 'bn_stats_finalize')
        else:
            _lib.check(L.egn_bn_stats_f32(_lib.ptr(zd), rows, cout, z.cs, bn.eps, _lib.ptr(mean), _lib.ptr(istd), None,
                                          _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), mom,
                                          _lib.ptr(self.o.col_ws), self.st), 'bn_stats')
        y = self.new(x.n, ho, wo, cout, cs=z.cs, name=tag)
        yd = self.data[id(y)]
        relu = 1 if act == ACT_RELU else 0
        if act not in (ACT_NONE, ACT_RELU):
            raise NotImplementedError('activation %d after BatchNorm' % act)
        rd = None if res is None else self.data[id(res)]
        _lib.check(L.egn_bn_act_fwd_f32(_lib.ptr(zd), _lib.ptr(mean), _lib.ptr(istd), _lib.ptr(bn.weight),
                                        _lib.ptr(bn.bias), None, 1.0, relu, _lib.ptr(rd), _lib.ptr(yd), rows, cout,
                                        z.cs, self.st), 'bn_act_fwd')
        self.named[tag] = y
        if self._dead(y, (x, res), param, bias, bn.weight, bn.bias):
            del self.data[id(z)]         # no backward will read the pre-BatchNorm tensor
            return y

        def backward():
            dy = self._take_grad(y)
            if dy is None:
                return
            self.counts['bn_bwd'] += 2
            dbeta = self.o.grad_of(bn.bias) if bn.bias.requires_grad else self._empty(cout)
            dgamma = self.o.grad_of(bn.weight) if bn.weight.requires_grad else self._empty(cout)
            _lib.check(L.egn_bn_bwd_sums_f32(_lib.ptr(dy), _lib.ptr(zd), None, 1.0, _lib.ptr(mean), _lib.ptr(istd),
                                             _lib.ptr(bn.weight), _lib.ptr(bn.bias), relu, _lib.ptr(rd), rows, cout,
                                             z.cs, _lib.ptr(dbeta), _lib.ptr(dgamma), _lib.ptr(self.o.col_ws),
                                             self.st), 'bn_bwd_sums')
            dz = self._empty(dy.numel())
            dres = self._empty(dy.numel()) if (res is not None and id(res) not in self.no_grad) else None
            _lib.check(L.egn_bn_bwd_dz_f32(_lib.ptr(dy), _lib.ptr(zd), None, 1.0, _lib.ptr(mean), _lib.ptr(istd),
                                           _lib.ptr(bn.weight), _lib.ptr(bn.bias), relu, _lib.ptr(rd),
                                           _lib.ptr(self.o.zeros if frozen else dbeta),
                                           _lib.ptr(self.o.zeros if frozen else dgamma), _lib.ptr(dz), _lib.ptr(dres), rows,
                                           cout, z.cs, self.st), 'bn_bwd_dz')
            # (frozen statistics: zero sum vectors leave dz = gamma * istd * dpre, the derivative with constant mean and
            # variance; the hook's dict describes the batch-statistics backward and is not called for such a layer)
            if self.o.debug_hook is not None and not frozen:
                self.o.debug_hook(dict(tag=tag, dy=dy, z=zd, mean=mean, istd=istd, bn=bn, res=rd, dbeta=dbeta,
                                       dgamma=dgamma, dz=dz, dres=dres, relu=relu, rows=rows, cols=cout, ld=z.cs))
            if dres is not None:
                self._accum(res, dres)
            if bias is not None and bias.requires_grad:
                # colsum(dz): zero up to rounding (BatchNorm removes a constant shift), as in the reference
                _lib.check(L.egn_colsum_f32(_lib.ptr(dz), rows, cout, z.cs, _lib.ptr(self.o.grad_of(bias)),
                                            _lib.ptr(self.o.col_ws), self.st), 'bias grad')
            if param.requires_grad:
                self._wgrad(x, xd, dz, z.cs, weight, stride, pad)
            self._accum_dgrad(x, dz, ho, wo, z.cs, weight, stride, pad)
        backward.params = [param, bn.weight, bn.bias] + ([bias] if bias is not None else [])
        self.back.append(backward)
        return y

    def _conv_frozen(self, x, xd, param, weight, bias, bn, act, res, stride, pad, ho, wo, cout_cs, tag):
        """conv + BatchNorm in eval mode with gamma and beta frozen (frozen_bn.FUSED): ONE forward launch, the conv with
        the folded scale / shift (the owner's FoldTable) plus residual and ReLU in its epilogue -- the inference form of
        the layer, on whichever family the tuner hands the tape; no pre-BatchNorm tensor exists.  Backward:
        egn_bn_frozen_bwd_f32 gates dy by the OUTPUT and scales it, one pass instead of two reductions and bn_bwd_dz."""
        L = self.L
        cout, cin, kh, kw = weight.shape
        if act not in (ACT_NONE, ACT_RELU):
            raise NotImplementedError('activation %d after BatchNorm' % act)
        relu = 1 if act == ACT_RELU else 0
        scale, shift = self.o.folds.get(bn, bias, frozen_bn.FUSED, self.st)
        y = self.new(x.n, ho, wo, cout, cs=cout_cs, name=tag)
        yd = self.data[id(y)]
        rd = None if res is None else self.data[id(res)]
        self._conv_launch(xd, None, shift, yd, x.n, x.h, x.w, cin, x.cs, cout, y.cs, kh, kw, stride, pad, act,
                          weight=weight, res=rd, scale=scale)
        self.named[tag] = y
        if self._dead(y, (x, res), param, bias):
            return y
        rows = x.n * ho * wo

        def backward():
            dy = self._take_grad(y)
            if dy is None:
                return
            dz = self._empty(dy.numel())
            dres = self._empty(dy.numel()) if (res is not None and id(res) not in self.no_grad) else None
            self.counts['bn_bwd'] += 1
            frozen_bn.frozen_bwd(L, dy, yd, scale, relu, dz, dres, rows, cout, y.cs, self.st)
            if dres is not None:
                self._accum(res, dres)
            if bias is not None and bias.requires_grad:
                _lib.check(L.egn_colsum_f32(_lib.ptr(dz), rows, cout, y.cs, _lib.ptr(self.o.grad_of(bias)),
                                            _lib.ptr(self.o.col_ws), self.st), 'bias grad')
            if param.requires_grad:
                self._wgrad(x, xd, dz, y.cs, weight, stride, pad)
            self._accum_dgrad(x, dz, ho, wo, y.cs, weight, stride, pad)
        backward.params = [param, bn.weight, bn.bias] + ([bias] if bias is not None else [])
        self.back.append(backward)
        return y

    def fuse(self, terms, relu, tag=''):
        L = self.L
        base = [t for t, s in terms if s == 0][0]
        y = self.new(base.n, base.h, base.w, base.c, cs=base.cs, name=tag)
        yd = self.data[id(y)]
        nt = len(terms)
        ptrs = (C.c_void_p * nt)(*[self.data[id(t)].data_ptr() for t, _ in terms])
        shifts = (C.c_int * nt)(*[s for _, s in terms])
        _lib.check(L.egn_fuse_sum_relu_f32(_lib.ptr(yd), y.n, y.h, y.w, y.c, y.cs, nt, ptrs, shifts, int(relu), self.st),
                   'fuse')
        self.named[tag] = y
        if self._dead(y, [t for t, _ in terms]):
            return y

        def backward():
            dy = self._take_grad(y)
            if dy is None:
                return
            gate = _lib.ptr(yd) if relu else None
            shared = {}
            for t, s in terms:
                if id(t) in self.no_grad:
                    continue
                g = shared.get(s)
                if g is None:
                    g = self._empty(t.n * t.h * t.w * t.cs)
                    _lib.check(L.egn_fuse_bwd_f32(_lib.ptr(dy), gate, _lib.ptr(g), y.n, y.h, y.w, y.cs, s, self.st),
                               'fuse_bwd')
                    shared[s] = g
                self._accum(t, g, owned=False)       # same-shift terms share one tensor
        self.back.append(backward)
        return y


# One output of the module on a finished tape: ``user`` = the tensor the caller sees, ``buf`` = the Buf where its
# gradient enters the tape, ``c`` = the caller tensor's channels (``buf`` may be wider: head1 carries two coordinate
# ramps), ``shuffle`` = the pixel-shuffle factor when ``buf`` holds the pre-shuffle activations (else 0)
HeadOutput = collections.namedtuple('HeadOutput', 'user buf c shuffle')


class TapeOwner(object):
    """What a ``_Tape`` needs from the object that drives it: the library, scratch vectors, the packed-filter
    cache, the weight-gradient side stream and workspace, the kernel-family switches, and ``grad_of(param)`` =
    the tensor a parameter's gradient kernels write.  Two owners: ``HRNetTrainStep`` (the whole iteration
    natively, gradients in one flat buffer) and ``egonet_amd.autograd.HRNetAutograd`` (forward / backward of a
    ``torch.autograd.Function``: torch owns loss and optimiser)."""

    def _init_tape_owner(self, model):
        p0 = next(model.parameters())
        if not p0.is_cuda:
            raise ValueError('%s needs the model on a GPU' % type(self).__name__)
        if model.head_type not in ('coordinates', 'heatmap', 'angleregression'):
            raise NotImplementedError('native training: head_type %r' % (model.head_type,))
        self.model = model
        self._lin4 = {}               # id(nn.Linear weight) -> (weight, its [out, in, 1, 1] view)
        self._lin_of = {}             # id(view) -> the Linear weight
        self.dev = p0.device
        self.L = _lib.lib()
        widest = max(p.shape[0] for p in model.parameters()) + 32
        self.ones = torch.ones(_round_up(widest, 16), dtype=torch.float32, device=self.dev)
        self.zeros = torch.zeros(_round_up(widest, 16), dtype=torch.float32, device=self.dev)
        self.col_ws = torch.zeros(self.L.egn_colreduce_ws_bytes(widest) // 4, dtype=torch.float32, device=self.dev)
        self._wgrad_ws = None         # (the stream whose pool holds it, the workspace)
        # EGONET_AMD_WGRAD_PRIORITY: HIP stream priority of the weight gradients' side stream (0 normal, positive =
        # lower where the runtime has a low level): the chain's latency-bound BatchNorm / reduction kernels should not
        # queue behind the weight gradients' grids.  Assignable: None = one stream (bench.py, GraphedStep).
        self.wgrad_stream = wgrad_side_stream(self.dev, int(os.environ.get('EGONET_AMD_WGRAD_PRIORITY', '0')))
        self.walker = HRNetEngine(model)
        self.packs = PackedFilters(self.dev)
        # frozen layers (frozen_bn.py): the folded scale / shift of the BatchNorm layers in eval mode, one launch per step;
        # the backward stops at the frozen frontier (EGONET_AMD_PRUNE_BACKWARD=0: every op registers its backward as
        # before, for A/B runs); what the last backward launched, plain host counters
        self.folds = frozen_bn.FoldTable(self.dev)
        self.prune_backward = frozen_bn.prune_enabled()
        self.last_backward_launches = None        # {'dgrad': n, 'wgrad': n, 'bn_bwd': n}
        self.debug_hook = None        # tests/train_debug.py: per-layer checks of the BatchNorm backward
        self.timing = None            # bench.py: a list collects (cfg, flops, start, end) per conv launch
        # 3x3 stride-1 forward / data-gradient convolutions may run on the fused Winograd kernels
        # (csrc/conv_wino.hip) where they measured faster (EGONET_AMD_TRAIN_WINO=0: direct kernels only)
        self.allow_wino = os.environ.get('EGONET_AMD_TRAIN_WINO', '1') != '0'
        # ... and on the F(4x4,3x3) kernels (csrc/conv_wino4.hip) [round 5]: EGONET_AMD_TRAIN_F43 = all (forward and
        # data-gradient convolutions), fwd (forward only), 0 (F(2x2,3x3) / direct only)
        f43 = os.environ.get('EGONET_AMD_TRAIN_F43', 'all')
        self.allow_f43 = {'1': 'all', 'all': 'all', 'fwd': 'fwd'}.get(f43, '0')
        # ticket words of the K-split configurations (cfg 83 / 84): zero between launches, shared by the launches of
        # the tape's one stream
        self.tickets = torch.zeros(1 << 16, dtype=torch.int32, device=self.dev)
        torch.cuda.current_stream(self.dev).synchronize()      # (zero in memory before any stream's first launch)
        self.fuse_bn_stats = os.environ.get('EGONET_AMD_FUSE_BN_STATS', '1') != '0'
        self.fuse_grad_add = os.environ.get('EGONET_AMD_FUSE_GRAD_ADD', '1') != '0'

    def grad_of(self, p):
        return p.grad

    def linear4(self, p):
        """The [out, in, 1, 1] view of an nn.Linear weight the tape convolves with: ONE view object per parameter
        (the packed-filter cache is keyed by its id), re-made when the parameter's storage moved."""
        ent = self._lin4.get(id(p))
        if ent is None or ent[1].data_ptr() != p.data_ptr():
            v = p.detach().view(p.shape[0], p.shape[1], 1, 1)
            ent = (p, v)
            self._lin4[id(p)] = ent
            self._lin_of[id(v)] = (v, p)
        return ent[1]

    def param_of(self, weight):
        """The parameter whose gradient a conv filter's weight-gradient launch writes (a Linear's view -> the Linear
        weight: ``grad_of`` is keyed by the parameter)."""
        ent = self._lin_of.get(id(weight))
        return ent[1] if ent is not None and ent[0] is weight else weight

    def wgrad_ws(self, nbytes):
        side = self.wgrad_stream
        if self._wgrad_ws is None or self._wgrad_ws[0] is not side or self._wgrad_ws[1].numel() * 4 < nbytes:
            # allocated in the pool of the stream that uses it: when it has to grow, or ``wgrad_stream`` was
            # reassigned, the old block is only handed to later work of the stream that used it
            with torch.cuda.stream(side if side is not None else torch.cuda.current_stream(self.dev)):
                self._wgrad_ws = (side, torch.empty(nbytes // 4 + 1024, dtype=torch.float32, device=self.dev))
        return self._wgrad_ws[1]

    def head_outputs(self, tape):
        """The module's outputs on ``tape`` as ``HeadOutput``s, in the order ``model(x)`` returns them."""
        m, n, J = self.model, tape.images.shape[0], self.model.num_joints
        if m.head_type == 'coordinates':
            return [HeadOutput(tape.maps_user, tape.named['head1'], J, 0),
                    HeadOutput(tape.user['head2.4'].view(n, J, 2), tape.named['head2.4'], 2 * J, 0)]
        if m.head_type == 'angleregression':
            out = tape.named['final_fc.3']
            return [HeadOutput(tape.user['final_fc.3'].view(n, out.c), out, out.c, 0)]
        if m.pixel_shuffle:            # the maps' gradient goes to the pre-shuffle activations
            return [HeadOutput(tape.user['upsample_layer.3'], tape.named['upsample_layer.3'], J, int(m.upsamp_fact))]
        return [HeadOutput(tape.user['final_layer'], tape.named['final_layer'], J, 0)]

    def seed_grad(self, tape, out, g):
        """The gradient ``g`` of ``out.user`` (contiguous fp32, the caller's layout) enters the tape: converted into
        the padded NHWC layout of ``out.buf``."""
        b = out.buf
        if id(b) in tape.no_grad:
            return
        d = tape._empty(b.n * b.h * b.w * b.cs)
        if out.shuffle:
            _lib.check(self.L.egn_pixel_unshuffle_nchw_to_nhwc_f32(_lib.ptr(g), _lib.ptr(d), b.n, out.c, b.h, b.w, b.cs,
                                                                  out.shuffle, tape.st), 'pixel_unshuffle')
        else:
            _lib.check(self.L.egn_nchw_to_nhwc_f32(_lib.ptr(g), _lib.ptr(d), b.n, out.c, b.h, b.w, b.cs, tape.st))
        tape._accum(b, d)

class HRNetTrainStep(TapeOwner):
    """``step(images, target, joints_xy)`` = one iteration of trainer.py:183-209.  On the plain 'heatmap' head
    ``w_coor`` and ``w_cr`` train the coordinate and cross-ratio terms on the soft-arg-max of the maps
    (function.py:187-201, csrc/softargmax.hip) and ``last_coords`` holds it; with ``w_coor=0`` and no ``w_cr`` the map
    term runs alone.  ``angle_type`` ('mse' | 'sl1'): the criterion of the 'angleregression' head (MSELoss1D /
    SmoothL1Loss1D, function.py:204-228); ``step(images, target [N,2])`` then, and ``last_angles`` holds the [N,2]
    prediction."""

    CR_CRITERIA = {'mse': 0, 'l1': 1, 'sl1': 2}      # loss_dict, function.py:17-20

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, w_hm=1.0, w_coor=0.1, grad_sync=None,
                 sigma=1, w_cr=None, cr_type='sl1', cr_indices=None, target_cr=4.0 / 3.0, cr_loss_thres=0.15,
                 hm_type='mse', coor_type='l1', optim_type='adam', momentum=0.0, weight_decay=0.0,
                 use_target_weight=False, angle_type=None, optim_spec=None, max_grad_norm=None):
        self._init_tape_owner(model)
        p0 = next(model.parameters())
        self.angle_crit = None
        if model.head_type == 'angleregression':
            if angle_type is None:
                raise NotImplementedError(
                    "the 'angleregression' head trains with MSELoss1D or SmoothL1Loss1D (function.py:204-228), not with "
                    "the heat-map / coordinate terms: pass angle_type='mse' or 'sl1' (trainer.make_step reads it from "
                    "the criterion); without it this head has no loss in the reference's composite criterion for the "
                    "step to run")
            if angle_type not in ('mse', 'sl1'):
                raise NotImplementedError("angle_type %r (function.py:204-228 defines 'mse' = MSELoss1D and 'sl1' = "
                                          "SmoothL1Loss1D)" % (angle_type,))
            given = dict(w_hm=(w_hm, 1.0), w_coor=(w_coor, 0.1), w_cr=(w_cr, None), cr_indices=(cr_indices, None),
                         hm_type=(hm_type, 'mse'), coor_type=(coor_type, 'l1'), use_target_weight=(use_target_weight, False))
            bad = sorted(k for k, (v, default) in given.items() if v is not default and v != default)
            if bad:
                raise ValueError("the angle head has one term, angle_type; %s belong to the heat-map, coordinate and "
                                 "cross-ratio terms of the other heads" % ', '.join(bad))
            self.angle_crit = self.CR_CRITERIA[angle_type]
            w_hm = w_coor = 0.0                   # the heat-map / coordinate terms do not exist for this head
        elif angle_type is not None:
            raise ValueError('angle_type is the criterion of the angle head; this model has head_type %r'
                             % (model.head_type,))
        # The plain 'heatmap' head trains the coordinate and cross-ratio terms on the soft-arg-max of its maps
        # (function.py:187-201: coordinates_pred == None -> soft_arg_max(heatmaps_pred) / hm_size), csrc/softargmax.hip.
        has_cr = w_cr not in (None, 'None')
        if model.head_type == 'heatmap' and (w_coor or has_cr):
            if model.pixel_shuffle:
                raise NotImplementedError("the pixel-shuffle 'heatmap' head trains with the heat-map term only (w_coor=0, "
                                          "no w_cr): the soft-arg-max kernel reads the maps of the plain head, not the "
                                          "pre-shuffle activations this head's gradient enters at")
            if use_target_weight:
                raise NotImplementedError('use_target_weight is JointsMSELoss (function.py:22-46), which has no '
                                          'coordinate or cross-ratio term: pass w_coor=0 and no w_cr with it')
        # JointsMSELoss(use_target_weight) (function.py:22-46, the heat-map head's criterion): both maps are multiplied
        # by target_weight[:, k] before the per-joint MSE.  JointsCompositeLoss (the coordinate head) stores the flag and
        # never uses it (function.py:95-111), so there it changes nothing -- like the reference.
        self.use_target_weight = bool(use_target_weight) and model.head_type == 'heatmap'
        if self.use_target_weight and hm_type != 'mse':
            raise NotImplementedError('JointsMSELoss is an MSE criterion (function.py:24-26)')
        self.lr, self.betas, self.eps = lr, betas, eps
        if optim_type not in ('adam', 'sgd'):
            raise NotImplementedError('optimizer %r (optimizer.py:8-40 knows adam and sgd)' % (optim_type,))
        self.optim_type, self.momentum, self.weight_decay = optim_type, float(momentum), float(weight_decay)
        # criteria of the heat-map and coordinate terms: any of loss_dict (function.py:17-20)
        self.hm_crit, self.coor_crit = self.CR_CRITERIA[hm_type], self.CR_CRITERIA[coor_type]
        self.w_hm, self.w_coor = float(w_hm), float(w_coor or 0.0)
        # cross-ratio term (function.py:113-153, train_IGRs.py:44-46): off unless a weight is
        # given ('None' in the shipped YAML) AND apply_cr_loss is set (trainer.py:168-169:
        # from the second epoch on)
        self.w_cr = None if w_cr in (None, 'None') else float(w_cr)
        self.apply_cr_loss = False
        self.cr_idx = None
        if self.w_cr is not None:
            if model.head_type not in ('coordinates', 'heatmap'):
                raise NotImplementedError('the cross-ratio term needs the coordinate head or the plain heat-map head')
            if cr_indices is None:
                from .common.img_proc import CR_INDICES_BBOX12
                cr_indices = CR_INDICES_BBOX12
            idx = torch.as_tensor(cr_indices, dtype=torch.int32).reshape(-1, 4)
            if int(idx.min()) < 0 or int(idx.max()) >= model.num_joints:
                raise ValueError('cr_indices outside 0..%d' % (model.num_joints - 1))
            self.cr_idx = idx.contiguous().to(p0.device)
            self.cr_crit = self.CR_CRITERIA[cr_type]
            self.target_cr, self.cr_loss_thres = float(target_cr), float(cr_loss_thres)
        self.grad_sync = grad_sync
        self.sigma = sigma           # heatmapModel.sigma: targets drawn on the device when step(target=None)
        self.last_target_weight = None
        self.flat = FlatParams(model.parameters())
        # parameter groups / AdamW / AMSGrad / Nesterov / dampening / clipping: the grouped update (optim.py); what the
        # old entry points can express stays on them (self.grouped is None)
        optim.attach(self, optim_spec, max_grad_norm)
        self.loss_dev = torch.zeros(1, dtype=torch.float64, device=self.dev)
        self.counters = StepCounters()
        self.last_maps = self.last_coords = self.last_angles = None

    def set_lrs(self, lrs):
        """One learning rate per parameter group (the scheduler's values); without groups, the one ``lr``."""
        optim.set_lrs(self, lrs)

    @property
    def last_grad_norm(self):
        """With ``max_grad_norm``: the last step's total gradient norm, a device scalar (no read-back); else None."""
        return None if self.grouped is None else self.grouped.last_grad_norm

    state_kind = 'hrnet'

    def state_dict(self):
        """Everything but the parameters that continues this step's run (train_state.py): a snapshot in plain
        containers and CPU tensors, ``apply_cr_loss`` included."""
        return train_state.state_dict(self)

    def load_state_dict(self, sd, strict=True):
        """In place, after validation (train_state.load_state_dict)."""
        train_state.load_state_dict(self, sd, strict)

    def _drawn_target(self, joints_xy, joints_vis, n, h, w, mh, mw):
        """Gaussian heat-map targets drawn on the device from the joints at heatmap_size (img_proc.py:347-409): the
        [N,K,h,w] target never crosses PCIe.  Their weights stay in ``last_target_weight``."""
        if joints_xy is None:
            raise ValueError('step() needs target heat-maps or joints_xy to draw them from')
        if mh != mw or h != w:
            raise NotImplementedError('device-side targets: square maps only (the reference mixes the '
                                      'width/height indices of input_size / heatmap_size, img_proc.py:376-383)')
        from .common import img_proc
        target, self.last_target_weight = img_proc.generate_target_batch(
            joints_xy, torch.ones(n, self.model.num_joints) if joints_vis is None else joints_vis,
            dict(target_type='gaussian', input_size=(w, h), heatmap_size=(mh, mw), sigma=self.sigma),
            device=self.dev)
        return target

    def _target_weight(self, target_weight, n):
        """JointsMSELoss's target_weight as [N, K] on the device (default: that of the device-drawn targets)."""
        tw = target_weight if target_weight is not None else self.last_target_weight
        if tw is None:
            raise ValueError('use_target_weight needs target_weight [N,K(,1)] (or device-drawn targets)')
        return torch.as_tensor(tw, dtype=torch.float32).reshape(n, self.model.num_joints).to(self.dev)

    def _angle_loss(self, tape, out, target, n, st):
        """MSELoss1D / SmoothL1Loss1D (function.py:204-228: nn.MSELoss / nn.SmoothL1Loss, 'mean' over the 2N elements)
        and the gradient seed at final_fc.3 in one launch of egn_elem_loss_f32: rows of the padded activations against
        the compact [N, 2] target; the padding columns of the gradient stay zero."""
        self.last_angles, out = out.user, out.buf
        if target is None or tuple(target.shape) != (n, out.c):
            raise ValueError('target must be [%d, %d] rows of [cos, sin], got %s'
                             % (n, out.c, None if target is None else tuple(target.shape)))
        dpad = torch.zeros(n * out.cs, dtype=torch.float32, device=self.dev)
        _lib.check(self.L.egn_elem_loss_f32(_lib.ptr(tape.data[id(out)]), _lib.ptr(target), n, out.c, out.cs, out.c,
                                            self.angle_crit, 1.0, 0, _lib.ptr(dpad), _lib.ptr(self.loss_dev), st),
                   'angle loss')
        tape.grad[id(out)] = [dpad, True]

    def _pixshuf_loss(self, tape, out, target, joints_xy, joints_vis, target_weight, n, h, w, st):
        """The pixel-shuffle head's JointsMSELoss-style term (hrnet.py:373-383, 598-600; function.py:22-46) as ONE
        launch, egn_pixshuf_loss_f32: it reads the pre-shuffle activations and the NCHW target and writes the gradient
        in the pre-shuffle layout (the shuffled maps in ``last_maps`` are for the caller only)."""
        L, J = self.L, self.model.num_joints
        u, f = out.buf, out.shuffle                       # pre-shuffle Buf [N, h, w, J*f*f (padded)]
        mh, mw = u.h * f, u.w * f
        if target is None:
            target = self._drawn_target(joints_xy, joints_vis, n, h, w, mh, mw)
        if tuple(target.shape) != (n, J, mh, mw):
            raise ValueError('target must be %s, got %s' % ((n, J, mh, mw), tuple(target.shape)))
        target = target.contiguous().float()
        twd = self._target_weight(target_weight, n).contiguous() if self.use_target_weight else None
        du = tape._empty(n * u.h * u.w * u.cs)
        _lib.check(L.egn_pixshuf_loss_f32(_lib.ptr(tape.data[id(u)]), _lib.ptr(target), _lib.ptr(twd), n, u.h, u.w, J,
                                          f, u.cs, self.hm_crit, 0.5 * self.w_hm, _lib.ptr(du), _lib.ptr(self.loss_dev),
                                          st), 'pixel-shuffle loss')
        tape._accum(u, du)

    def _coord_terms_on(self):
        return bool(self.w_coor) or (self.w_cr is not None and self.apply_cr_loss)

    def _coord_terms(self, tape, cd, n, n_fs, n_cr, J, joints_xy, w, h, st):
        """L_2d over the first ``n_fs`` rows of the compact coordinates ``cd`` [N, 2K] (function.py:159-168, 194-198)
        and L_cr over the first ``n_cr`` (function.py:113-153, 199-201), added to ``loss_dev``.  Returns d loss /
        d coords as [N * 2K], zero for the rows no term reads."""
        L = self.L
        dc = tape._empty(cd.numel())
        if self.w_coor:
            if joints_xy is None:
                raise ValueError('the coordinate term needs joints_xy')
            gt = torch.as_tensor(joints_xy, dtype=torch.float32).to(self.dev)[..., :2].clone()
            gt[..., 0] /= w            # function.py:160-161 (img_size = (width, height))
            gt[..., 1] /= h
            gt = gt.contiguous()
            if n_fs < n:
                dc.zero_()                            # the unlabelled rows: no coordinate gradient
            cnt = n_fs * 2 * J                        # the labelled rows come first (function.py:194-198)
            _lib.check(L.egn_elem_loss_f32(_lib.ptr(cd), _lib.ptr(gt), 1, cnt, cnt, cnt,
                                           self.coor_crit, self.w_coor, 0, _lib.ptr(dc),
                                           _lib.ptr(self.loss_dev), st), 'coor loss')
        else:
            dc.zero_()
        if self.w_cr is not None and self.apply_cr_loss:
            nl = self.cr_idx.shape[0]
            ws = tape._empty(L.egn_cross_ratio_ws_bytes(n_cr, nl) // 4)
            _lib.check(L.egn_cross_ratio_f32(_lib.ptr(cd), n_cr, J, _lib.ptr(self.cr_idx), nl,
                                             self.target_cr, self.cr_loss_thres, self.cr_crit, self.w_cr,
                                             _lib.ptr(dc), _lib.ptr(self.loss_dev), _lib.ptr(ws), st),
                       'cross_ratio')
        return dc

    def _integral_terms(self, tape, aug, da, n, n_fs, J, joints_xy, w, h, st):
        """The heat-map head's L_2d and L_cr on the soft-arg-max of its maps (function.py:187-201), two launches of
        csrc/softargmax.hip around the coordinate head's term kernels: the forward reads the padded NHWC maps where
        the tape keeps them, the backward adds d loss / d maps to ``da``, which the heat-map term has written.

        The reference's own arithmetic, quirks included: x is divided by hm_size[1] and y by hm_size[0] with hm_size =
        [w, h] (function.py:192-193) -- on non-square maps each axis by the OTHER size; and on a mixed batch the maps
        are cut to the labelled prefix for the heat-map term BEFORE the soft-arg-max (function.py:184-185 rebinds
        heatmaps_pred), so with the heat-map term on L_cr sees the ``n_fs`` labelled crops only; without it all ``n``.
        ``last_coords`` holds all ``n`` rows either way."""
        from . import softargmax
        div_x, div_y = float(aug.h), float(aug.w)     # hm_size[1], hm_size[0]
        z = tape.data[id(aug)]
        coords, save = softargmax.forward(z, n, aug.h, aug.w, J, aug.cs, div_x, div_y, st)
        self.last_coords = coords
        n_cr = n_fs if self.w_hm else n
        dc = self._coord_terms(tape, coords.view(n, 2 * J), n, n_fs, n_cr, J, joints_xy, w, h, st)
        rows = max(n_fs if self.w_coor else 0, n_cr if self.w_cr is not None and self.apply_cr_loss else 0)
        softargmax.backward(z, save, dc, n, rows, aug.h, aug.w, J, aug.cs, div_x, div_y, da, True, st)

    def _labelled_rows(self, n, target, joints_xy):
        """``n_fs``: the rows of ``target`` when it holds fewer than the ``n`` images (a mixed batch: the labelled crops
        first), else ``n``.  Raises where the reference has no labelled-prefix slice or this step has none."""
        m = self.model
        if target is None:
            if joints_xy is not None and len(joints_xy) != n:
                raise ValueError('a labelled prefix (%d joints_xy rows for %d images) with device-drawn targets '
                                 '(target=None): pass the [n_fs,K,h,w] target of the labelled crops'
                                 % (len(joints_xy), n))
            return n
        n_fs = int(target.shape[0])
        if n_fs == n:
            return n
        if n_fs > n or n_fs < 1:
            raise ValueError('target has %d rows for %d images' % (n_fs, n))
        what = ('the angle head' if self.angle_crit is not None else
                'the pixel-shuffle head' if m.head_type != 'coordinates' and m.pixel_shuffle else
                'use_target_weight (JointsMSELoss has no slice, function.py:22-46)' if self.use_target_weight else None)
        if what is not None:
            raise ValueError('a labelled prefix (%d target rows for %d images) with %s: mixed batches train the '
                             "'coordinates' head and the plain 'heatmap' head only" % (n_fs, n, what))
        if joints_xy is not None and len(joints_xy) != n_fs:
            raise ValueError('joints_xy must be [%d, %d, 2] like the target of the labelled crops, got %d rows'
                             % (n_fs, m.num_joints, len(joints_xy)))
        return n_fs

    @torch.no_grad()
    def step(self, images, target, joints_xy=None, update=True, joints_vis=None, target_weight=None):
        """images [N,3,H,W], target [N,K,h,w] heat-maps (None: drawn on the device from
        joints_xy / joints_vis with ``self.sigma``), joints_xy [N,K,2] in input pixels
        (``meta['transformed_joints'][:, :, :2]``).  Returns the loss as a 1-element
        float64 device tensor (no host sync).

        Mixed batches (function.py:183-201): ``target`` and ``joints_xy`` may hold ``n_fs < N`` rows -- the labelled
        crops are the first ``n_fs`` images, the others are unlabelled.  The heat-map and coordinate terms then run
        over the labelled prefix (their means over ``n_fs`` rows, zero gradient for the rest), the cross-ratio term
        and the BatchNorm statistics over all ``N``; ``last_maps`` / ``last_coords`` keep ``N`` rows.  For the
        'coordinates' head and the plain 'heatmap' head with ``target`` given and ``use_target_weight`` off.
        (The plain 'heatmap' head with ``w_coor`` / ``w_cr``: its coordinates are the soft-arg-max of the maps, which the
        reference cuts to the labelled prefix first -- there L_cr covers ``n_fs`` rows too, see ``_integral_terms``.)

        The cyclic garbage collector is paused while the ~1 500 launches of the iteration are issued: a
        full collection in the middle (35 ms measured, every ~10 iterations) starves the GPU and doubles
        that step's time; between steps it hides behind the queued work.  Nothing here needs it -- the
        tape's reference cycles are broken explicitly (``_Tape.release``)."""
        with _gc_paused():
            return self._step(images, target, joints_xy, update, joints_vis, target_weight)

    def _step(self, images, target, joints_xy, update, joints_vis, target_weight=None):
        m, L = self.model, self.L
        if not m.training:
            raise RuntimeError('HRNetTrainStep.step needs model.train()')
        if self.angle_crit is not None and not (joints_xy is None and joints_vis is None and target_weight is None):
            raise ValueError("the angle head's step takes (images, target [N,2]) only: joints_xy, joints_vis and "
                             'target_weight belong to the heat-map and coordinate heads')
        images = images.contiguous().float()
        if target is not None:
            target = target.contiguous().float()
        n, cin, h, w = images.shape
        if h % 32 or w % 32:
            raise ValueError('HRNet input height/width must be multiples of 32, got %dx%d' % (h, w))
        n_fs = self._labelled_rows(n, target, joints_xy)
        with torch.cuda.device(self.dev):
            st = _lib.current_stream(self.dev)
            self.flat.grad.zero_()
            self.packs.pack_all(st)          # every forward / data-gradient filter, one launch
            self.folds.fold_all(st)          # scale / shift of every eval-mode BatchNorm layer, one launch (none: nothing)
            tape = _Tape(self, images)
            self.walker._record(n, cin, h, w, None, r=tape)
            J = m.num_joints
            self.counters.tick(tape.bns, self.loss_dev, st)       # num_batches_tracked += 1, loss = 0: one launch
            outs = self.head_outputs(tape)
            maps = outs[0]
            if m.head_type != 'angleregression':                  # (the angle head has no map term)
                self.last_maps = maps.user
            if m.head_type == 'coordinates':
                self.last_coords = outs[1].user
                cd = self.last_coords.view(n, 2 * J)              # compact [N, 2K] = coords [N,K,2]
                if self._coord_terms_on():
                    dc = self._coord_terms(tape, cd, n, n_fs, n, J, joints_xy, w, h, st)
                    self.seed_grad(tape, outs[1], dc)             # back to the padded NHWC row layout
            if m.head_type == 'angleregression':
                self._angle_loss(tape, outs[0], target, n, st)    # loss and gradient seed in one launch
            elif maps.shuffle:                                    # its loss reads the pre-shuffle activations
                self._pixshuf_loss(tape, maps, target, joints_xy, joints_vis, target_weight, n, h, w, st)
            else:
                aug = maps.buf
                if target is None:
                    target = self._drawn_target(joints_xy, joints_vis, n, h, w, aug.h, aug.w)
                if tuple(target.shape) != (n_fs, J, aug.h, aug.w):
                    raise ValueError('target must be %s, got %s' % ((n_fs, J, aug.h, aug.w), tuple(target.shape)))
                # the labelled crops are a contiguous prefix of the NHWC maps (function.py:183-186): the rows beyond
                # n_fs * h * w are not read, and their gradient stays zero
                tg = tape._empty(n_fs * aug.h * aug.w * aug.cs)
                _lib.check(L.egn_nchw_to_nhwc_f32(_lib.ptr(target), _lib.ptr(tg), n_fs, J, aug.h, aug.w, aug.cs, st))
                da = torch.zeros(n * aug.h * aug.w * aug.cs, dtype=torch.float32, device=self.dev)
                pred_flat = tape.data[id(aug)]
                wv = None
                if self.use_target_weight:
                    # 0.5 * mean((pred * w - gt * w)^2): the same kernel on the weighted maps, gradient * w afterwards
                    # (three broadcast multiplies over [N,h,w,K]; an option no shipped configuration switches on)
                    wv = torch.zeros(n, 1, 1, aug.cs, dtype=torch.float32, device=self.dev)
                    wv[:, 0, 0, :J] = self._target_weight(target_weight, n)
                    pred_flat = (pred_flat.view(n, aug.h, aug.w, aug.cs) * wv).reshape(-1)
                    tg = (tg.view(n, aug.h, aug.w, aug.cs) * wv).reshape(-1)
                # (1/K) sum_k 0.5*crit_k = 0.5 * crit over all joints (equal element counts), function.py:95-111
                _lib.check(L.egn_elem_loss_f32(_lib.ptr(pred_flat), _lib.ptr(tg), n_fs * aug.h * aug.w, J, aug.cs,
                                               aug.cs, self.hm_crit, 0.5 * self.w_hm, 0, _lib.ptr(da),
                                               _lib.ptr(self.loss_dev), st), 'hm loss')
                if wv is not None:
                    da = (da.view(n, aug.h, aug.w, aug.cs) * wv).reshape(-1)
                if m.head_type == 'heatmap' and self._coord_terms_on():     # (the coordinate head has its own, above)
                    self._integral_terms(tape, aug, da, n, n_fs, J, joints_xy, w, h, st)
                tape._accum(aug, da)
            sess = begin_grad_sync(self, tape.back)
            for fn in reversed(tape.back):
                fn()
                if sess is not None:
                    sess.done(getattr(fn, 'params', ()))
            tape.join_side()
            finish_step(self, sess, update, st)
            self.packs.finalize()     # first step: the set of filters is known now
            self.folds.finalize()
            self.last_backward_launches = dict(tape.counts)
            invalidate(m)             # the inference engine caches folded weights (raw-pointer writes)
            if self.debug_hook is not None:
                self.last_tape = tape
            else:
                tape.release()
        return self.loss_dev
