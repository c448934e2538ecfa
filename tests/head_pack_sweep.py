"""The launches of a native training step that no other sweep owns -- csrc/heads.hip (the pixel-shuffle criterion,
PixelUnshuffle, the angle head's average pools), csrc/cross_ratio.hip and the filter packers of csrc/filter_pack.hip /
filter_pack.h / wino4_pack.h -- as the product records them, the edges of their kernels and launchers, their inputs and
the element-wise checks of the sweep.

Helper module of tests/test_head_pack_sweep_cpu.py and tests/test_gpu_head_pack_sweep.py (imported, not a conftest).
Sixth of the family of tests/conv_sweep.py, tests/wgrad_sweep.py, tests/train_ops_sweep.py, tests/gemm_sweep.py and
tests/program_ops_sweep.py, and the one that closes it for training: ``OWNERS`` names, for every entry point the step
modules (train_hrnet.py, train_lifter.py, train_common.py, filters.py) call, the GPU test file that holds it to float64;
``QUERIES`` are the host-only ones.  A step that starts calling a new entry point fails the CPU test until it is listed.

A request is a dict as in train_ops_sweep: 'name' (the entry point), 's' (its scalars by the names of ``ARGS``), 'null'
(the pointer arguments that are NULL), 'alias', 'opt' (input options: 'content', 'off' = floats an operand starts
inside its allocation, 'loss0' / 'base' = what an accumulated output holds on entry, 'idx' = the line table, 'refuse' =
the launcher must return EGN_E_BADARG and write nothing), 'srcs' and, on an edge request, 'line': (file, text) of the
kernel line it is there for.  ``recorded_requests`` runs conv_sweep.TAPE_STEPS and ``EXTRA_RUNS`` under ``HeadRecorder``
(train_ops_sweep.Recorder with this module's names; it keeps a double argument as a double and notes which operands were
not 16-byte aligned).  The batch packer's request is its descriptor table read back from the device after the second
step: [(Cout, Cin, taps, code, begin)].  egn_pixel_unshuffle_nchw_to_nhwc_f32 is reached through one backward of the
autograd.py bridge of a pixel-shuffle model (a tiny one: the bridge runs in well under a second).
``EDGE_ONLY``: egn_pack_matrix_f32 is not launched by any recorded step -- LifterCore._gemm calls it only for a matrix
that is neither on the dense-GEMM route (egn_gemm_supported) nor a registered nn.Linear weight (those go through
PackedFilters as 1 x 1 filters: egn_pack_conv_weight_f32), which no shipped lifter has; the edge list alone covers it.

Every launch (tests/test_gpu_head_pack_sweep.py): outputs NaN-filled between sweep_guards bands, the cross-ratio
workspace a band of exactly egn_cross_ratio_ws_bytes; inputs with NaN where the kernel must not look (pad channels of
the pixel-shuffle x, pad columns of a pitched matrix, 64 floats in front of and behind every operand) and compared bit
for bit afterwards; a second launch gives the same bits (the pixshuf loss scalar, reached by atomicAdd from many blocks:
twice the bound).  A refused request launches nothing: its NaN-filled outputs keep their bits.

THE CHECKS.  U = 2^-24;  |got - want64| <= C U A,  A the same formula on absolute values; A = 0 means exact.
pixshuf_loss  d = x w - t w (w = 1 without tw), inv = weight / (N C H up W up) in double.
  dx    mse: A = 2 inv |w| (|x w| + |t w|);  smooth-l1 is 1-Lipschitz in d: the same with factor 1;  l1: the gradient is
        +-inv w rounded once, A = inv |w|, where the sign of d is decided: an element with |d64| <= C U (|x w| + |t w|)
        is left out (cap 0.1 % of a case).  'ints' content (x, t integers in [-4, 4], tw in {0, 1, 2}, weight a power
        of two): every d is exact and the gradient equals float32(c'(d) inv) w, A = 0.  Planted in every content:
        d = 0 (x bit-equal to t: l1's gradient exactly 0) and |d| = 1 exactly.  Pad channels of dx: exactly 0.
  loss  loss0 + inv sum(v);  A = |loss0| + inv sum A_v,  A_v = (|x w| + |t w|)^2 for mse (v = d^2, d with a relative
        error on |x w| + |t w|), |x w| + |t w| otherwise; the double sum's own rounding (2^-53 per term) is far below.
pixel_unshuffle  every bit against the index formula of include/egonet_hip.h; pads exactly 0.
avgpool  forward: the k^2 taps summed, then / k^2: A = sum|x| / k^2.  backward: dx = dy / k^2 (+ base), A = |dy| / k^2
  (+ |base|); without accumulate at a power-of-two k exact (A = 0); a floor-cropped row / column is 0, or the base's bits.
cross_ratio  written out in ``_cross_ratio``: with e = the relative error of cr (four squared lengths of rounded
  differences, three multiply / divide, the rounded target^2), x = cr - 1:
      A_x = |cr| + |x|;   A_g = 2 A_x (mse), A_x (smooth-l1), 0 (l1: the sign is decided or the case is left out);
      A_v = |c'(x)| A_x;  the four quotients q = +-2 g cr / |PQ|^2:  A_q = 2 (A_g |cr| + |g| |cr|) / |PQ|^2;
      ws[0..7] = sums of q (Q - P):  A = sum A_q |Q - P|;   ws[8] = v: A_v;   ws[9] = the mask, exact;
      dcoords = base + float(scale sum_lines ws):  A = |base| + scale sum A_ws;   loss = loss0 + scale sum v (double):
      A = |loss0| + scale sum A_v;   scale = weight / sum(mask).
  The mask is exact away from the undecided lines: |dmin64 - thres| <= 4 U dmin64 (then the whole case's normalisation
  moves and the case is checked for writes and guards only; only the case that plants dmin == thres may be).  Where
  float64 gives no finite number (a kept line with B == C or A == D: cr = inf in the reference too) the kernel must not
  either.  A kept line with A == C or B == D has cr = 0 and, by the reference's autograd, gradient 0 for all four
  points; the kernel computed 0 / 0 there until this sweep (fixed in cross_ratio.hip, the request stays in the list).
  The issue's collinear points 0, 1, 3, 4 have cross ratio 9/8, not 4/3; 0, 1, 2, 3 have 4/3 and give cr = 1 exactly
  in fp32 (checked on the CPU), but float64 divides the exact 16/9 by the fp32-rounded target^2 and sees 6e-8: the zero
  gradient that is exact in BOTH arithmetics is planted with a square of side 1/4 and target 2 (cr = 4 / 4); the same
  square with target sqrt(2) gives cr = 2, |cr - 1| = 1 exactly.
packers  direct layout (egn_pack_conv_weight_f32, egn_pack_matrix_f32): a permutation plus zeros, every bit against
  the index formula of include/egonet_hip.h on all-distinct values (``pack_ref``; filters.pack_conv_weight is the
  independent statement on the CPU).  Winograd layouts: U = G g G^T in float64 rounded once: |U - U64| <= U |U64|
  (derived: one rounding of a float64 value; the float64 transform's own error is 2^-29 of that), and every bit on
  integer filters (multiples of 4 / of 576: G g G^T is exact); pads of the F(4x4) layout exactly 0; every float written.
  The *_floats queries against the launches on a grid around the accepted shapes: a count means return 0 and that many
  floats written, no count means EGN_E_BADARG and nothing written.  Batch packer: every descriptor's output equal bit
  for bit, on the device, to the single entry point's for that (weight, code).

THE CONSTANTS: four times the worst ratio of ``emulate`` (the header's arithmetic in fp32 torch on the CPU, on the edge
list's inputs; tests/test_head_pack_sweep_cpu.py prints the table), + 2 per sqrtf or non-power-of-two division of the
kernel (1 ulp each by the HIP math API's table, as in train_ops_sweep).  Never from the kernel.
  entry               worst emulation ratio            C
  pixshuf_loss        dx 1.84 (mse, tw with zeros), loss 0.11    8
  avgpool_fwd         2.90 (k 3 on 7 x 6, cs 260)                12 + 2   (the division by k^2)
  avgpool_bwd         1.38 (k 3, accumulate)                     6 + 2    (the same)
  cross_ratio         ws 2.84, dcoords 2.72, loss 1.16 (l1 / mse, the product's 12 lines)
                                                                 12 + 6   (three divisions on every value's path: by
                                                                          |BC|^2 |AD|^2, by target^2, by |PQ|^2; the six
                                                                          sqrtf feed the mask only)
  pixel_unshuffle, the direct layout: exact.  Winograd layouts: 1 (derived).
``MUTANTS``: wrong kernels applied to the emulations / the layout references; each breaks an exact case or the bound on
the list's own inputs (CPU test).  'cr_gather_joint_order' adds the lines' gradients of a joint in another order: it
changes only the last bits of a float sum, far inside the bound; it is listed in ``BITS_ONLY`` and the CPU test asserts
that it is NOT caught, so that nobody believes it is.

Measured on the MI355X (tests/test_gpu_head_pack_sweep.py, worst |err| / (U A) per entry point):
  3482 recorded launches, 156 distinct requests; 193 edge requests (26 refusals); 318 query-grid shapes (32 accepted);
  the recorded batch table: 611 descriptors, 32 041 856 units (W48 'coordinates', second step), and four edge tables.
  entry                 recorded                          edge                                      C
  pixshuf_loss          3 requests    1.94 (dx, W48 f 2)   51 requests   below that                  8
  pixel_unshuffle       1             every bit            11            every bit                   exact
  avgpool_fwd           1             1.97                 15            2.90 (k 3 on 7 x 6, cs 260)  14
  avgpool_bwd           1             exact (k 4)          22            1.38 (k 3, accumulate)      8
  cross_ratio           2             1.75 (ws, mse)       33            2.69 (ws, l1, 12 lines)     18
  pack_conv_weight      134           every bit            29            every bit                   exact
  pack_matrix           none (EDGE_ONLY)                   8             every bit                   exact
  wino_pack_weight      7             1.00                 16            1.00                        1
  wino4_pack_weight     7             1.00                 8             1.00                        1
The kernels follow the emulated order to the figure (avgpool 2.90 / 1.38 are the emulation's own numbers on the same
request; cross_ratio 2.69 against 2.84).  Only the Winograd layouts sit above a third of their constant, at all of it:
the bound is the derived one, a single rounding of a float64 value, and |fl(u) - u| / (U |u|) reaches 1 for a u just
above a power of two; among 10^5 values some are.  A second rounding anywhere would show as a ratio above 1.
No kernel body failed.  Reading the launchers for the sweep found: egn_pack_matrix_f32, egn_avgpool_fwd / bwd_f32 and
egn_pixel_unshuffle_nchw_to_nhwc_f32 launched on NULL operands (now EGN_E_BADARG, on the list as refusals), and the
0 / 0 of cr_lines_kernel on a kept line with A == C or B == D (above).  The size queries and the launches agree on every
shape of the grid: both go through fp_floats.
"""
import ctypes as C
import math
import os
import re
import zlib

import numpy as np
import torch

import conv_sweep as S
import train_ops_sweep as T
from egonet_amd import _lib, filters

U = S.U
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, 'egonet_amd', 'csrc')
GPU_TEST = 'test_gpu_head_pack_sweep.py'
CK = filters.CK
NAN = float('nan')
L1_CAP = 1e-3                    # share of a case's elements whose l1 sign may be undecided
FP_DGRAD, FP_WINO2, FP_WINO4 = 1, 2, 4

_ARGS_TEXT = {
    'egn_pixshuf_loss_f32': 'x:in tgt:in tw:in N H W C up cs crit weight dx:out loss:io',
    'egn_pixel_unshuffle_nchw_to_nhwc_f32': 'x:in y:out N C H W cs up',
    'egn_avgpool_fwd_f32': 'x:in y:out N H W cs k',
    'egn_avgpool_bwd_f32': 'dy:in dx:io N H W cs k accumulate',
    'egn_cross_ratio_f32': 'coords:in N K idx:in L target_cr thres crit weight dcoords:io loss:io ws:ws',
    'egn_pack_conv_weight_f32': 'w:in Cout Cin KH KW dgrad dst:out',
    'egn_pack_matrix_f32': 'src:in ld cout cin transpose dst:out',
    'egn_wino_pack_weight_f32': 'w:in Cout Cin dgrad dst:out',
    'egn_wino4_pack_weight_f32': 'w:in Cout Cin dgrad dst:out',
    'egn_pack_conv_weights_batch_f32': 'descs:in n total',
}
ARGS = {k: [tuple((a.split(':') + [None])[:2]) for a in v.split()] for k, v in _ARGS_TEXT.items()}
LAUNCHING = tuple(ARGS)
BATCH = 'egn_pack_conv_weights_batch_f32'
EDGE_ONLY = ('egn_pack_matrix_f32',)         # called by train_lifter.py, reached by no recorded step (docstring)
PACKERS = ('egn_pack_conv_weight_f32', 'egn_pack_matrix_f32', 'egn_wino_pack_weight_f32', 'egn_wino4_pack_weight_f32')
# host-only queries of this sweep -> the launch each sizes
SIZES = {'egn_packed_weight_floats': 'egn_pack_conv_weight_f32', 'egn_wino_weight_floats': 'egn_wino_pack_weight_f32',
         'egn_wino4_pack_weight_floats': 'egn_wino4_pack_weight_f32', 'egn_cross_ratio_ws_bytes': 'egn_cross_ratio_f32',
         'egn_pack_desc_bytes': BATCH}
# every host-only query the step modules call: nothing launched, nothing to replay
QUERIES = set(SIZES) | {'egn_conv2d_bnstats_rows', 'egn_conv2d_wgrad_ws_bytes', 'egn_colreduce_ws_bytes',
                        'egn_gemm_supported', 'egn_gemm_ws_bytes', 'egn_gemm_stats_rows'}
STEP_MODULES = ('train_hrnet.py', 'train_lifter.py', 'train_common.py', 'filters.py')
# every launching entry point the step modules call -> the GPU test file of the sweep that owns it
OWNERS = dict(
    {k: 'test_gpu_conv_sweep.py' for k in ('egn_conv2d_f32', 'egn_conv2d_ex_f32', 'egn_conv2d_bnstats_f32')},
    **{'egn_conv2d_wgrad_f32': 'test_gpu_wgrad_sweep.py'},
    **{k: 'test_gpu_train_ops_sweep.py' for k in (
        'egn_add_f32', 'egn_zero_insert2_f32', 'egn_sigmoid_bwd_f32', 'egn_colsum_f32', 'egn_bn_stats_f32',
        'egn_bn_stats_finalize_f32', 'egn_bn_act_fwd_f32', 'egn_bn_act_fwd_drop_f32', 'egn_bn_bwd_sums_f32',
        'egn_bn_bwd_sums_drop_f32', 'egn_bn_bwd_dz_f32', 'egn_bn_bwd_dz_drop_f32', 'egn_fuse_bwd_f32',
        'egn_elem_loss_f32', 'egn_mse_f32', 'egn_step_counters_i64', 'egn_adam_step_dev_f32',
        'egn_adam_l2_step_dev_f32', 'egn_sgd_step_dev_f32')},
    **{k: 'test_gpu_gemm_sweep.py' for k in ('egn_gemm_f32', 'egn_gemm_ex_f32')},
    **{k: 'test_gpu_program_ops_sweep.py' for k in (
        'egn_nchw_to_nhwc_f32', 'egn_nhwc_to_nchw_f32', 'egn_pixel_shuffle_nhwc_to_nchw_f32',
        'egn_fill_coord_ramps_f32', 'egn_fuse_sum_relu_f32')},
    **{k: GPU_TEST for k in LAUNCHING})

C_BOUND = {
    'egn_pixshuf_loss_f32': 8.0, 'egn_pixel_unshuffle_nchw_to_nhwc_f32': 0.0, 'egn_avgpool_fwd_f32': 14.0,
    'egn_avgpool_bwd_f32': 8.0, 'egn_cross_ratio_f32': 18.0, 'egn_pack_conv_weight_f32': 0.0,
    'egn_pack_matrix_f32': 0.0, 'egn_wino_pack_weight_f32': 1.0, 'egn_wino4_pack_weight_f32': 1.0,
}


def kernel_text(name):
    with open(os.path.join(_CSRC, name)) as fh:
        return fh.read()


def called_entries():
    """Every egn_* name the step modules call, from their text."""
    called = set()
    for f in STEP_MODULES:
        with open(os.path.join(_ROOT, 'egonet_amd', f)) as fh:
            called |= set(re.findall(r'\.(egn_\w+)\(', fh.read()))
    return called


# ---------------------------------------------------------------------------------------------------------------
# the launchers' decisions, restated (the CPU test holds the literals against the kernels' text)
# ---------------------------------------------------------------------------------------------------------------
HEADS_GRID = 4096 * 256          # work items of one trip of heads.hip's grid-stride loops (heads_grid)
PACK_ONE_GRID = 4096 * 256       # ... of pack_one_kernel
PACK_BATCH_GRID = 16384 * 256    # ... of pack_conv_weights_batch_kernel
LDS_LIMIT = 65024


def pixshuf_tw(cs):
    tw = 16
    while tw > 1 and tw * (cs + 1) * 4 > LDS_LIMIT:
        tw >>= 1
    return tw


def pixshuf_plan(r):
    """(vec, TW, tiles per row, pixels of the last tile) the launcher decides for a pixshuf request."""
    s = r['s']
    tw = pixshuf_tw(s['cs'])
    off = dict(r['opt'].get('off', ()))
    vec = (s['W'] * s['up']) % 4 == 0 and (tw * s['up']) % 4 == 0 and off.get('tgt', 0) % 4 == 0
    ntw = (s['W'] + tw - 1) // tw
    return vec, tw, ntw, s['W'] - (ntw - 1) * tw


def wino_cot(c):
    return 48 if c > 0 and c % 48 == 0 else (32 if c > 0 and c % 32 == 0 else 0)


def layout_floats(code, Cout, Cin, taps):
    """Floats of the packed filter by the header's rules (0: the layout does not take the shape) -- what the
    *_floats queries must answer and the launches must write."""
    n_out, n_in = (Cin, Cout) if code & FP_DGRAD else (Cout, Cin)
    if n_out <= 0 or n_in <= 0 or taps <= 0:
        return 0
    if code & FP_WINO4:
        return n_out * n_in * 48 if taps == 9 and n_out % 48 == 0 and n_in % 8 == 0 and n_in >= 16 else 0
    if code & FP_WINO2:
        return n_out * n_in * 16 if taps == 9 and wino_cot(n_out) and n_in % CK == 0 else 0
    return ((n_in + CK - 1) // CK) * taps * 4 * ((n_out + 15) // 16 * 16) * 4


def unit_floats(code):
    return 48 if code & FP_WINO4 else (64 if code & FP_WINO2 else 4)


def pack_code(r):
    """(code, Cout, Cin, taps) of a single-pack request, as pack_one gets them."""
    s, name = r['s'], r['name']
    if name == 'egn_pack_conv_weight_f32':
        return (FP_DGRAD if s['dgrad'] else 0), s['Cout'], s['Cin'], s['KH'] * s['KW']
    if name == 'egn_pack_matrix_f32':
        return (FP_DGRAD, s['cin'], s['cout'], 1) if s['transpose'] else (0, s['cout'], s['cin'], 1)
    base = FP_WINO2 if name == 'egn_wino_pack_weight_f32' else FP_WINO4
    return base | (FP_DGRAD if s['dgrad'] else 0), s['Cout'], s['Cin'], 9


def query(L, r):
    """What the *_floats query of a single-pack request answers (<= 0: no layout)."""
    s, name = r['s'], r['name']
    if name == 'egn_pack_conv_weight_f32':
        return L.egn_packed_weight_floats(s['Cout'], s['Cin'], s['KH'], s['KW'], s['dgrad'])
    if name == 'egn_wino_pack_weight_f32':
        return L.egn_wino_weight_floats(s['Cout'], s['Cin'], s['dgrad'])
    if name == 'egn_wino4_pack_weight_f32':
        return L.egn_wino4_pack_weight_floats(s['Cout'], s['Cin'], s['dgrad'])
    return None


# ---------------------------------------------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------------------------------------------
class HeadRecorder(T.Recorder):
    """train_ops_sweep.Recorder over this sweep's entry points: the arguments by their names of ``ARGS``, a double
    kept as a double, the operands that were not 16-byte aligned in opt['off'] (floats into a 16-byte line)."""

    def __init__(self, handle=None, names=LAUNCHING):
        super(HeadRecorder, self).__init__(handle=handle, names=names)

    def note(self, name, args):
        super(HeadRecorder, self).note(name, args)
        n = self.notes[-1]
        types = self.sig[name][1]
        ren, s, off = {}, {}, []
        for i, ((arg, role), t) in enumerate(zip(ARGS[name], types)):
            ren['a%d' % i] = arg
            if role is None:
                s[arg] = float(args[i]) if t is C.c_double else n['s']['a%d' % i]
            elif T._addr(args[i]) & 15:
                off.append((arg, (T._addr(args[i]) & 15) // 4))
        n['s'] = s
        n['null'] = frozenset(ren[a] for a in n['null'] if a in ren)            # (the trailing stream is no operand)
        n['alias'] = tuple(sorted(tuple(sorted(ren[a] for a in g)) for g in n['alias']))
        n['opt'] = {'off': tuple(off)} if off else {}
        if name == BATCH:
            n['table_addr'] = T._addr(args[0])


def _hrnet_step(cfg, n, device, g, target=None, tw=False, steps=1, **kw):
    """As conv_sweep.hrnet_run, for the heads it has no arguments for: an explicit target, target_weight, more steps."""
    from egonet_amd.model.heatmapModel import hrnet
    from egonet_amd.train_hrnet import HRNetTrainStep
    net = hrnet.get_pose_net(cfg, is_train=False).to(device).train()
    iw, ih = cfg['heatmapModel']['input_size']
    hw, hh = cfg['heatmapModel']['heatmap_size']
    J = cfg['heatmapModel']['num_joints']
    x = torch.randn(n, 3, ih, iw, generator=g).to(device)
    tgt = (torch.rand(n, J, hh, hw, generator=g) if target is None else target).to(device)
    jxy = (torch.rand(n, J, 2, generator=g) * iw).to(device)
    weights = (torch.rand(n, J, generator=g) > 0.3).float() if tw else None
    cr = kw.pop('apply_cr_loss', False)
    tr = HRNetTrainStep(net, lr=1e-3, **kw)
    tr.apply_cr_loss = cr

    def step():
        for _ in range(steps):
            if net.head_type == 'angleregression':
                tr.step(x, tgt, update=False)
            else:
                tr.step(x, tgt, None if net.pixel_shuffle else jxy, update=False, target_weight=weights)
    return tr, step


def _tiny_pixshuf(f):
    from egonet_amd import configs
    cfg = configs.tiny_config('heatmap')
    cfg['heatmapModel']['pixel_shuffle'] = True
    cfg['heatmapModel']['heatmap_size'] = [16 * f, 16 * f]
    return cfg


def _angle(device, g):
    from egonet_amd import configs
    cfg = configs.tiny_config('angleregression', input_size=(256, 256))
    return _hrnet_step(cfg, 2, device, g, target=torch.randn(2, 2, generator=g), angle_type='mse', w_coor=0.1)


def _cr(cr_type, steps=1):
    def make(device, g):
        from egonet_amd import configs
        return _hrnet_step(configs.w48_config('coordinates'), 3, device, g, steps=steps, w_coor=0.1, w_cr=0.05,
                           cr_type=cr_type, apply_cr_loss=True)
    return make


def _bridge(device, g):
    """One backward through the autograd.py bridge of a pixel-shuffle model: the only caller of the unshuffle."""
    from egonet_amd.autograd import HRNetAutograd
    from egonet_amd.model.heatmapModel import hrnet
    cfg = _tiny_pixshuf(2)
    net = hrnet.get_pose_net(cfg, is_train=False).to(device).train()
    br = HRNetAutograd(net)
    x = torch.randn(2, 3, 64, 64, generator=g).to(device)

    def step():
        out = br(x)
        (out[0] if isinstance(out, (tuple, list)) else out).sum().backward()
    return br, step


# (where it is seen, make(device, g) -> (owner, step()); the owner of the LAST run with 'two steps' gives the table)
EXTRA_RUNS = [
    ('train-angle-tiny/b2', _angle),
    ('train-w48-cr-sl1/b3', _cr('sl1')),
    ('train-w48-cr-mse/b3 two steps', _cr('mse', steps=2)),
    ('train-pixshuf2-tiny/b2', lambda device, g: _hrnet_step(_tiny_pixshuf(2), 2, device, g, w_coor=0.0)),
    ('train-pixshuf4-tiny-tw/b2', lambda device, g: _hrnet_step(_tiny_pixshuf(4), 2, device, g, tw=True, w_coor=0.0,
                                                                 use_target_weight=True)),
    ('autograd-bridge-pixshuf2-tiny/b2', _bridge),
]
_RECORDED = {}


def read_table(packs):
    """The descriptor table of a train_common.PackedFilters, read back from the device:
    (address, n, total, [(Cout, Cin, taps, code, begin)])."""
    raw = packs.table.cpu().numpy().view(np.dtype(packs._DESC, align=True))
    return (packs.table.data_ptr(), len(raw), int(packs.total),
            [(int(d['Cout']), int(d['Cin']), int(d['taps']), int(d['code']), int(d['begin'])) for d in raw])


def recorded_requests(device='cuda'):
    """(every note, the distinct requests, the batch packer's tables [(src, n, total, rows)]) of the recorded runs;
    once per session."""
    if device in _RECORDED:
        return _RECORDED[device]
    g = torch.Generator().manual_seed(0)
    prev = os.environ.get('EGONET_AMD_AUTOTUNE')
    os.environ['EGONET_AMD_AUTOTUNE'] = '0'
    tables = []
    try:
        with HeadRecorder() as rec:
            for src, make in S.TAPE_STEPS + EXTRA_RUNS:
                rec.src = src
                first = len(rec.notes)
                tr, step = make(device, g)        # built inside: the owner keeps the proxy
                step()
                torch.cuda.synchronize()
                for n in rec.notes[first:]:
                    if n['name'] == BATCH:
                        addr, cnt, total, rows = read_table(tr.packs)
                        assert addr == n.pop('table_addr') and cnt == n['s']['n'] and total == n['s']['total']
                        tables.append((src, cnt, total, rows))
                del tr, step
    finally:
        if prev is None:
            del os.environ['EGONET_AMD_AUTOTUNE']
        else:
            os.environ['EGONET_AMD_AUTOTUNE'] = prev
    reqs = [r for r in T.merged(rec.notes) if r['name'] != BATCH]
    _RECORDED[device] = (rec.notes, reqs, tables)
    return _RECORDED[device]


# ---------------------------------------------------------------------------------------------------------------
# the edge requests
# ---------------------------------------------------------------------------------------------------------------
def _req(name, why, line=None, null=(), opt=None, **s):
    want = [a for a, role in ARGS[name] if role is None]
    assert sorted(want) == sorted(s), (name, want, sorted(s))
    types = dict(zip([a for a, _ in ARGS[name]], _lib.SIGNATURES[name][1]))
    s = {k: (float(np.float32(v)) if types[k] is C.c_float else (float(v) if types[k] is C.c_double else int(v)))
         for k, v in s.items()}
    r = dict(name=name, s=s, null=frozenset(null), alias=(), src=why, srcs=[why], opt=dict(opt or {}))
    if line is not None:
        r['line'] = line
    return r


HD, CRH, FPH, FPC, W4H = 'heads.hip', 'cross_ratio.hip', 'filter_pack.h', 'filter_pack.hip', 'wino4_pack.h'
PIX = 'egn_pixshuf_loss_f32'
UNS = 'egn_pixel_unshuffle_nchw_to_nhwc_f32'
APF, APB = 'egn_avgpool_fwd_f32', 'egn_avgpool_bwd_f32'
CRE = 'egn_cross_ratio_f32'
PCW, PMX, PW2, PW4 = PACKERS


def _pix(why, line, W, C_, up, cs=None, N=2, H=3, crit=0, weight=0.5, null=(), **opt):
    cs = cs if cs is not None else (C_ * up * up + 3) // 4 * 4
    return _req(PIX, why, (HD, line), null=null, opt=opt, N=N, H=H, W=W, C=C_, up=up, cs=cs, crit=crit, weight=weight)


def _pix_edges():
    out = []
    L_SC = 'for (int e = tid; e < tot; e += 256) {'
    L_VEC = 'for (int q = tid; q < tot / 4; q += 256) {'
    L_NPX = 'const int npx = min(TW, w - w0);'
    L_TW = 'while (TW > 1 && (size_t)TW * (cs + 1) * 4 > 65024) TW >>= 1;'
    L_PAD = 'dr[q] = make_float4(c < C ? s[0] : 0.f, c + 1 < C ? s[1] : 0.f, c + 2 < C ? s[2] : 0.f, c + 3 < C ? s[3] : 0.f);'
    L_VECP = 'const bool vec = ((W * up) % 4 == 0) && ((TW * up) % 4 == 0) && !((uintptr_t)tgt & 15);'
    L_S1 = 'for (int q = tid; q < nq; q += 256) {'
    L_CR = 'else if (ad < 1.f) { v = 0.5 * (double)d * d; gd = d; }'
    L_TWT = 'const float wj = tw ? tw[(size_t)n * J + j] : 1.f;'
    L_AT = 'if (tid == 0) atomicAdd(loss, (red[0] + red[1] + red[2] + red[3]) * inv);'
    L_ARG = 'if (N < 1 || H < 1 || W < 1 || C < 1 || up < 1 || cs % 4 || cs < C * up * up || crit < 0 || crit > 2 || !x ||'
    out.append(_pix('scalar path, one ragged tile, three pad channels in the last float4', L_SC, 5, 5, 1, cs=8))
    out.append(_pix('scalar path, two tiles, the last of 1 pixel', L_NPX, 17, 5, 1, cs=8))
    out.append(_pix('scalar path, up 2, W up = 34', L_SC, 17, 3, 2))
    out.append(_pix('vector path, last tile of 2 pixels, segw 4', L_VEC, 18, 3, 2, cs=12))
    out.append(_pix('vector path, last tile of 5 pixels', L_VEC, 21, 2, 4, cs=32))
    out.append(_pix('vector path, whole tiles only', L_VEC, 32, 3, 2, cs=12))
    out.append(_pix('vector path, one tile', L_VEC, 8, 3, 2, cs=12))
    out.append(_pix('scalar path, one whole tile', L_SC, 16, 5, 1, cs=8))
    out.append(_pix('scalar path, three tiles, ragged', L_SC, 37, 5, 1, cs=8))
    for W, C_, up, cs in ((18, 3, 2, 12), (21, 2, 4, 32)):
        out.append(_pix('vector shape, target 4 bytes into its allocation: scalar path', L_VECP, W, C_, up, cs=cs,
                        off=(('tgt', 1),)))
    out.append(_pix('whole tiles only, target 4 bytes into its allocation: scalar path', L_VECP, 32, 3, 2, cs=12,
                    off=(('tgt', 1),)))
    for cs in (1012, 1016):
        out.append(_pix('TW %d at cs %d, up 1' % (pixshuf_tw(cs), cs), L_TW, 9, 1010, 1, cs=cs))
        out.append(_pix('TW %d at cs %d, up 2' % (pixshuf_tw(cs), cs), L_TW, 18, 253, 2, cs=cs))
    for extra in (4, 8):
        out.append(_pix('cs %d floats beyond C up^2: dx pads zero, x pads never used' % extra, L_PAD, 18, 3, 2,
                        cs=12 + extra))
    out.append(_pix('stage 2 with more than one trip', L_VEC, 16, 33, 4))
    out.append(_pix('stage 1 with more than 512 float4 (and fewer than 256 in the cs 8 cases)', L_S1, 16, 33, 4,
                    cs=33 * 16 + 8))
    out.append(_pix('N 1, H 1', 'const int n = row / h, y = row - n * h;', 18, 3, 2, N=1, H=1))
    out.append(_pix('N 3, H 4', 'const int n = row / h, y = row - n * h;', 18, 3, 2, N=3, H=4))
    for crit in (0, 1, 2):
        for tw in (False, True):
            for W, up in ((17, 1), (18, 2)):
                out.append(_pix('criterion %d, tw %s, planted d = 0 and |d| = 1' % (crit, tw), L_CR, W, 3, up, crit=crit,
                                null=() if tw else ('tw',)))
            out.append(_pix('criterion %d, tw %s, exact integers' % (crit, tw), L_CR, 18, 3, 2, crit=crit,
                            null=() if tw else ('tw',), content='ints'))
    out.append(_pix('tw with zeros and one sample all zero', L_TWT, 18, 3, 2, N=3, tw='sample0'))
    out.append(_pix('dx NULL', 'if (dx) {', 18, 3, 2, null=('dx',)))
    out.append(_pix('dx NULL, l1, scalar', 'if (dx) {', 17, 3, 1, crit=1, null=('dx', 'tw')))
    out.append(_pix('loss 1.0 on entry', L_AT, 18, 3, 2, loss0=1.0))
    out.append(_pix('weight 0.1', 'const double inv = (double)weight / total;', 18, 3, 2, weight=0.1))
    out.append(_pix('weight 0.1, smooth-l1, scalar', 'const double inv = (double)weight / total;', 17, 3, 1, crit=2,
                    weight=0.1, null=('tw',)))
    # refusals
    out.append(_pix('refused: cs % 4', L_ARG, 8, 3, 2, cs=14, refuse=1))
    out.append(_pix('refused: cs < C up^2', L_ARG, 8, 4, 2, cs=12, refuse=1))
    out.append(_pix('refused: crit 3', L_ARG, 8, 3, 2, crit=3, refuse=1))
    out.append(_pix('refused: x 4 bytes off', 'if (((uintptr_t)x | (uintptr_t)dx) & 15) return EGN_E_BADARG;', 8, 3, 2,
                    off=(('x', 1),), refuse=1))
    out.append(_pix('refused: NULL loss', L_ARG, 8, 3, 2, null=('loss',), refuse=1))
    return out


def _uns(why, line, N, C_, H, W, up, extra=0, **opt):
    cs = (C_ * up * up + 3) // 4 * 4 + extra
    return _req(UNS, why, (HD, line), opt=opt, N=N, C=C_, H=H, W=W, cs=cs, up=up)


def _uns_edges():
    L_IX = 'const int j = c / uu, r = c - j * uu, a = r / up, b = r - a * up;'
    L_LOOP = 'for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {'
    out = []
    for up in (1, 2, 3, 4):
        for extra in (0, 8):
            out.append(_uns('up %d, cs %d beyond the rounding' % (up, extra), L_IX, 1 if up % 2 else 3, 3, 5, 7, up, extra))
    # N H W cs / 4 = 2 x 4096 x 256 + 77 = 2097229 = 29 x 72318.2...: 1 x 1 x 2097229 at cs 4 (C 1, up 2)
    out.append(_uns('second trip of the stride loop, ragged', L_LOOP, 1, 1, 1, 2 * HEADS_GRID + 77, 2, big=1))
    out.append(_req(UNS, 'refused: cs < C up^2', (HD, 'cs < C * up * up'), opt=dict(refuse=1), N=1, C=3, H=4, W=4, cs=8,
                    up=2))
    out.append(_req(UNS, 'refused: NULL x', (HD, 'if (!x || !y'), null=('x',), opt=dict(refuse=1), N=1, C=3, H=4, W=4,
                    cs=12, up=2))
    return out


def _pool_edges():
    out = []
    L_F = 'for (int u = 0; u < k; ++u) {'
    L_B = 'if (oy < Ho && ox < Wo) {'
    L_ACC = 'if (accumulate) {'
    L_ARG = 'N < 1 || k < 1 || H < k || W < k || cs < 4 || cs % 4'
    shapes = (('k 4 on 4 x 4 (the product\'s)', 2, 4, 4, 4), ('k 2 on 5 x 7: a cropped row and column', 2, 5, 7, 2),
              ('k 3 on 7 x 6: the divisor is no power of two', 3, 7, 6, 3), ('k 1', 1, 3, 5, 1))
    for why, N, H, W, k in shapes:
        for cs in (4, 260):
            out.append(_req(APF, '%s, cs %d' % (why, cs), (HD, L_F), N=N, H=H, W=W, cs=cs, k=k))
            for acc in (0, 1):
                out.append(_req(APB, '%s, cs %d, accumulate %d' % (why, cs, acc), (HD, L_ACC if acc else L_B), N=N, H=H,
                                W=W, cs=cs, k=k, accumulate=acc))
    out.append(_req(APF, 'integers: the sum and the quotient by 4 are exact', (HD, L_F), opt=dict(content='ints'), N=2,
                    H=5, W=7, cs=8, k=2))
    # beyond one trip of 4096 x 256 work items (forward: outputs; backward: inputs), ragged
    out.append(_req(APF, 'second trip of the stride loop', (HD, 'const size_t total = (size_t)N * Ho * Wo * cq;'),
                    opt=dict(big=1), N=1, H=2, W=2 * (HEADS_GRID + 77), cs=4, k=2))
    out.append(_req(APB, 'second trip of the stride loop', (HD, 'const size_t total = (size_t)N * H * W * cq;'),
                    opt=dict(big=1), N=1, H=3, W=HEADS_GRID // 2 + 39, cs=4, k=2, accumulate=0))
    for name in (APF, APB):
        kw = dict(accumulate=0) if name == APB else {}
        out.append(_req(name, 'refused: H < k', (HD, L_ARG), opt=dict(refuse=1), N=1, H=3, W=8, cs=4, k=4, **kw))
        out.append(_req(name, 'refused: cs 0', (HD, L_ARG), opt=dict(refuse=1), N=1, H=4, W=4, cs=0, k=2, **kw))
        for null in (('x', 'y') if name == APF else ('dy', 'dx')):
            out.append(_req(name, 'refused: NULL %s' % null, (HD, 'if (!x || !y' if name == APF else 'if (!dy || !dx'),
                            null=(null,), opt=dict(refuse=1), N=1, H=4, W=4, cs=4, k=2, **kw))
        out.append(_req(name, 'refused: a pointer 4 bytes off', (HD, '& 15))'), N=1, H=4, W=4, cs=4, k=2,
                        opt=dict(refuse=1, off=((('x' if name == APF else 'dy'), 1),)), **kw))
    return out


TC = 4.0 / 3.0


def _cre(why, line, N, K, L, idx='rand', crit=2, thres=0.15, weight=1.0, target_cr=TC, null=(), **opt):
    return _req(CRE, why, (CRH, line), null=null, opt=dict(opt, idx=idx), N=N, K=K, L=L, target_cr=target_cr,
                thres=thres, crit=crit, weight=weight)


def _cr_edges():
    out = []
    L_E = 'if (e >= N * L) return;'
    L_AP = 'for (int e = threadIdx.x; e < N * L; e += 256) {'
    L_K = 'for (int e = threadIdx.x; e < N * K; e += 256) {'
    L_G = 'if (idx[l * 4 + q] == j) {'
    L_D = 'if (d != 0.f && d < dmin) dmin = d;'
    L_KEEP = 'const bool keep = dmin != INFINITY && dmin > thres;'
    L_CNT = 'if (count == 0.0) return;'
    L_CRIT = 'const float v = cr_crit(crit, cr - 1.f, &g);'
    L_ARG = 'if (!coords || !idx || !loss || !ws || N <= 0 || K <= 0 || L <= 0 || crit < 0 || crit > 2 || target_cr == 0.0)'
    for N in (1, 3):
        for crit in (0, 1, 2):
            out.append(_cre("the product's K 33, L 12, N %d, criterion %d" % (N, crit), L_CRIT, N, 33, 12, idx='bbox12',
                            crit=crit))
    out.append(_cre('N L = 257: the second block of cr_lines_kernel', L_E, 1, 33, 257))
    out.append(_cre('N L = 600: the stride loop of cr_apply_kernel', L_AP, 3, 40, 200, crit=0))
    out.append(_cre('N K = 264 > 256', L_K, 8, 33, 12, idx='bbox12'))
    out.append(_cre('joint 0 on three lines, joint K - 1 on none', L_G, 2, 9, 5, idx='shared', thres=0.05))
    for crit in (0, 1, 2):
        out.append(_cre('a kept line with A == C (numerator 0): cr = 0, gradient 0 like the reference', L_D, 1, 8, 2,
                        idx='disjoint', crit=crit, plant='num0', thres=0.05))
    out.append(_cre('a kept line with B == C (denominator 0): not finite, like the reference', L_D, 1, 8, 2,
                    idx='disjoint', plant='den0', thres=0.05))
    out.append(_cre('four coincident points: not kept', L_KEEP, 1, 8, 2, idx='disjoint', plant='four', thres=0.05))
    out.append(_cre('smallest distance == thres (0.25): not kept', L_KEEP, 1, 8, 2, idx='disjoint', plant='thres_eq',
                    thres=0.25, edge_mask=1))
    out.append(_cre('no line kept: loss and dcoords keep their bits', L_CNT, 2, 33, 12, idx='bbox12', thres=2.0, loss0=1.5,
                    base=1))
    for crit in (0, 1, 2):
        out.append(_cre('planted cr = 1 exactly (a square of side 1/4, target 2)', L_CRIT, 1, 8, 2, idx='disjoint',
                        crit=crit, plant='cr2', thres=0.05, target_cr=2.0, exact0=1))
        if crit != 1:       # (float64 sees cr - 1 = 6e-8 against the fp32-rounded 16/9: l1's sign would be undecided)
            out.append(_cre('planted cr = 1 in fp32 (collinear 0, 1, 2, 3 eighths, target 4/3)', L_CRIT, 1, 8, 2,
                            idx='disjoint', crit=crit, plant='cr1', thres=0.05))
        out.append(_cre('planted |cr - 1| = 1 exactly (a square of side 1/4, target sqrt 2)', L_CRIT, 1, 8, 2,
                        idx='disjoint', crit=crit, plant='cr2', thres=0.05, target_cr=math.sqrt(2.0)))
    out.append(_cre('dcoords NULL', 'if (!dcoords) return;', 3, 33, 12, idx='bbox12', null=('dcoords',)))
    out.append(_cre('dcoords and loss non-zero on entry', 'dcoords[(size_t)e * 2 + 0] += (float)(gx * scale);', 3, 33, 12,
                    idx='bbox12', loss0=1.5, base=1))
    out.append(_cre('weight 0.05', 'const double scale = (double)weight / count;', 3, 33, 12, idx='bbox12', weight=0.05,
                    crit=0))
    for null in ('idx', 'ws', 'loss'):
        out.append(_cre('refused: NULL %s' % null, L_ARG, 1, 33, 12, idx='bbox12', null=(null,), refuse=1))
    out.append(_cre('refused: target_cr 0', L_ARG, 1, 33, 12, idx='bbox12', target_cr=0.0, refuse=1))
    out.append(_cre('refused: crit 3', L_ARG, 1, 33, 12, idx='bbox12', crit=3, refuse=1))
    return out


def _pack_edges():
    out = []
    L_DIR = ': d.w[(size_t)o * ld + (size_t)i * d.taps + tap];'
    L_DG = 'v[r] = dg ? d.w[(size_t)i * ld + (size_t)o * d.taps + (d.taps - 1 - tap)]'
    L_ONE = 'for (long long le = (long long)blockIdx.x * blockDim.x + threadIdx.x; le < units;'
    # direct layout: Cout x Cin x taps, both directions (a cross, not the full grid: each axis at a fixed other)
    for dg in (0, 1):
        for co in (1, 15, 16, 17, 48):
            out.append(_req(PCW, 'Cout %d' % co, (FPH, 'const int CoP = (n_out + 15) & ~15;'), Cout=co, Cin=CK + 1, KH=3,
                            KW=3, dgrad=dg))
        for ci in (1, 3, CK - 1, CK, CK + 1):
            out.append(_req(PCW, 'Cin %d' % ci, (FPH, 'const int i = chunk * EGN_CK + quad * 4 + r;'), Cout=17, Cin=ci,
                            KH=3, KW=3, dgrad=dg))
        for kh, kw in ((1, 1), (3, 3), (4, 3), (1, 7)):
            out.append(_req(PCW, 'taps %d x %d' % (kh, kw), (FPH, L_DG if dg else L_DIR), Cout=17, Cin=CK + 1, KH=kh,
                            KW=kw, dgrad=dg))
    for tr in (0, 1):
        for pitch in (0, 5):
            line = ('pack_one(src, dst, cin, cout, 1, FP_DGRAD, ld, stream)' if tr
                    else 'pack_one(src, dst, cout, cin, 1, 0, ld, stream);')
            out.append(_req(PMX, 'transpose %d, ld = row length + %d' % (tr, pitch), (FPC, line),
                            ld=(17 if tr else 35) + pitch, cout=17, cin=35, transpose=tr, opt=dict(pitch=pitch)))
    out.append(_req(PMX, 'the stride loop of pack_one_kernel: 4096 x 256 + 64 units or more', (FPC, L_ONE), ld=2064,
                    cout=2048, cin=2064, transpose=0, opt=dict(big=1)))
    for null in ('src', 'dst'):
        out.append(_req(PMX, 'refused: NULL %s' % null, (FPC, 'if (!src || !dst || cout <= 0'), null=(null,), ld=35, cout=17,
                        cin=35, transpose=0, opt=dict(refuse=1)))
    out.append(_req(PMX, 'refused: ld below the row length', (FPC, 'ld < (transpose ? cout : cin)'), ld=34, cout=17, cin=35,
                    transpose=0, opt=dict(refuse=1)))
    out.append(_req(PCW, 'refused: KH 0', (FPC, 'KH <= 0 || KW <= 0) return EGN_E_BADARG;'), Cout=16, Cin=16, KH=0, KW=3,
                    dgrad=0, opt=dict(refuse=1)))
    # F(2x2,3x3): one shape per co-tile class, two chunks, both directions, Cout != Cin
    L_W2 = 'slab[(f * 4 + quad) * cot + col] = make_float4(u[f][0], u[f][1], u[f][2], u[f][3]);'
    for dg in (0, 1):
        for n_out, n_in in ((48, 32), (96, 32), (32, 48), (64, 32)):
            co, ci = (n_in, n_out) if dg else (n_out, n_in)
            for content in ('gauss', 'ints'):
                out.append(_req(PW2, 'co-tile %d, %d output x %d input channels' % (wino_cot(n_out), n_out, n_in),
                                (FPH, L_W2), Cout=co, Cin=ci, dgrad=dg, opt=dict(content=content)))
    # F(4x4,3x3): one and two co-tiles, n_in 16 (4 k-groups) and 24, both directions (n_in 4 and 20 of the issue are
    # not shapes the layout takes: input channels % 8, >= 16 -- they are in the query grid as refusals)
    L_W4 = 'base[(size_t)wave * 768 + (p >> 2) * 256 + (p & 3)] = (float)u[b];'
    for dg in (0, 1):
        for n_out, n_in in ((48, 16), (96, 24)):
            co, ci = (n_in, n_out) if dg else (n_out, n_in)
            for content in ('gauss', 'ints'):
                line = L_W4 if content == 'gauss' else 'pad[1] = 0.f; pad[2] = 0.f; pad[3] = 0.f;'
                out.append(_req(PW4, '%d co-tiles, n_in %d' % (n_out // 48, n_in), (W4H, line), Cout=co, Cin=ci,
                                dgrad=dg, opt=dict(content=content)))
    return out


def query_grid():
    """Single-pack requests around the accepted Winograd shapes: Cout, Cin in accepted +-1, +-4, +-16; the query and
    the launch must agree on each (``layout_floats`` says what both must say)."""
    out = []
    deltas = (0, -1, 1, -4, 4, -16, 16)
    for name, centres in ((PW2, ((48, 32), (32, 16), (64, 48))), (PW4, ((48, 16), (96, 24), (48, 32), (48, 4)))):
        seen = set()
        for n_out, n_in in centres:
            for da in deltas:
                for db in deltas:
                    if da and db and abs(da) != abs(db):
                        continue
                    for dg in (0, 1):
                        a, b = n_out + da, n_in + db
                        co, ci = (b, a) if dg else (a, b)
                        if (co, ci, dg) in seen:
                            continue
                        seen.add((co, ci, dg))
                        out.append(_req(name, 'query grid', (FPH, 'inline long long fp_floats('), Cout=co, Cin=ci, dgrad=dg,
                                        opt=dict(grid=1)))
    return out


# batch tables of the edge list: (why, [(Cout, Cin, taps, code)]); ``begin`` is the running sum of the units.  Every
# layout's unit count is a multiple of 64 (direct: 4 quads x CoutP; F(2x2): n_out n_in / 4 with n_out % 32, n_in % 16;
# F(4x4): n_out n_in with n_out % 48, n_in % 8), so no begin can fall inside a wavefront; they do fall inside a block.
BATCH_EDGES = [
    ('n = 1', [(17, 17, 9, 0)]),
    ('3 descriptors, the begins at 64 and 640: inside a block', [(1, 1, 1, 0), (3, 16, 9, 1), (48, 16, 9, 4)]),
    ('7 descriptors: all three layouts, both directions; the smallest direct one has 64 units',
     [(1, 1, 1, 0), (48, 32, 9, 2), (16, 48, 9, 5), (17, 3, 12, 1), (32, 48, 9, 3), (48, 16, 9, 4), (5, 17, 7, 0)]),
    ('more than 16384 x 256 units: the second trip',
     [(2048, 2064, 1, 0), (2048, 2064, 1, 1), (2048, 2064, 1, 0), (2048, 2064, 1, 1), (17, 17, 9, 0)]),
]
BATCH_REFUSALS = ('NULL table', 'n = 0', 'total = 0')


def table_begins(rows):
    out, begin = [], 0
    for co, ci, taps, code in rows:
        fl = layout_floats(code, co, ci, taps)
        assert fl > 0, (co, ci, taps, code)
        out.append((co, ci, taps, code, begin))
        begin += fl // unit_floats(code)
    return out, begin


def edge_requests():
    return _pix_edges() + _uns_edges() + _pool_edges() + _cr_edges() + _pack_edges()


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def _gen(r):
    key = repr((r['name'], sorted(r['s'].items()), sorted(r['null']), sorted(r['opt'].items())))
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def cr_idx(r):
    s, kind = r['s'], r['opt'].get('idx', 'rand')
    K, L = s['K'], s['L']
    if kind == 'bbox12':
        from egonet_amd.common.img_proc import CR_INDICES_BBOX12
        idx = np.asarray(CR_INDICES_BBOX12, dtype=np.int32).reshape(-1, 4)
        assert idx.shape[0] == L and idx.max() < K
        return idx
    if kind == 'disjoint':
        assert K == 4 * L
        return np.arange(4 * L, dtype=np.int32).reshape(L, 4)
    rs = np.random.RandomState(zlib.crc32(repr((K, L, kind)).encode()) & 0x7fffffff)
    top = K - 1 if kind == 'shared' else K
    idx = np.stack([rs.permutation(top)[:4] for _ in range(L)]).astype(np.int32)
    if kind == 'shared':                    # joint 0 on lines 0, 1, 2 in three different places; K - 1 on none
        idx[idx == 0] = 1
        for l in range(L):
            if len(set(idx[l])) < 4:
                idx[l] = [1, 2, 3, 4]
        idx[0, 0], idx[1, 2], idx[2, 3] = 0, 0, 0
        for l in range(3):
            assert len(set(idx[l])) == 4
    return idx


_PLANTS = {      # line 0 of sample 0: (A, B, C, D)
    'num0': ((0.25, 0.25), (0.5, 0.25), (0.25, 0.25), (0.75, 0.5)),
    'den0': ((0.25, 0.25), (0.5, 0.5), (0.5, 0.5), (0.75, 0.25)),
    'four': ((0.5, 0.5),) * 4,
    'thres_eq': ((0.0, 0.5), (0.25, 0.5), (0.5, 0.5), (1.0, 0.5)),
    'cr1': ((0.125, 0.25), (0.25, 0.25), (0.375, 0.25), (0.5, 0.25)),
    'cr2': ((0.25, 0.25), (0.25, 0.5), (0.5, 0.5), (0.5, 0.25)),
}


def inputs(r):
    """The request's operands on the CPU, by argument name: inputs, and what an accumulated output holds on entry.
    fp32 unless said; NaN where the kernel must not look."""
    name, s, opt = r['name'], r['s'], r['opt']
    g = _gen(r)
    x = {}
    if name == PIX:
        N, H, W, C_, up, cs = s['N'], s['H'], s['W'], s['C'], s['up'], s['cs']
        cc = C_ * up * up
        if opt.get('content') == 'ints':
            xv = torch.randint(-4, 5, (N, H, W, cc), generator=g).float()
            t = torch.randint(-4, 5, (N, C_, H * up, W * up), generator=g).float()
            tw = torch.randint(0, 3, (N, C_), generator=g).float()
        else:
            t = torch.rand(N, C_, H * up, W * up, generator=g)
            t = torch.round(t * 64) / 64                              # dyadic: the planted differences are exact
            xv = torch.randn(N, H, W, cc, generator=g) * 1.5 + 0.3
            tw = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (N, C_), generator=g)]
            # planted: x = t (d = 0), x = t +- 1 (|d| = 1) -- exact with the dyadic tw as well
            ts = t.reshape(N, C_, H, up, W, up).permute(0, 2, 4, 1, 3, 5).reshape(N, H, W, cc)
            m = torch.rand(N, H, W, cc, generator=g)
            xv = torch.where(m < 0.05, ts, xv)
            xv = torch.where((m >= 0.05) & (m < 0.08), ts + 1.0, xv)
            xv = torch.where((m >= 0.08) & (m < 0.11), ts - 1.0, xv)
        if opt.get('tw') == 'sample0':
            tw[0] = 0.0
        full = torch.full((N, H, W, cs), NAN)
        full[..., :cc] = xv
        x['x'], x['tgt'] = full.reshape(-1), t.reshape(-1)
        if 'tw' not in r['null']:
            x['tw'] = tw.reshape(-1)
        x['loss'] = torch.tensor([opt.get('loss0', 0.0)], dtype=torch.float64)
    elif name == UNS:
        N, C_, H, W, up = s['N'], s['C'], s['H'], s['W'], s['up']
        n = N * C_ * H * up * W * up
        x['x'] = (torch.arange(n, dtype=torch.float32) % 65521.0) + 1.0          # all distinct up to 65521: a permutation shows
    elif name == APF:
        shape = (s['N'], s['H'], s['W'], s['cs'])
        x['x'] = (torch.randint(-8, 9, shape, generator=g).float() if opt.get('content') == 'ints'
                  else torch.randn(shape, generator=g) + 0.25).reshape(-1)
    elif name == APB:
        k = max(s['k'], 1)
        x['dy'] = torch.randn(s['N'] * (s['H'] // k) * (s['W'] // k) * s['cs'], generator=g)
        if s['accumulate']:
            base = torch.randn(s['N'] * s['H'] * s['W'] * s['cs'], generator=g)
            base[::7] = 0.0
            base[3::7] = -0.0
            x['dx'] = base
    elif name == CRE:
        N, K = s['N'], s['K']
        c = torch.randint(0, 1025, (N, K, 2), generator=g).float() / 1024.0
        idx = cr_idx(r)
        if opt.get('plant'):
            for q, (px, py) in enumerate(_PLANTS[opt['plant']]):
                c[0, idx[0, q], 0], c[0, idx[0, q], 1] = px, py
        x['coords'] = c.reshape(-1)
        x['idx'] = torch.from_numpy(idx.reshape(-1).copy())
        x['loss'] = torch.tensor([opt.get('loss0', 0.0)], dtype=torch.float64)
        if 'dcoords' not in r['null']:
            x['dcoords'] = (torch.randn(N * K * 2, generator=g) if opt.get('base') else torch.zeros(N * K * 2))
    elif name in (PCW, PW2, PW4):
        taps = s['KH'] * s['KW'] if name == PCW else 9
        n = max(s['Cout'], 0) * max(s['Cin'], 0) * max(taps, 0)
        if name == PCW:
            x['w'] = torch.arange(1, n + 1, dtype=torch.float32)                 # all distinct: a rotation shows
        elif opt.get('content') == 'ints':
            x['w'] = torch.randint(-8, 9, (n,), generator=g).float() * (4.0 if name == PW2 else 576.0)
        else:
            x['w'] = torch.randn(max(n, 1), generator=g)[:n] / 3.0
    elif name == PMX:
        rows, cols = (s['cin'], s['cout']) if s['transpose'] else (s['cout'], s['cin'])
        m = torch.full((rows, s['ld']), NAN)
        m[:, :cols] = (torch.arange(rows * cols, dtype=torch.float32) % 16777213.0 + 1.0).reshape(rows, cols)
        x['src'] = m.reshape(-1)
    return x


# ---------------------------------------------------------------------------------------------------------------
# references (float64) and emulations (fp32): one formula, two arithmetics
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ('pix_w0_dropped', 'pix_dy_dx_swapped', 'pix_tw_once', 'pix_sl1_at_half', 'pix_sign0_is_1', 'pix_pads_kept',
           'pool_div_before_sum', 'pool_bwd_writes_cropped', 'pack_taps_not_rotated', 'pack_channels_not_swapped',
           'pack_ld_is_row', 'w4_pads_unwritten', 'w2_cot32_as_48', 'cr_norm_by_NL', 'cr_mask_ge', 'cr_zero_not_skipped',
           'cr_gather_joint_order')
BITS_ONLY = ('cr_gather_joint_order',)
MUTANT_ENTRY = {'pix': PIX, 'pool': None, 'pack': None, 'w4': PW4, 'w2': PW2, 'cr': CRE}


def mutant_targets(mut):
    """The entry points a mutant is a wrong version of."""
    if mut.startswith('pool_bwd'):
        return (APB,)
    if mut.startswith('pool'):
        return (APF,)
    if mut == 'pack_ld_is_row':
        return (PMX,)
    if mut.startswith('pack'):
        return (PCW,)
    return (MUTANT_ENTRY[mut.split('_')[0]],)


def _res(want, A, keep=None):
    return (want.reshape(-1), A.reshape(-1), None if keep is None else keep.reshape(-1))


def _pixshuf(r, x, dt, mut):
    s = r['s']
    N, H, W, C_, f, cs = s['N'], s['H'], s['W'], s['C'], s['up'], s['cs']
    cc = C_ * f * f
    emu = dt == torch.float32
    xp = x['x'].reshape(N, H, W, cs)[..., :cc].to(dt)
    t = x['tgt'].reshape(N, C_, H * f, W * f).to(dt)
    if mut == 'pix_w0_dropped':                     # every tile reads the target of the row's first tile
        TW = pixshuf_tw(cs) * f
        col = torch.arange(W * f)
        t = t[..., col % TW]
    xs = xp.reshape(N, H, W, C_, f, f)
    xs = xs.permute(0, 3, 1, 5, 2, 4) if mut == 'pix_dy_dx_swapped' else xs.permute(0, 3, 1, 4, 2, 5)
    xs = xs.reshape(N, C_, H * f, W * f)
    has_tw = 'tw' in x
    w = x['tw'].reshape(N, C_, 1, 1).to(dt) if has_tw else torch.ones(1, 1, 1, 1, dtype=dt)
    d = (xs * w - t * w) if has_tw else (xs - t)
    total = float(N) * C_ * H * f * W * f
    inv = float(np.float32(s['weight'])) / total
    crit = s['crit']
    dd, ad = d.double(), d.double().abs()
    sgn = torch.sign(dd)
    if mut == 'pix_sign0_is_1':
        sgn = torch.where(dd == 0, torch.ones_like(dd), sgn)
    if crit == 0:
        v, gd = dd * dd, 2.0 * dd
    elif crit == 1:
        v, gd = ad, sgn
    else:
        cut = 0.5 if mut == 'pix_sl1_at_half' else 1.0
        v = torch.where(ad < cut, 0.5 * dd * dd, ad - 0.5)
        gd = torch.where(ad < cut, dd, torch.where(dd > 0, 1.0, -1.0).to(torch.float64))
    gq = gd * inv
    wd = w.double().expand_as(gq) if has_tw else None
    if emu:
        gq = gq.float()
        gout = ((gq * w) if (has_tw and mut != 'pix_tw_once') else gq).double()
    else:
        gout = gq * wd if (has_tw and mut != 'pix_tw_once') else gq
    aw = w.double().abs()
    mag = (xs.double() * w.double()).abs() + (t.double() * w.double()).abs()
    ints = r['opt'].get('content') == 'ints'
    keep = None
    if ints and not emu:                            # every d exact: float32(c'(d) inv) w, nothing to allow
        gout = (gd * inv).float().double() * (wd if has_tw else 1.0)
        A = torch.zeros_like(gout)
    elif crit == 1:
        A = torch.where(ad == 0, torch.zeros_like(gout), (inv * aw).expand_as(gout))     # d = 0 exactly: gradient 0
        keep = (ad > C_BOUND[PIX] * U * mag) | (ad == 0)
    else:
        A = (2.0 if crit == 0 else 1.0) * inv * aw * mag
    A_v = mag * mag if crit == 0 else mag
    loss0 = float(x['loss'][0])
    out = {'loss': _res(torch.tensor([loss0 + float(v.sum()) * inv], dtype=torch.float64),
                        torch.tensor([abs(loss0) + float(A_v.sum()) * inv], dtype=torch.float64))}

    def pre(tn, pad):                               # NCHW maps -> the pre-shuffle layout, pads = pad
        full = torch.full((N, H, W, cs), pad, dtype=tn.dtype)
        full[..., :cc] = tn.reshape(N, C_, H, f, W, f).permute(0, 2, 4, 1, 3, 5).reshape(N, H, W, cc)
        return full
    if 'dx' not in r['null']:
        pads = NAN if mut == 'pix_pads_kept' else 0.0
        out['dx'] = _res(pre(gout.expand(N, C_, H * f, W * f), pads), pre(A.expand(N, C_, H * f, W * f), 0.0),
                         None if keep is None else pre(keep.expand(N, C_, H * f, W * f), True))
    return out


def _unshuffle(r, x):
    s = r['s']
    N, C_, H, W, cs, up = s['N'], s['C'], s['H'], s['W'], s['cs'], s['up']
    xs = x['x'].reshape(N, C_, H * up, W * up)
    y = torch.zeros(N, H, W, cs, dtype=torch.float64)
    for j in range(C_):                              # the header's formula, index by index
        for a in range(up):
            for b in range(up):
                y[:, :, :, (j * up + a) * up + b] = xs[:, j, a::up, b::up].double()
    return {'y': _res(y, torch.zeros_like(y))}


def _pool(r, x, dt, mut):
    s = r['s']
    N, H, W, cs, k = s['N'], s['H'], s['W'], s['cs'], s['k']
    Ho, Wo = H // k, W // k
    if r['name'] == APF:
        xs = x['x'].reshape(N, H, W, cs).to(dt)
        acc, A = torch.zeros(N, Ho, Wo, cs, dtype=dt), torch.zeros(N, Ho, Wo, cs, dtype=torch.float64)
        taps = [(u, v) for u in range(k) for v in range(k)]
        div = float(k * k)
        for u, v in taps:
            tap = xs[:, u:Ho * k:k, v:Wo * k:k]
            if mut == 'pool_div_before_sum':
                if (u, v) == taps[-1] and k > 1 and (H % k or W % k):
                    continue                         # ... over a cropped window of k^2 - 1 taps
                tap = tap / div
            acc = acc + tap
            A += tap.double().abs() if mut != 'pool_div_before_sum' else 0
        y = acc if mut == 'pool_div_before_sum' else acc / div
        exact = r['opt'].get('content') == 'ints' and dt == torch.float64
        return {'y': _res(y.double(), torch.zeros_like(A) if exact else A / div)}
    dy = x['dy'].reshape(N, Ho, Wo, cs).to(dt)
    gq = dy / float(k * k)
    dx = torch.zeros(N, H, W, cs, dtype=dt)
    A = torch.zeros(N, H, W, cs, dtype=torch.float64)
    up = gq.repeat_interleave(k, 1).repeat_interleave(k, 2)
    dx[:, :Ho * k, :Wo * k] = up
    if mut == 'pool_bwd_writes_cropped' and (H % k or W % k):
        dx[:, Ho * k:] = dx[:, Ho * k - 1:Ho * k]
        dx[:, :, Wo * k:] = dx[:, :, Wo * k - 1:Wo * k]
    pow2 = k & (k - 1) == 0
    if not pow2 or s['accumulate']:
        A[:, :Ho * k, :Wo * k] = up.double().abs()
    if s['accumulate']:
        base = x['dx'].reshape(N, H, W, cs).to(dt)
        A = torch.where(dx == 0, torch.zeros_like(A), A + base.double().abs())    # (0 added: the base's value)
        dx = base + dx
    return {'dx': _res(dx.double(), A)}


def _crit(crit, xx, dt):
    ax = xx.abs()
    if crit == 0:
        return xx * xx, 2.0 * xx
    if crit == 1:
        return ax, torch.sign(xx)
    one = torch.ones_like(xx)
    return (torch.where(ax < 1, 0.5 * xx * xx, ax - 0.5), torch.where(ax < 1, xx, torch.where(xx > 0, one, -one)))


def _cross_ratio(r, x, dt, mut):
    """ws [N L, 10], dcoords, loss; '_undecided' when a line's mask hangs on the rounding of its smallest distance."""
    s = r['s']
    N, K, L, crit = s['N'], s['K'], s['L'], s['crit']
    idx = x['idx'].reshape(L, 4).long()
    c = x['coords'].reshape(N, K, 2).to(dt)
    p = c[:, idx]                                    # [N, L, 4, 2]
    thres = float(np.float32(s['thres']))
    tsq = float(np.float32(s['target_cr'] * s['target_cr']))

    def len2(a, b):
        dxy = p[:, :, b] - p[:, :, a]
        return dxy[..., 0] * dxy[..., 0] + dxy[..., 1] * dxy[..., 1], dxy
    inf = torch.full((N, L), float('inf'), dtype=dt)
    dmin = inf.clone()
    for a in range(4):
        for b in range(a + 1, 4):
            dist = torch.sqrt(len2(a, b)[0])
            ok = (dist < dmin) if mut == 'cr_zero_not_skipped' else ((dist != 0) & (dist < dmin))
            dmin = torch.where(ok, dist, dmin)
    keep = (dmin != inf) & ((dmin >= thres) if mut == 'cr_mask_ge' else (dmin > thres))
    gap = (dmin.double() - thres).abs()          # (0: a planted distance, exact in fp32 -- decided)
    undecided = bool(((dmin != inf) & (gap > 0) & (gap <= 4 * U * dmin.double())).any())
    (ac, acd), (bd, bdd), (bc, bcd), (ad, add) = len2(0, 2), len2(1, 3), len2(1, 2), len2(0, 3)
    cr = ((ac * bd) / (bc * ad)) / tsq
    xx = cr - 1.0
    v, gg = _crit(crit, xx, dt)
    zero = torch.zeros_like(cr)
    gac = torch.where(ac != 0, 2.0 * gg * cr / ac, zero)
    gbd = torch.where(bd != 0, 2.0 * gg * cr / bd, zero)
    gbc, gad = -2.0 * gg * cr / bc, -2.0 * gg * cr / ad
    e = lambda q, dxy: q.unsqueeze(-1) * dxy                                     # noqa: E731
    pts = [-e(gac, acd) - e(gad, add), -e(gbd, bdd) - e(gbc, bcd), e(gac, acd) + e(gbc, bcd), e(gbd, bdd) + e(gad, add)]
    ws = torch.cat(pts + [v.unsqueeze(-1), torch.ones(N, L, 1, dtype=dt)], dim=-1)            # [N, L, 10]
    ws = torch.where(keep.unsqueeze(-1), ws, torch.zeros_like(ws))
    # the allowance, float64 on absolute values (docstring)
    crd, xd, gd_ = cr.double().abs(), xx.double().abs(), gg.double().abs()
    A_x = crd + xd
    A_g = {0: 2.0 * A_x, 1: torch.zeros_like(A_x), 2: A_x}[crit]
    A_v = A_x if crit == 1 else gd_ * A_x + U * C_BOUND[CRE] * A_x * A_x          # (second order where c'(x) = 0)

    def A_q(l2):
        return 2.0 * (A_g * crd + gd_ * crd) / l2.double()
    ab = lambda q, dxy: q.unsqueeze(-1) * dxy.double().abs()                     # noqa: E731
    qa, qb, qc, qd = A_q(ac), A_q(bd), A_q(bc), A_q(ad)
    A_pts = [ab(qa, acd) + ab(qd, add), ab(qb, bdd) + ab(qc, bcd), ab(qa, acd) + ab(qc, bcd), ab(qb, bdd) + ab(qd, add)]
    A_ws = torch.cat(A_pts + [A_v.unsqueeze(-1), torch.zeros(N, L, 1, dtype=torch.float64)], dim=-1)
    A_ws = torch.where(keep.unsqueeze(-1) & torch.isfinite(A_ws), A_ws, torch.zeros_like(A_ws))
    if r['opt'].get('exact0'):         # cr = 1 exactly in both arithmetics (CPU test): the line's nine values are exactly 0
        A_ws[0, 0] = 0.0
    # l1: the sign of x decides g; |x64| inside the allowance of x leaves the line's gradient undecided
    if crit == 1 and bool((keep & (xd <= C_BOUND[CRE] * U * A_x) & (xd > 0)).any()):
        undecided = True
    out = {'ws': _res(ws.double(), A_ws), '_undecided': undecided, '_kept': int(keep.sum())}
    count = float(keep.sum())
    if mut == 'cr_norm_by_NL':
        count = float(N * L)
    loss0 = float(x['loss'][0])
    if count == 0:
        out['loss'] = _res(torch.tensor([loss0], dtype=torch.float64), torch.zeros(1, dtype=torch.float64))
        if 'dcoords' in x:
            base = x['dcoords'].double()
            out['dcoords'] = _res(base, torch.zeros_like(base))
        return out
    scale = float(np.float32(s['weight'])) / count
    out['loss'] = _res(torch.tensor([loss0 + float(ws[..., 8].double().sum()) * scale], dtype=torch.float64),
                       torch.tensor([abs(loss0) + float(A_ws[..., 8].sum()) * scale], dtype=torch.float64))
    if 'dcoords' in x:
        g = torch.zeros(N, K, 2, dtype=dt)
        Ag = torch.zeros(N, K, 2, dtype=torch.float64)
        order = [(l, q) for l in range(L) for q in range(4)]
        if mut == 'cr_gather_joint_order':
            order = [(l, q) for q in range(4) for l in reversed(range(L))]
        for l, q in order:                           # line order, as the kernel gathers (no atomics)
            j = int(idx[l, q])
            g[:, j] = g[:, j] + ws[:, l, 2 * q:2 * q + 2]
            Ag[:, j] += A_ws[:, l, 2 * q:2 * q + 2]
        base = x['dcoords'].reshape(N, K, 2)
        add = (g.double() * scale)
        if dt == torch.float32:
            add = add.float()
            want = (base + add).double()
        else:
            want = base.double() + add
        out['dcoords'] = _res(want, base.double().abs() + Ag * scale)
    return out


def effective_filter(w, Cout, Cin, taps, dgrad, mut=None):
    """[n_out, n_in, taps] the packed filter holds: the weight itself, or for the data gradient in / out channels
    swapped and the taps rotated by 180 degrees."""
    w3 = w.reshape(Cout, Cin, taps)
    if not dgrad:
        return w3
    if mut != 'pack_taps_not_rotated':
        w3 = w3.flip(2)
    if mut == 'pack_channels_not_swapped':
        return w3.reshape(Cin, Cout, taps) if Cin != Cout else w3
    return w3.permute(1, 0, 2)


def direct_layout(eff):
    """include/egonet_hip.h: [nchunk][taps][CK / 4][CoutP][4], ci = chunk CK + quad 4 + r, zero padded -- written as
    the index of every element, not as a permutation."""
    n_out, n_in, taps = eff.shape
    cop, nch = (n_out + 15) // 16 * 16, (n_in + CK - 1) // CK
    dst = torch.zeros(nch * taps * 4 * cop * 4, dtype=eff.dtype)
    o, i, t = torch.meshgrid(torch.arange(n_out), torch.arange(n_in), torch.arange(taps), indexing='ij')
    at = ((((i // CK) * taps + t) * 4 + (i % CK) // 4) * cop + o) * 4 + i % 4
    dst[at.reshape(-1)] = eff.reshape(-1)
    return dst


def wino_u(eff, four):
    """U = G g G^T in float64: [n_out, n_in, 4, 4] or [.., 6, 6]."""
    G = (torch.tensor([[1 / 4., 0., 0.], [-1 / 6., -1 / 6., -1 / 6.], [-1 / 6., 1 / 6., -1 / 6.],
                       [1 / 24., 1 / 12., 1 / 6.], [1 / 24., -1 / 12., 1 / 6.], [0., 0., 1.]], dtype=torch.float64)
         if four else torch.tensor([[1., 0., 0.], [.5, .5, .5], [.5, -.5, .5], [0., 0., 1.]], dtype=torch.float64))
    g = eff.double().reshape(eff.shape[0], eff.shape[1], 3, 3)
    return torch.einsum('ia,ocab,jb->ocij', G, g, G)


def wino2_layout(u, mut=None):
    """[Cout / T][Cin / 16][f = 4i + j][quad][T][4], T = 48 if Cout % 48 == 0 else 32 (include/egonet_hip.h)."""
    n_out, n_in = u.shape[:2]
    cot = wino_cot(n_out)
    if mut == 'w2_cot32_as_48' and cot == 32 and n_out % 48 == 0:
        cot = 48
    elif mut == 'w2_cot32_as_48' and cot == 32:
        cot = 16                                     # (a wrong tile at a width 48 does not divide)
    nch = n_in // CK
    dst = torch.zeros(n_out * n_in * 16, dtype=torch.float64)
    o, i, f = torch.meshgrid(torch.arange(n_out), torch.arange(n_in), torch.arange(16), indexing='ij')
    at = (((((o // cot) * nch + i // CK) * 16 + f) * 4 + (i % CK) // 4) * cot + o % cot) * 4 + i % 4
    dst[at.reshape(-1)] = u.reshape(n_out, n_in, 16).reshape(-1)
    return dst


def wino4_layout(u, mut=None):
    """[Cout / 48][k-group Cin / 4][wave 12][3][64 lanes][4]: value p = 4 q + r = 3 pl + nt (< 9; the rest padding) of
    lane 16 kq + li is point 3 wave + pl of co = 48 ct + 16 nt + li, ci = 4 group + kq (include/egonet_hip.h,
    filters.pack_wino4_weight).  -> (floats, written mask)."""
    n_out, n_in = u.shape[:2]
    dst = torch.full((n_out * n_in * 48,), NAN if mut == 'w4_pads_unwritten' else 0.0, dtype=torch.float64)
    o, i, pt = torch.meshgrid(torch.arange(n_out), torch.arange(n_in), torch.arange(36), indexing='ij')
    ct, nt, li = o // 48, (o % 48) // 16, o % 16
    p = 3 * (pt % 3) + nt
    at = ((((ct * (n_in // 4) + i // 4) * 12 + pt // 3) * 3 + p // 4) * 64 + 16 * (i % 4) + li) * 4 + p % 4
    dst[at.reshape(-1)] = u.reshape(n_out, n_in, 36).reshape(-1)
    return dst


def pack_ref(r, x, mut=None):
    """The packed filter of a single-pack request in float64 and its allowance."""
    code, Cout, Cin, taps = pack_code(r)
    dg = code & FP_DGRAD
    if r['name'] == PMX:
        s = r['s']
        rows, cols = (s['cin'], s['cout']) if s['transpose'] else (s['cout'], s['cin'])
        m = x['src'].reshape(rows, s['ld'])
        if mut == 'pack_ld_is_row' and s['ld'] > cols:
            m = x['src'][:rows * cols].reshape(rows, cols)
        m = m[:, :cols]
        eff = (m.t() if s['transpose'] else m).reshape(s['cout'], s['cin'], 1)
        want = direct_layout(eff).double()
        return {'dst': _res(want, torch.zeros_like(want))}
    eff = effective_filter(x['w'], Cout, Cin, taps, dg, mut)
    if code & (FP_WINO2 | FP_WINO4):
        four = bool(code & FP_WINO4)
        u = wino_u(eff, four)
        want = wino4_layout(u, mut) if four else wino2_layout(u, mut)
        if r['opt'].get('content') == 'ints':
            # G g G^T is an integer here.  The einsum multiplies by float64's 1 / 6 and leaves 2^-53 of noise on it (1e-14
            # where the true value is 0); the kernel DIVIDES by 4, 6, 12, 24, every quotient exact: it must give the integer.
            assert float(torch.nan_to_num(want - want.round()).abs().max()) < 1e-9
            want, A = want.round(), torch.zeros_like(want)
        else:
            A = want.abs()
        return {'dst': _res(want, torch.where(torch.isfinite(A), A, torch.zeros_like(A)))}
    want = direct_layout(eff).double()
    return {'dst': _res(want, torch.zeros_like(want))}


def host_pack(r, x):
    """The independent statement of a layout: the host packers of filters.py on the effective filter (fp32)."""
    code, Cout, Cin, taps = pack_code(r)
    if r['name'] == PMX:
        s = r['s']
        rows, cols = (s['cin'], s['cout']) if s['transpose'] else (s['cout'], s['cin'])
        m = x['src'].reshape(rows, s['ld'])[:, :cols]
        return filters.pack_conv_weight((m.t() if s['transpose'] else m).reshape(s['cout'], s['cin'], 1, 1))
    eff = effective_filter(x['w'], Cout, Cin, taps, code & FP_DGRAD).contiguous()
    if code & FP_WINO4:
        return filters.pack_wino4_weight(eff.reshape(eff.shape[0], eff.shape[1], 3, 3))
    if code & FP_WINO2:
        return filters.pack_wino_weight(eff.reshape(eff.shape[0], eff.shape[1], 3, 3))
    return filters.pack_conv_weight(eff.reshape(eff.shape[0], eff.shape[1], taps, 1))


def _compute(r, x, dt, mut=None):
    name = r['name']
    if name == PIX:
        return _pixshuf(r, x, dt, mut)
    if name == UNS:
        return _unshuffle(r, x)
    if name in (APF, APB):
        return _pool(r, x, dt, mut)
    if name == CRE:
        return _cross_ratio(r, x, dt, mut)
    if name in PACKERS:
        out = pack_ref(r, x, mut)
        if dt == torch.float32 and name in (PW2, PW4):           # U rounded once, as the header says
            w, A, k = out['dst']
            out['dst'] = (w.float().double(), A, k)
        return out
    raise ValueError(name)


def reference(r, x, mut=None):
    """{output: (want float64, A, keep mask or None)} (+ '_undecided', '_kept' for the cross-ratio)."""
    return _compute(r, x, torch.float64, mut)


def emulate(r, x, mut=None):
    """The header's arithmetic in fp32 (torch on the CPU): {output: value as float64}."""
    return {k: (v[0] if isinstance(v, tuple) else v) for k, v in _compute(r, x, torch.float32, mut).items()}


def outputs(r):
    """The checked outputs of a request (the cross-ratio's workspace is one: its ten floats per line are defined)."""
    return [a for a, role in ARGS[r['name']] if role in ('out', 'io', 'ws') and a not in r['null']]


def check(r, got, ref, scale=1.0):
    """({output: worst |err| / (U A)}, [failures], share of elements left out) of ``got`` {output: tensor} against
    ``ref``; an element with A = 0 must be exact, one float64 has no finite value for must not be finite."""
    worst, fails, left = {}, [], 0.0
    C_ = C_BOUND[r['name']] * scale
    for a in outputs(r):
        if a not in ref:
            continue
        want, A, keep = ref[a]
        g = got[a].reshape(-1).double()
        if g.numel() != want.numel():
            fails.append('%s: %d elements, want %d' % (a, g.numel(), want.numel()))
            continue
        fin = torch.isfinite(want)
        if bool((torch.isfinite(g) & ~fin).any()):
            fails.append('%s: finite where float64 is not' % a)
        use = fin if keep is None else (fin & keep)
        if keep is not None:
            left = max(left, 1.0 - float(keep.double().mean()))
        if bool((~torch.isfinite(g) & fin).any()):
            fails.append('%s: %d elements not written / not finite' % (a, int((~torch.isfinite(g) & fin).sum())))
            continue
        ra = S.ratio(g[use], want[use], A[use]) if bool(use.any()) else torch.zeros(1, dtype=torch.float64)
        w = float(ra.max())
        worst[a] = w
        if not w <= C_:
            k = int(ra.argmax())
            fails.append('%s: error %.3g x 2^-24 A > %g (got %r, want %r)' % (a, w, C_, float(g[use][k]),
                                                                               float(want[use][k])))
    return worst, fails, left
