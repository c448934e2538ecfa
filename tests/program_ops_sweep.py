"""The ops of an inference program that are not convolutions -- 'pwpair' (csrc/conv_pw.hip), 'decode' (csrc/decode.hip,
decode_map.h), 'fuse', 'to_nhwc', 'to_nchw', 'pixshuf', 'ramps' (csrc/elementwise.hip) -- as the product records them,
the edges of their kernels and launchers, the inputs and the element-wise checks of the sweep.

Helper module of tests/test_program_ops_sweep_cpu.py and tests/test_gpu_program_ops_sweep.py (imported, not a
conftest).  Fifth of the family of tests/conv_sweep.py, tests/wgrad_sweep.py, tests/train_ops_sweep.py and
tests/gemm_sweep.py: conv_sweep._program_requests keeps the 'conv' ops of a recording and skips the rest; this module
keeps the rest.  ``OWNERS`` says, for every op kind engine._Recorder can push, which test file holds it to float64.

A request is a dict: 'kind', the scalar arguments Program._emit passes for that kind, 'null' (the pointer arguments
that are NULL), 'lead' (floats in front of operands that start inside their allocation), 'srcs' (where it was seen:
model / batch / decode mode / tag of a recording, or the reason of an edge request) and, on an edge request, 'line':
(file, text) of the kernel line it is there for, at the smallest shape that reaches it.
  pwpair   M, res, fused, relu1          decode   N, K, H, W, mode, idx, content
  fuse     N, H, W, C, cs, shifts, relu  to_nhwc / to_nchw   N, C, H, W, cs
  pixshuf  N, C, H, W, cs, up            ramps    N, H, W, cs, c0
``recorded_requests`` walks conv_sweep.INFERENCE_MODELS at their batch sizes with every decode mode (None, 0, 1, 2:
HRNetEngine hands the mode to egn_program_add_decode unchanged, which takes 0 .. 2) on the host; ``edge_requests(G)``
is the hand-written list, G = 2 x the device's CU count (the grid cap of conv_pw.hip).  A recorded 'pwpair' above
M = 32 (4 G + 3) is replayed at that M: nothing in the kernel depends on M except the tile count against the grid,
and at 4 G + 3 tiles every block has gone round four times and three of them a fifth.

Every launch (tests/test_gpu_program_ops_sweep.py) has its outputs between guard bands, pre-filled with NaN (a
sentinel where only part is written: 'ramps'), its inputs compared bit for bit afterwards, NaN in the input pad the
kernel must not read (channels >= C of the NHWC input of 'to_nchw', >= C up^2 of 'pixshuf'; 64 floats behind every
input), and is made twice: the second gives the same bits.  Every distinct recorded request runs once more as a
one-op program inside a fork / join on lane 1 and gives the bits of the direct entry point, one launch counted.

THE CHECKS.  U = 2^-24.
pwpair, two input sets (gemm_sweep.CASES):
  exact     h, res, both folded filters, both shifts integers in [-4, 4]: |out| <= 64 x 16 + 8, the second product's
            absolute sums <= 256 x 1032 x 4 + 4 < 2^24 (asserted on the reference): out and hn equal float64 bit for bit;
  rounding  h = conv_sweep.act_like, res and shifts Gaussian, filters conv_sweep.filt times gemm_sweep.column_scale
            (2^0 .. 2^-10 in blocks of 16 output channels):  |out - out64| <= C_PW U A,  A = |h||w3'|^T + |shift3| +
            |res|;  hn against float64 ON THE KERNEL'S STORED out (only the second product is judged),
            A = |out||w1'|^T + |shift1|.  ReLU is 1-Lipschitz: no element is left out.
  C_PW = 20 = gemm_sweep.CG[0], reused: ``emulate`` (the kernel's k order: chunk c, then s, an MFMA step the four
  k = 16 c + 4 kq + s, their product-sum formed in a double and rounded once, fp32 epilogue) measures on the rounding
  inputs of the edge list (first 2048 rows; tests/test_program_ops_sweep_cpu.py prints the table):
      out  4.10  (M = 64, first product alone, no residual, no ReLU)      hn  2.60  (M = 64, fused, residual, ReLU)
  gemm_sweep's emulation has 4.90 at K = 64; about 4x for the order in which v_mfma_f32_16x16x4_f32 adds its four
  products, which the emulation cannot know.  The constant never comes from the kernel's output.
decode: index and maximum equal numpy's on the same fp32 map in every mode; mode 0's xy exactly (idx % W, idx // W),
  zero where max <= 0.  Modes 1 (softmax) and 2 (map / sum) against float64 of the same formula, per coordinate
      |x - x64| <= C_DEC U (sum|p_i| x_i + |x64| sum|w_i| / |sum w_i|)  +  2 sum p_i d_i |x_i - x64|  (+ 2^-126 terms)
  the first part for a quotient of fp32 sums, C_DEC = 11 about 4x the worst ratio of ``emulate`` (64 strided per-lane
  partials with fused multiply-adds, the xor butterfly, on the register and the scalar path, correctly rounded exp) on
  the edge list: 2.63 in mode 1 (2 maps of 64 x 64, 'peaks'), 1.46 in mode 2 (2 maps of 32 x 128, 'peaks'); the
  second (mode 1 only) for a relative error d_i of weight i, to first order.  d_i: the HIP math API's accuracy
  table (the one train_ops_sweep.py cites for sqrtf and division) is not in this tree and could not be consulted
  for __expf, so d_i is derived from the instruction: the compiler lowers __expf(x) for gfx950 to
  v_exp_f32(v_mul_f32(x, 0x3fb8aa3b)) (read from its assembly).  The CDNA ISA guide gives v_exp_f32 1 ulp: 2 U
  relative, results below 2^-126 flushed (the absolute 2^-126 term).  The argument t of 2^t carries three relative
  errors: x = v_i - max rounds once (U), the constant is log2(e) (1 - 0.23 U), the product rounds once (U); an
  error e |t| on t is e |t| ln 2 = e |x| relative on 2^t.  So  d_i = (2 + 2.25 |v_i - max|) U, argument included.
  Mode 2's inputs are non-negative (sigmoid-like); one mixed-sign content with sum|v| / |sum v| <= 8 (asserted).
  Where float64 gives no number (mode 2 of a map with -inf entries, mode 1 of an all -inf map) the kernel must not
  either.  Maps with some NaN are out of scope: numpy's arg-max and the kernel differ there by design (numpy returns
  the first NaN, the kernel skips it).
  The allowance on the 64 x 64 'peaks' maps is 8.5e-5 pixels (mode 1) and 4.2e-5 (mode 2), on the 128 x 128 maps of
  the pixel-shuffle head up to 3.5e-4 (it grows with the coordinate: U x 11 x 2 x 128 alone is 1.7e-4);
  tests/test_gpu_decode.py allows 1e-3 / 1e-4 on 64 x 64 maps.
fuse: exact (integers) bit for bit; rounding |y - y64| <= nterms U A, A = sum|terms|: nterms - 1 left-to-right
  additions of at most U of the running sum each, plus 1 for second order.  Derived, not measured.
to_nhwc, to_nchw, pixshuf, ramps: bit for bit against the index formula / np.linspace(0, 1, n).astype(float32).

``MUTANTS``: wrong kernels applied to the emulations; each is flagged by ``check`` on the edge inputs (CPU test).

Measured on the MI355X (tests/test_gpu_program_ops_sweep.py: requests, launches, worst |err| / (U A) over every
element of every launch; 'to_nhwc', 'to_nchw', 'pixshuf', 'ramps' are bit for bit and have no ratio):
  kind      recorded                                               edge
  pwpair    21 requests 105 launches  7.88  (M 256, first product   21 requests  84 launches  7.74  (M 32 (G + 1), residual,
            alone: tiny/b1 layer1.0.downsample)                    ReLU, first product alone)
  fuse      78 requests 390 launches  2.92 of 4  (70 x 64 x 64 x   11 requests  44 launches  2.41 of 4  (2 x 8 x 16, 18 in
            48, shifts (0, 1, 2, 3))                               20, shifts (0, 1, 2, 3))
  decode    36 requests 108 launches  5.79  (3 x 33 maps of 128 x  255 requests 510 launches  2.10  (1 map of 128 x 128,
            128, mode 1)                                           mode 1)
  to_nhwc 8 + 11, to_nchw 8 + 11, pixshuf 4 + 7, ramps 8 + 11 requests: every bit.
Three of these sit above a third of their constant.
  pwpair 7.88 of 20: ``emulate`` rounds an MFMA step once (4.10); the same chain with every one of the four products
  rounded on its own -- the other way the instruction may add them -- measures 8.27 on the same inputs (CPU).  The
  kernel lies between the two models, where the 4x was put for; and the GPU looks at 16.8 M elements per launch at the
  largest M, the emulation at 0.5 M.
  decode 5.79 of 11: the emulation itself gives 5.79 on that request (99 peaked maps of 128 x 128 on the scalar path,
  256 sequential terms per lane), and 2.72 on the 256 x 256 maps in mode 2; the kernel follows the emulated order to
  the figure.  The constant was set on the edge list (2 maps per shape) before the recorded shapes were emulated and
  is left there: the margin on the recorded maps is 1.9x, not 4x, and the order is known.
  fuse 2.92 of 4: its constant is the derived worst case, not 4x a measurement: three additions of up to U of a
  running sum that A bounds can reach 3, and among 13.8 M elements with spikes some nearly do.
"""
import ctypes
import math
import os
import re
import zlib

import numpy as np
import torch

import conv_sweep as S
import gemm_sweep as GS
from egonet_amd import _lib, engine

U = S.U
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, 'egonet_amd', 'csrc')

KINDS = ('pwpair', 'fuse', 'to_nhwc', 'to_nchw', 'pixshuf', 'ramps', 'decode')
GPU_TEST = 'test_gpu_program_ops_sweep.py'
OWNERS = dict({'conv': 'test_gpu_conv_sweep.py', 'convh': 'test_gpu_conv_h.py', 'convh2': 'test_gpu_conv_h2.py',
               'convhx': 'test_gpu_conv_hx.py', 'convpair': 'test_gpu_conv_pair.py'}, **{k: GPU_TEST for k in KINDS})
DECODE_MODES = (None, 0, 1, 2)
PRECISIONS = ('f32', 'f16', 'f16s2', 'f16x')
CASES = GS.CASES

C_PW = GS.CG[0]
C_DEC = 11.0
TINY = 2.0 ** -126
NOMINAL_G = 512                  # 2 x 256 CUs: what the CPU tests build the edge list with
GRID_CAP = 2048 * 256            # threads of one trip of an elementwise kernel's grid-stride loop
SENTINEL = -7777.0               # what a partly written output holds before the launch
EMU_ROWS = 2048                  # rows of a pwpair request the CPU emulation runs


def kernel_text(name):
    with open(os.path.join(_CSRC, name)) as fh:
        return fh.read()


def pushed_kinds():
    """Every kind engine._Recorder._push is called with, from engine.py's text."""
    with open(os.path.join(_ROOT, 'egonet_amd', 'engine.py')) as fh:
        return set(re.findall(r"self\._push\('(\w+)'", fh.read()))


# ---------------------------------------------------------------------------------------------------------------
# requests
# ---------------------------------------------------------------------------------------------------------------
def req_key(r):
    return tuple(sorted((k, v) for k, v in r.items() if k not in ('srcs', 'line')))


def _req(kind, why, line=None, null=(), lead=0, **s):
    r = dict(s, kind=kind, null=tuple(sorted(null)), lead=lead, srcs=[why])
    if line is not None:
        r['line'] = line
    return r


def pw_clamp(G):
    return 32 * (4 * G + 3)


def from_op(kind, op, src):
    """A recorded op as a request (the scalars Program._emit passes, the NULL pointers)."""
    if kind == 'pwpair':
        null = ([] if op['res'] is not None else ['res']) + ([] if op['hn'] is not None else ['w1', 'shift1', 'hn'])
        return _req(kind, src, null=null, M=op['m'], res=op['res'] is not None, fused=op['hn'] is not None,
                    relu1=op['relu1'])
    if kind == 'fuse':
        y = op['y']
        return _req(kind, src, N=y.n, H=y.h, W=y.w, C=y.c, cs=y.cs, shifts=tuple(s for _, s in op['terms']),
                    relu=op['relu'])
    if kind == 'to_nhwc':
        y = op['y']
        return _req(kind, src, N=y.n, C=y.c, H=y.h, W=y.w, cs=y.cs)
    if kind == 'to_nchw':
        x = op['x']
        return _req(kind, src, N=x.n, C=op['c'], H=x.h, W=x.w, cs=x.cs)
    if kind == 'pixshuf':
        x = op['x']
        return _req(kind, src, N=x.n, C=op['c'], H=x.h, W=x.w, cs=x.cs, up=op['up'])
    if kind == 'ramps':
        y = op['y']
        return _req(kind, src, N=y.n, H=y.h, W=y.w, cs=y.cs, c0=op['c0'])
    if kind == 'decode':
        null = [k for k in ('xy', 'mx', 'idx') if op[k].slot < 0]
        return _req(kind, src, null=null, N=op['n'], K=op['k'], H=op['h'], W=op['w'], mode=op['mode'],
                    idx='idx' not in null, content='peaks')
    raise ValueError(kind)


def merged(reqs):
    seen, out = {}, []
    for r in reqs:
        k = req_key(r)
        if k in seen:
            seen[k]['srcs'] += r['srcs']
            continue
        seen[k] = dict(r, srcs=list(r['srcs']))
        out.append(seen[k])
    return out


_RECORDED = {}


def recorded_kinds(precision='f32', modes=DECODE_MODES):
    """(every (kind, op, src) of the recordings, the set of kinds) of conv_sweep.INFERENCE_MODELS at their batch sizes,
    host only."""
    key = (precision, tuple(modes))
    if key in _RECORDED:
        return _RECORDED[key]
    from egonet_amd.model.heatmapModel import hrnet
    ops, kinds = [], set()
    with torch.no_grad():
        for name, mk, batches in S.INFERENCE_MODELS:
            cfg = mk()
            net = hrnet.get_pose_net(cfg, is_train=False).eval()
            if precision != 'f32':
                net.precision = precision
            eng = engine.HRNetEngine(net)
            assert eng.precision == precision
            iw, ih = cfg['heatmapModel']['input_size']
            for n in batches:
                for mode in modes:
                    rec, _, _ = eng._record(n, 3, ih, iw, mode)
                    for kind, op in rec.ops:
                        kinds.add(kind)
                        if kind in KINDS:
                            ops.append((kind, op, '%s/b%d/decode %s:%s' % (name, n, mode, op.get('tag', ''))))
            del net, eng
    _RECORDED[key] = (ops, kinds)
    return _RECORDED[key]


def recorded_requests():
    """The distinct requests of the seven kinds in the f32 recordings."""
    ops, _ = recorded_kinds()
    return merged([from_op(kind, op, src) for kind, op, src in ops])


def replayed(r, G):
    """The request as the sweep launches it: a 'pwpair' above 32 (4 G + 3) rows at that many."""
    if r['kind'] == 'pwpair' and r['M'] > pw_clamp(G):
        return dict(r, M=pw_clamp(G))
    return r


PW = 'conv_pw.hip'
DM = 'decode_map.h'
EW = 'elementwise.hip'
PW_FORMS = ((False, False, 0), (True, True, 1), (False, True, 1))     # (fused, res, relu1) the product records
DECODE_SHAPES = (
    ((1, 1, 1, 1), 0, (DM, 'for (int i = lane; i < hw; i += 64) {'), 'one element'),
    ((3, 5, 5, 7), 0, ('decode.hip', 'if (map >= nmaps) return;'), 'hw = 35: scalar path; 15 maps: ragged last block'),
    ((2, 3, 4, 4), 0, (DM, 'reg[j] = q < nvec ? p4[q] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);'),
     'register path with 60 idle lanes'),
    ((1, 2, 64, 64), 0, (DM, 'constexpr int VMAX = 16;'), 'exactly 4096: every register used'),
    ((1, 2, 32, 128), 0, (DM, 'const int y = (i0 + c) / W;'), '4096 elements, wide: the i / W split'),
    ((1, 2, 128, 32), 0, (DM, 'const int x = (i0 + c) - y * W;'), '4096 elements, tall: the i / W split'),
    ((1, 2, 64, 65), 0, (DM, 'const bool vec = (hw & 3) == 0 && hw <= 64 * VMAX * 4'), 'hw % 4 == 0 but > 4096: scalar'),
    ((1, 1, 128, 128), 0, (DM, 'const int y = i / W;'), "the pixel-shuffle head's maps"),
    ((1, 3, 6, 6), 1, (DM, '((reinterpret_cast<size_t>(p) & 15) == 0)'), 'base one float into its allocation: scalar'),
)
CONTENTS = ('peaks', 'ties_lanes', 'ties_quad', 'all_equal', 'max_first', 'max_last', 'nonpos', 'neginf_some',
            'all_neginf', 'mixed')


def edge_requests(G=NOMINAL_G):
    E = []
    add = lambda kind, why, line, **k: E.append(_req(kind, why, line=line, **k))

    def pw(M, fused, res, relu1, why, line, lead=0):
        null = ([] if res else ['res']) + ([] if fused else ['w1', 'shift1', 'hn'])
        add('pwpair', why, (PW, line), null=null, lead=lead, M=M, res=res, fused=fused, relu1=relu1)
    for M, why, line in (
            (32, 'one tile, one block: the prologue only', 'if (tn < ntiles) {'),
            (64, 'two blocks', 'int t = blockIdx.x;'),
            (32 * G, 'every block exactly one tile', 'const int grid = ntiles < 2 * cus ? ntiles : 2 * cus;'),
            (32 * (G + 1), 'one block takes a second tile: par flips, h lands in buffer 1',
             'egn_lds_dma16<true>(rh, lds0 + (unsigned)((par ^ 1) * PW_A_BYTES) + aldst[j]'),
            (32 * (2 * G + 3), 'three blocks take three tiles: par returns to 0, the R tile is reused twice',
             'par ^= 1;')):
        for fused, res, relu1 in PW_FORMS:
            pw(M, fused, res, relu1, why, line)
    for fused in (False, True):
        for res in (False, True):
            for relu1 in (0, 1):
                pw(32 * (G + 1), fused, res, relu1, 'all eight forms', 'if (has_res) v += *p;' if res else
                   ('const float lo1 = g.relu1 ? 0.f : -__builtin_inff();' if not fused else 'if constexpr (FUSED) {'))
    pw(32 * (G + 1), True, True, 1, 'every operand 16 bytes into its allocation',
       'const u32x4 rh = egn_rsrc(g.h, (size_t)g.M * PW_C1 * 4);', lead=4)

    for (N, K, H, W), lead, line, why in DECODE_SHAPES:
        for mode in (0, 1, 2):
            for content in CONTENTS:
                if content == 'mixed' and mode != 2:
                    continue
                add('decode', why + ', ' + content, line, lead=lead, N=N, K=K, H=H, W=W, mode=mode, idx=True,
                    content=content)
    for mode in (0, 1, 2):
        add('decode', 'out_idx NULL', ('decode.hip', 'if (out_idx) out_idx[map] = bidx;'), null=['idx'], N=2, K=3, H=4,
            W=4, mode=mode, idx=False, content='peaks')

    fz = lambda why, line, **k: add('fuse', why, (EW, line), **k)
    for relu in (0, 1):
        for shifts in ((0,), (0, 1), (0, 1, 2), (0, 1, 2, 3)):
            fz('%d terms, C < cs, 8 x 16: H >> 3 == 1' % len(shifts), 'if (k >= a.nterms) break;', N=2, H=8, W=16, C=18,
               cs=20, shifts=shifts, relu=relu)
        fz('the identity term in the middle', 'const int hs = a.H >> s, ws = a.W >> s;', N=1, H=6, W=10, C=8, cs=8,
           shifts=(0, 0, 1), relu=relu)
    fz('589 824 float4 outputs: a second trip with a ragged tail', 'if (g > 2048) g = 2048;', N=3, H=128, W=128, C=48,
       cs=48, shifts=(0, 1), relu=1)

    for C in (1, 3, 33, 35, 48):
        for cs in sorted({(C + 3) // 4 * 4, (C + 5 + 3) // 4 * 4}):
            add('to_nhwc', 'C %d in cs %d, 5 x 7' % (C, cs), (EW, 'v[k] = c < C ? x[((size_t)n * C + c) * hw + p] : 0.f;'),
                N=2, C=C, H=5, W=7, cs=cs)
            add('to_nchw', 'C %d in cs %d, 7 x 5' % (C, cs), (EW, 'y[e] = x[((size_t)n * hw + p) * cs + c];'), N=2, C=C,
                H=7, W=5, cs=cs)
    add('to_nhwc', '527 067 threads: a second trip with a ragged tail', (EW, 'if (g > 2048) g = 2048;'), N=1, C=35, H=241,
        W=243, cs=36)
    add('to_nchw', '526 683 threads: a second trip with a ragged tail', (EW, 'if (g > 2048) g = 2048;'), N=1, C=3, H=419,
        W=419, cs=4)
    for up in (1, 2, 4):
        for pad in (0, 5):
            cs = (33 * up * up + pad + 3) // 4 * 4
            add('pixshuf', 'up %d, C 33 in cs %d, 5 x 7' % (up, cs),
                (EW, 'y[e] = x[(((size_t)n * H + h) * W + w) * cs + (j * up + a) * up + b];'), N=2, C=33, H=5, W=7, cs=cs,
                up=up)
    add('pixshuf', '529 188 threads: a second trip with a ragged tail', (EW, 'if (g > 2048) g = 2048;'), N=1, C=3, H=209,
        W=211, cs=16, up=2)
    lens = (1, 2, 3, 7, 48, 64, 96, 255, 257)
    for i, W in enumerate(lens):
        add('ramps', 'W %d, H %d' % (W, lens[(i + 4) % 9]),
            (EW, 'const double fx = W > 1 ? (double)x * (1.0 / (double)(W - 1)) : 0.0;'), N=2, H=lens[(i + 4) % 9], W=W,
            cs=8, c0=3 if i % 2 else 6)
    add('ramps', 'c0 + 2 == cs', (EW, 'if (c0 < 0 || c0 + 2 > cs) return EGN_E_BADARG;'), N=1, H=5, W=7, cs=20, c0=18)
    add('ramps', '526 683 threads: a second trip with a ragged tail', (EW, 'if (g > 2048) g = 2048;'), N=3, H=419, W=419,
        cs=4, c0=2)
    return E


def cases_of(r):
    """The input sets a request runs on: two where arithmetic rounds, one where the kernel only moves data."""
    return CASES if r['kind'] in ('pwpair', 'fuse') else ('rounding',)


# ---------------------------------------------------------------------------------------------------------------
# inputs: {name: flat fp32 CPU tensor as it lies in memory}, the order of ``IN_NAMES``
# ---------------------------------------------------------------------------------------------------------------
IN_NAMES = {'pwpair': ('h', 'res', 'w3', 'shift3', 'w1', 'shift1'), 'fuse': ('t0', 't1', 't2', 't3'),
            'to_nhwc': ('x',), 'to_nchw': ('x',), 'pixshuf': ('x',), 'ramps': (), 'decode': ('hm',)}
OUT_NAMES = {'pwpair': ('out', 'hn'), 'fuse': ('y',), 'to_nhwc': ('y',), 'to_nchw': ('y',), 'pixshuf': ('y',),
             'ramps': ('y',), 'decode': ('xy', 'mx', 'idx')}
NAN = float('nan')


def _gen(r, case):
    return torch.Generator().manual_seed(zlib.crc32(repr((req_key(r), case)).encode()))


def out_numel(r):
    k = r['kind']
    if k == 'pwpair':
        return dict(out=r['M'] * 256, **({'hn': r['M'] * 64} if r['fused'] else {}))
    if k in ('fuse', 'to_nhwc', 'ramps'):
        return dict(y=r['N'] * r['H'] * r['W'] * r['cs'])
    if k == 'to_nchw':
        return dict(y=r['N'] * r['C'] * r['H'] * r['W'])
    if k == 'pixshuf':
        return dict(y=r['N'] * r['C'] * r['H'] * r['W'] * r['up'] ** 2)
    n = r['N'] * r['K']
    return dict(xy=2 * n, mx=n, **({'idx': n} if r['idx'] else {}))


def decode_maps(r, g):
    """fp32 [N K][H][W] of the request's content; non-negative for mode 2 except 'nonpos', 'mixed' and the -inf ones."""
    n, H, W, hw = r['N'] * r['K'], r['H'], r['W'], r['H'] * r['W']
    c = r['content']
    u = torch.rand(n, hw, generator=g)
    pick = lambda k: torch.stack([torch.randperm(hw, generator=g)[:k].sort().values for _ in range(n)])
    if c in ('peaks', 'neginf_some'):
        ys, xs = torch.arange(hw) // W, torch.arange(hw) % W
        cy, cx = torch.rand(n, 1, generator=g) * H, torch.rand(n, 1, generator=g) * W
        m = torch.randn(n, hw, generator=g) + 8.0 * torch.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / 8.0)
        if r['mode'] == 2:
            m = torch.sigmoid(m)
        if c == 'neginf_some':
            m[torch.rand(n, hw, generator=g) < 0.3] = -math.inf
    elif c in ('ties_lanes', 'ties_quad'):
        m = u
        if c == 'ties_lanes':
            at = pick(min(3, hw))
        else:
            q = torch.randint(0, max(hw // 4, 1), (n, 1), generator=g) * 4
            at = torch.cat([q + 1, q + 3], 1).clamp_max(hw - 1)
        m.scatter_(1, at, 2.0)
    elif c == 'all_equal':
        m = torch.full((n, hw), 0.5)
    elif c in ('max_first', 'max_last'):
        m = u
        m[:, 0 if c == 'max_first' else hw - 1] = 1.5
    elif c == 'nonpos':
        m = -3.0 * u
        m[::2, hw // 2] = 0.0                   # every other map: a maximum of exactly 0
    elif c == 'all_neginf':
        m = torch.full((n, hw), -math.inf)
    elif c == 'mixed':
        m = u - 0.25
    else:
        raise ValueError(c)
    return m.float().view(n, H, W)


def inputs(r, case):
    k = r['kind']
    g = _gen(r, case)
    x = {}
    if k == 'pwpair':
        M = r['M']
        if case == 'exact':
            draw = lambda *shape: torch.randint(-4, 5, shape, generator=g).float()
            t = dict(h=draw(M, 64), res=draw(M, 256), w3=draw(256, 64), shift3=draw(256), w1=draw(64, 256),
                     shift1=draw(64))
        else:
            t = dict(h=S.act_like(1, M // 32, 32, 64, 64, g).view(M, 64), res=torch.randn(M, 256, generator=g),
                     w3=S.filt(256, 64, 1, 1, g).view(256, 64) * GS.column_scale(256)[:, None],
                     shift3=torch.randn(256, generator=g),
                     w1=S.filt(64, 256, 1, 1, g).view(64, 256) * GS.column_scale(64)[:, None],
                     shift1=torch.randn(64, generator=g))
        x = {n: v.reshape(-1) for n, v in t.items() if n not in r['null']}
    elif k == 'fuse':
        N, H, W, C, cs = (r[n] for n in ('N', 'H', 'W', 'C', 'cs'))
        for i, s in enumerate(r['shifts']):
            hs, ws = H >> s, W >> s
            if case == 'exact':
                t = torch.zeros(N, hs, ws, cs)
                t[..., :C] = torch.randint(-4, 5, (N, hs, ws, C), generator=g).float()
            elif i == 0:
                t = S.act_like(N, hs, ws, C, cs, g)
            else:
                t = torch.zeros(N, hs, ws, cs)
                t[..., :C] = torch.randn(N, hs, ws, C, generator=g) * 2.0 ** -(3 * i)
            x['t%d' % i] = t.reshape(-1)
    elif k == 'to_nhwc':
        x['x'] = torch.randn(r['N'] * r['C'] * r['H'] * r['W'], generator=g)
    elif k in ('to_nchw', 'pixshuf'):
        used = r['C'] * (r['up'] ** 2 if k == 'pixshuf' else 1)
        t = torch.full((r['N'], r['H'], r['W'], r['cs']), NAN)
        t[..., :used] = torch.randn(r['N'], r['H'], r['W'], used, generator=g)
        x['x'] = t.reshape(-1)
    elif k == 'decode':
        x['hm'] = decode_maps(r, g).reshape(-1)
    return x


# ---------------------------------------------------------------------------------------------------------------
# the launches
# ---------------------------------------------------------------------------------------------------------------
def call_direct(r, ptr, stream):
    """The direct entry point; ``ptr(name)`` is the operand's address or None."""
    L = _lib.lib()
    k = r['kind']
    if k == 'pwpair':
        return L.egn_pw_pair_f32(ptr('h'), ptr('res'), ptr('w3'), ptr('shift3'), ptr('w1'), ptr('shift1'), ptr('out'),
                                 ptr('hn'), r['M'], r['relu1'], stream)
    if k == 'fuse':
        n = len(r['shifts'])
        terms = (ctypes.c_void_p * n)(*[ptr('t%d' % i) for i in range(n)])
        return L.egn_fuse_sum_relu_f32(ptr('y'), r['N'], r['H'], r['W'], r['C'], r['cs'], n, terms,
                                       (ctypes.c_int * n)(*r['shifts']), r['relu'], stream)
    if k == 'to_nhwc':
        return L.egn_nchw_to_nhwc_f32(ptr('x'), ptr('y'), r['N'], r['C'], r['H'], r['W'], r['cs'], stream)
    if k == 'to_nchw':
        return L.egn_nhwc_to_nchw_f32(ptr('x'), ptr('y'), r['N'], r['C'], r['H'], r['W'], r['cs'], stream)
    if k == 'pixshuf':
        return L.egn_pixel_shuffle_nhwc_to_nchw_f32(ptr('x'), ptr('y'), r['N'], r['C'], r['H'], r['W'], r['cs'], r['up'],
                                                    stream)
    if k == 'ramps':
        return L.egn_fill_coord_ramps_f32(ptr('y'), r['N'], r['H'], r['W'], r['cs'], r['c0'], stream)
    return L.egn_decode_heatmaps_f32(ptr('hm'), r['N'], r['K'], r['H'], r['W'], r['mode'], ptr('xy'), ptr('mx'),
                                     ptr('idx'), stream)


def add_to_program(r, prog, ref):
    """The egn_program_add_* call Program._emit makes for the kind; ``ref(name)`` is the operand's Ref or NULL_REF."""
    L = _lib.lib()
    k = r['kind']
    if k == 'pwpair':
        return L.egn_program_add_pw_pair(prog, ref('h'), ref('res'), ref('w3'), ref('shift3'), ref('w1'), ref('shift1'),
                                         ref('out'), ref('hn'), r['M'], r['relu1'])
    if k == 'fuse':
        n = len(r['shifts'])
        refs = (_lib.Ref * n)(*[ref('t%d' % i) for i in range(n)])
        return L.egn_program_add_fuse(prog, ref('y'), r['N'], r['H'], r['W'], r['C'], r['cs'], n, refs,
                                      (ctypes.c_int * n)(*r['shifts']), r['relu'])
    if k == 'to_nhwc':
        return L.egn_program_add_nchw_to_nhwc(prog, ref('x'), ref('y'), r['N'], r['C'], r['H'], r['W'], r['cs'])
    if k == 'to_nchw':
        return L.egn_program_add_nhwc_to_nchw(prog, ref('x'), ref('y'), r['N'], r['C'], r['H'], r['W'], r['cs'])
    if k == 'pixshuf':
        return L.egn_program_add_pixel_shuffle(prog, ref('x'), ref('y'), r['N'], r['C'], r['H'], r['W'], r['cs'], r['up'])
    if k == 'ramps':
        return L.egn_program_add_ramps(prog, ref('y'), r['N'], r['H'], r['W'], r['cs'], r['c0'])
    return L.egn_program_add_decode(prog, ref('hm'), r['N'], r['K'], r['H'], r['W'], r['mode'], ref('xy'), ref('mx'),
                                    ref('idx'))


# ---------------------------------------------------------------------------------------------------------------
# references and the checks.  ``got``: {output name: flat tensor as the launch left it}; the checks run on its device.
# ---------------------------------------------------------------------------------------------------------------
def _judge(name, case, got, want, A, Cb):
    """(worst ratio, failure strings) of one output under the case's rule."""
    bad = ~torch.isfinite(got)
    if bool(bad.any()):
        return math.inf, ['%s: %d elements not written / not finite' % (name, int(bad.sum()))]
    if case == 'exact':
        bad = got.double() != want
        if bool(bad.any()):
            i = int(bad.reshape(-1).nonzero()[0])
            return math.inf, ['%s, exact case: %d elements differ, first at flat %d: %r for %r'
                              % (name, int(bad.sum()), i, float(got.reshape(-1)[i]), float(want.reshape(-1)[i]))]
        return 0.0, []
    q = S.ratio(got, want, A)
    w = float(q.max()) if q.numel() else 0.0
    if not w <= Cb:
        return w, ['%s: error %.2f x 2^-24 A > %g at flat %d' % (name, w, Cb, int(q.reshape(-1).argmax()))]
    return w, []


def _bit_equal(name, got, want):
    same = got.contiguous().view(torch.int32) == want.to(got.device).contiguous().view(torch.int32)
    if bool(same.all()):
        return []
    i = int((~same).reshape(-1).nonzero()[0])
    return ['%s: %d elements differ from the index formula, first at flat %d: %r for %r'
            % (name, int((~same).sum()), i, float(got.reshape(-1)[i]), float(want.reshape(-1)[i]))]


def pw_reference(r, x, out_stored=None, dev='cpu'):
    """float64 on ``dev``: (out64, A_out) and, fused, (hn64, A_hn) on ``out_stored`` (default: fp32 of out64)."""
    M = r['M']
    d = lambda n, *shape: x[n].to(dev).double().view(*shape)
    h, w3, s3 = d('h', M, 64), d('w3', 256, 64), d('shift3', 256)
    pre, A = h @ w3.t() + s3, h.abs() @ w3.abs().t() + s3.abs()
    if r['res']:
        pre, A = pre + d('res', M, 256), A + d('res', M, 256).abs()
    out = pre.clamp_min(0) if r['relu1'] else pre
    if not r['fused']:
        return (out, A), None
    o = (out.float() if out_stored is None else out_stored.view(M, 256)).double()
    w1, s1 = d('w1', 64, 256), d('shift1', 64)
    return (out, A), ((o @ w1.t() + s1).clamp_min(0), o.abs() @ w1.abs().t() + s1.abs())


def upsampled(t, r, i, dt=torch.float64):
    s = r['shifts'][i]
    t = t.to(dt).view(r['N'], r['H'] >> s, r['W'] >> s, r['cs'])
    return t.repeat_interleave(1 << s, 1).repeat_interleave(1 << s, 2) if s else t


def decode_reference(r, hm):
    """numpy float64 of img_proc's three decoders on the fp32 maps: dict(idx, mx, xy [n][2], bound [n][2], A [n][2]);
    ``bound`` is the whole allowance of the soft modes, ``A`` the summation part's scale (0 in mode 0)."""
    n, W, hw = r['N'] * r['K'], r['W'], r['H'] * r['W']
    f = hm.detach().cpu().numpy().reshape(n, hw)
    idx = np.argmax(f, 1)
    mx = f[np.arange(n), idx]
    pos = np.stack([np.arange(hw) % W, np.arange(hw) // W], 1).astype(np.float64)         # [hw][2]
    zero = ~(mx > 0)
    A = np.zeros((n, 2))
    bound = np.zeros((n, 2))
    if r['mode'] == 0:
        xy = pos[idx].copy()
        xy[zero] = 0
    else:
        f64 = f.astype(np.float64)
        with np.errstate(all='ignore'):
            d = f64 - mx.astype(np.float64)[:, None]
            w = np.exp(d) if r['mode'] == 1 else f64
            s = w.sum(1)
            xy = (w[:, :, None] * pos[None]).sum(1) / s[:, None]
            A = (np.abs(w)[:, :, None] * pos[None]).sum(1) / np.abs(s)[:, None] + \
                np.abs(xy) * (np.abs(w).sum(1) / np.abs(s))[:, None]
            bound = C_DEC * U * A
            if r['mode'] == 1:
                da = np.where(np.isfinite(d), np.abs(d), 0.0)
                ea = w * (2 + 2.25 * da) * U + TINY
                bound = bound + 2 * (ea[:, :, None] * np.abs(pos[None] - xy[:, None, :])).sum(1) / s[:, None]
        if r['mode'] == 2:
            for t in (xy, A, bound):
                t[zero] = 0
    return dict(idx=idx.astype(np.int32), mx=mx, xy=xy, bound=bound, A=A)


def mixed_conditioning(r, hm):
    f = hm.double().view(r['N'] * r['K'], -1)
    return float((f.abs().sum(1) / f.sum(1).abs()).max())


def linspace_ramp(n):
    return torch.from_numpy(np.linspace(0, 1, n).astype(np.float32))


def check(r, case, x, got):
    """(worst ratio of the summation bounds, failure strings, notes) of what a launch (or an emulation) left."""
    k = r['kind']
    fails, worst, notes = [], 0.0, {}
    dev = next(iter(got.values())).device
    if k == 'pwpair':
        M = r['M']
        out = got['out'].view(M, 256)
        (o64, A), _ = pw_reference(r, x, dev=dev)
        worst, fails = _judge('out', case, out, o64, A, C_PW)
        notes['out'] = worst
        if r['fused']:
            if fails:
                fails.append('hn: not judged, out is not sound')
            else:
                _, (h64, A2) = pw_reference(r, x, out_stored=out, dev=dev)
                w2, f2 = _judge('hn', case, got['hn'].view(M, 64), h64, A2, C_PW)
                notes['hn'] = w2
                notes['hn_abs_sum_max'] = float(A2.max())
                fails += f2
                worst = max(worst, w2)
        notes['out_abs_max'] = float(o64.abs().max())
    elif k == 'fuse':
        n = len(r['shifts'])
        ts = [upsampled(x['t%d' % i].to(dev), r, i) for i in range(n)]
        y64, A = sum(ts), sum(t.abs() for t in ts)
        if r['relu']:
            y64 = y64.clamp_min(0)
        y = got['y'].view(y64.shape)
        worst, fails = _judge('y', case, y, y64, A, float(n))
        if not fails and r['C'] < r['cs'] and bool((y[..., r['C']:] != 0).any()):
            fails.append('y: pad channels of zero-padded terms are not zero')
    elif k == 'to_nhwc':
        N, C, H, W, cs = (r[n] for n in ('N', 'C', 'H', 'W', 'cs'))
        want = torch.zeros(N, H, W, cs)
        want[..., :C] = x['x'].view(N, C, H, W).permute(0, 2, 3, 1)
        fails = _bit_equal('y', got['y'].view(N, H, W, cs), want)
    elif k == 'to_nchw':
        N, C, H, W, cs = (r[n] for n in ('N', 'C', 'H', 'W', 'cs'))
        want = x['x'].view(N, H, W, cs)[..., :C].permute(0, 3, 1, 2).contiguous()
        fails = _bit_equal('y', got['y'].view(N, C, H, W), want)
    elif k == 'pixshuf':
        N, C, H, W, cs, up = (r[n] for n in ('N', 'C', 'H', 'W', 'cs', 'up'))
        # y[n, j, h up + a, w up + b] = x[n, h, w, (j up + a) up + b]
        want = x['x'].view(N, H, W, cs)[..., :C * up * up].reshape(N, H, W, C, up, up).permute(0, 3, 1, 4, 2, 5) \
            .reshape(N, C, H * up, W * up)
        fails = _bit_equal('y', got['y'].view(want.shape), want)
    elif k == 'ramps':
        N, H, W, cs, c0 = (r[n] for n in ('N', 'H', 'W', 'cs', 'c0'))
        want = torch.full((N, H, W, cs), SENTINEL)
        want[..., c0] = linspace_ramp(W)[None, None, :]
        want[..., c0 + 1] = linspace_ramp(H)[None, :, None]
        fails = _bit_equal('y', got['y'].view(N, H, W, cs), want)
    else:
        ref = decode_reference(r, x['hm'])
        n, hw = r['N'] * r['K'], r['H'] * r['W']
        if r['idx']:
            idx = got['idx'].view(torch.int32).cpu().numpy()
            if not np.array_equal(idx, ref['idx']):
                fails.append('idx: %s for %s' % (idx.tolist()[:8], ref['idx'].tolist()[:8]))
        mx = got['mx'].cpu().numpy()
        if not np.array_equal(mx, ref['mx']):
            fails.append('mx: %s for %s' % (mx.tolist()[:8], ref['mx'].tolist()[:8]))
        xy = got['xy'].double().cpu().numpy().reshape(n, 2)
        want, bound = ref['xy'], ref['bound']
        fin = np.isfinite(want)
        if r['mode'] == 0:
            if not np.array_equal(xy, want):
                fails.append('xy: hard arg-max differs: %s for %s' % (xy.tolist()[:4], want.tolist()[:4]))
        else:
            if bool(np.isfinite(xy[~fin]).any()):
                fails.append('xy: a number where float64 has none')
            err = np.abs(xy - want)
            ok = np.where(fin, err <= bound, True)
            if not bool(ok.all()):
                i = int(np.argmax(np.where(fin, err - bound, -np.inf)))
                fails.append('xy: %d outside the bound, worst |err| %.3g > %.3g at map %d coordinate %d'
                             % (int((~ok).sum()), err.reshape(-1)[i], bound.reshape(-1)[i], i // 2, i % 2))
            with np.errstate(all='ignore'):
                q = np.where(fin & (ref['A'] > 0), err / (U * ref['A']), 0.0)
            worst = float(np.nan_to_num(q, nan=0.0, posinf=0.0).max()) if q.size else 0.0
            notes['bound_max'] = float(np.where(fin, bound, 0.0).max())
    return worst, fails, notes


# ---------------------------------------------------------------------------------------------------------------
# the fp32 emulations (CPU) and the wrong kernels
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = {
    'pwpair': ('operands_10_bits', 'quads_swapped', 'res_of_previous_tile', 'shift_dropped', 'relu_before_residual',
               'hn_from_pre_relu_out'),
    'decode': ('last_index_on_ties', 'xy_swapped', 'last_float4_dropped', 'nonpos_not_zeroed_mode2'),
    'fuse': ('shift_off_by_one', 'relu_missing'),
    'pixshuf': ('a_b_swapped',),
    'ramps': ('one_over_w',),
    'to_nhwc': ('pad_not_zeroed',),
    'to_nchw': (),
}


def _mfma_chain(a, b):
    """acc[m][n] over k in the kernel's order: chunk c of 16, then s; one MFMA step takes k = 16 c + 4 kq + s,
    kq = 0 .. 3: the four products and the accumulator summed in a double, rounded once to fp32."""
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    ad, bd = a.double(), b.double()
    for c in range(a.shape[1] // 16):
        for s in range(4):
            ks = [16 * c + 4 * kq + s for kq in range(4)]
            acc = (acc.double() + ad[:, ks] @ bd[:, ks].t()).float()
    return acc


def emulated(r):
    """The request the CPU emulation runs: a 'pwpair' on its first EMU_ROWS rows."""
    return dict(r, M=min(r['M'], EMU_ROWS)) if r['kind'] == 'pwpair' else r


def _emulate_pw(r, x, mut):
    M = r['M']
    v = lambda n, *shape: x[n].view(*shape)
    h, w3, s3 = v('h', M, 64), v('w3', 256, 64), v('shift3', 256)
    if mut == 'operands_10_bits':
        h, w3 = GS.tf32(h), GS.tf32(w3)
    if mut == 'shift_dropped':
        s3 = torch.zeros_like(s3)
    pre = _mfma_chain(h, w3) + s3
    if r['res']:
        res = v('res', M, 256)
        if mut == 'res_of_previous_tile':
            res = torch.cat([res[:32], res[:-32]])
        if mut == 'relu_before_residual':
            pre = pre.clamp_min(0)
        pre = pre + res
    out = pre.clamp_min(0) if r['relu1'] and mut != 'relu_before_residual' else pre
    got = {}
    if r['fused']:
        a = pre if mut == 'hn_from_pre_relu_out' else out
        w1 = v('w1', 64, 256)
        if mut == 'operands_10_bits':
            a, w1 = GS.tf32(a), GS.tf32(w1)
        got['hn'] = (_mfma_chain(a, w1) + v('shift1', 64)).clamp_min(0).reshape(-1)
    if mut == 'quads_swapped':
        out = out.clone()
        t = out.view(M // 32, 32, 256)
        t[:, 5, 0:4], t[:, 5, 4:8] = t[:, 5, 4:8].clone(), t[:, 5, 0:4].clone()
    got['out'] = out.reshape(-1)
    return got


def decode_vec_path(r):
    hw = r['H'] * r['W']
    return hw % 4 == 0 and hw <= 4096 and r['lead'] % 4 == 0


def _lane_order(r):
    """[64][steps] element indices in the order a lane accumulates them (-1: nothing), register or scalar path."""
    hw = r['H'] * r['W']
    lane = np.arange(64)[:, None]
    if decode_vec_path(r):
        j, c = np.divmod(np.arange(64)[None, :], 4)
        q = lane + 64 * j
        o = np.where(q < hw // 4, 4 * q + c, -1)
    else:
        o = lane + 64 * np.arange((hw + 63) // 64)[None, :]
        o = np.where(o < hw, o, -1)
    return o


def _emulate_decode(r, x, mut):
    n, H, W = r['N'] * r['K'], r['H'], r['W']
    hw = H * W
    f = x['hm'].numpy().reshape(n, hw).copy()
    if mut == 'last_float4_dropped' and hw >= 8:
        f[:, -4:] = -np.inf
    idx = np.argmax(f, 1)
    if mut == 'last_index_on_ties':
        idx = hw - 1 - np.argmax(f[:, ::-1], 1)
    mx = f[np.arange(n), idx]
    i = np.arange(hw)
    px, py = (i % H, i // H) if mut == 'xy_swapped' else (i % W, i // W)
    zero = ~(mx > 0)
    if r['mode'] == 0:
        xy = np.stack([px[idx], py[idx]], 1).astype(np.float32)
        xy[zero] = 0
    else:
        with np.errstate(all='ignore'):
            if r['mode'] == 1:
                w = np.exp((f - mx[:, None]).astype(np.float32).astype(np.float64)).astype(np.float32)
            else:
                w = f
            if mut == 'last_float4_dropped' and hw >= 8:
                w = w.copy()
                w[:, -4:] = 0
            order = _lane_order(r)
            acc = np.zeros((3, n, 64), np.float32)                  # s, sx, sy per lane
            for st in range(order.shape[1]):
                o = order[:, st]
                live = o >= 0
                e = np.where(live[None, :], w[:, np.where(live, o, 0)], np.float32(0))
                e64 = e.astype(np.float64)
                new = np.stack([(acc[0] + e).astype(np.float32),
                                (e64 * px[np.where(live, o, 0)][None, :] + acc[1]).astype(np.float32),
                                (e64 * py[np.where(live, o, 0)][None, :] + acc[2]).astype(np.float32)])
                acc = np.where(live[None, None, :], new, acc)
            lanes = np.arange(64)
            for off in (32, 16, 8, 4, 2, 1):
                acc = (acc + acc[:, :, lanes ^ off]).astype(np.float32)
            xy = np.stack([acc[1, :, 0] / acc[0, :, 0], acc[2, :, 0] / acc[0, :, 0]], 1).astype(np.float32)
        if r['mode'] == 2 and mut != 'nonpos_not_zeroed_mode2':
            xy[zero] = 0
    got = dict(xy=torch.from_numpy(xy.reshape(-1)), mx=torch.from_numpy(mx.copy()))
    if r['idx']:
        got['idx'] = torch.from_numpy(idx.astype(np.int32))
    return got


def emulate(r, case, x, mut=None):
    """{output name: flat CPU tensor} as an fp32 kernel of the stated order (or the wrong kernel ``mut``) leaves it."""
    k = r['kind']
    if k == 'pwpair':
        return _emulate_pw(r, x, mut)
    if k == 'decode':
        return _emulate_decode(r, x, mut)
    if k == 'fuse':
        acc = None
        for i, s in enumerate(r['shifts']):
            if mut == 'shift_off_by_one' and s and i == len(r['shifts']) - 1:
                # the last term indexed with y >> (s + 1), x >> (s + 1) inside its own [H >> s][W >> s] map
                t = x['t%d' % i].view(r['N'], r['H'] >> s, r['W'] >> s, r['cs'])
                yy = (torch.arange(r['H']) >> (s + 1))[:, None]
                xx = (torch.arange(r['W']) >> (s + 1))[None, :]
                t = t[:, yy, xx]
            else:
                t = upsampled(x['t%d' % i], r, i, torch.float32)
            acc = t.clone() if acc is None else acc + t
        if r['relu'] and mut != 'relu_missing':
            acc = acc.clamp_min(0)
        return dict(y=acc.reshape(-1))
    N, H, W, cs = r['N'], r['H'], r['W'], r['cs']
    if k == 'to_nhwc':
        y = torch.full((N, H, W, cs), NAN if mut == 'pad_not_zeroed' else 0.0)
        y[..., :r['C']] = x['x'].view(N, r['C'], H, W).permute(0, 2, 3, 1)
        return dict(y=y.reshape(-1))
    if k == 'to_nchw':
        return dict(y=x['x'].view(N, H, W, cs)[..., :r['C']].permute(0, 3, 1, 2).reshape(-1))
    if k == 'pixshuf':
        C, up = r['C'], r['up']
        t = x['x'].view(N, H, W, cs)[..., :C * up * up].reshape(N, H, W, C, up, up)
        t = t.permute(0, 3, 1, 5, 2, 4) if mut == 'a_b_swapped' else t.permute(0, 3, 1, 4, 2, 5)
        return dict(y=t.reshape(-1))
    if k == 'ramps':
        y = torch.full((N, H, W, cs), SENTINEL)
        ramp = lambda n: (torch.arange(n).double() * (1.0 / (n if mut == 'one_over_w' else n - 1))).float() if n > 1 \
            else torch.zeros(1)
        y[..., r['c0']] = ramp(W)[None, None, :]
        y[..., r['c0'] + 1] = ramp(H)[None, :, None]
        return dict(y=y.reshape(-1))
    raise ValueError(k)


def mutant_applies(mut, r):
    """Whether the wrong kernel differs from the right one on this request at all."""
    k = r['kind']
    if k == 'pwpair':
        return {'res_of_previous_tile': r['res'] and r['M'] >= 64, 'relu_before_residual': r['res'] and r['relu1'] == 1,
                'hn_from_pre_relu_out': r['fused'] and r['relu1'] == 1}.get(mut, True)
    if k == 'decode':
        return {'last_index_on_ties': r['content'] in ('ties_lanes', 'ties_quad', 'all_equal') and r['H'] * r['W'] >= 4,
                'xy_swapped': r['H'] != r['W'] and r['content'] == 'peaks',
                'last_float4_dropped': r['content'] == 'max_last' and r['H'] * r['W'] >= 8,
                'nonpos_not_zeroed_mode2': r['mode'] == 2 and r['content'] == 'nonpos'}[mut]
    if k == 'fuse':
        return r['shifts'][-1] > 0 and r['H'] >> r['shifts'][-1] > 1 if mut == 'shift_off_by_one' else r['relu'] == 1
    if k == 'pixshuf':
        return r['up'] > 1
    if k == 'ramps':
        return max(r['H'], r['W']) > 1
    if k == 'to_nhwc':
        return r['cs'] > r['C']
    return True
