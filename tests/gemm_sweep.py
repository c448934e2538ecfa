"""The launches of csrc/gemm.hip (the lifter's dense layers: forward NT, data gradient NN, weight gradient TN) that the
training step makes on its default route, the edges of the kernel and its launcher, the inputs and the element-wise
bound of the sweep.

Helper module of tests/test_gemm_sweep_cpu.py and tests/test_gpu_gemm_sweep.py (imported, not a conftest).  Fourth of
the family of tests/conv_sweep.py, tests/wgrad_sweep.py and tests/train_ops_sweep.py: those three record the lifter
at a ragged 30 rows, where egn_gemm_supported answers 0 and the step takes the conv-kernel route, so none of them
launches gemm.hip.

A request is a dict:
  form, M, N, K, lda, ldb, ldc, variant     what a caller passes to egn_gemm_ex_f32
  bias, stats, ws                           whether that pointer is there (ws: the workspace pointer is non-NULL)
  addend                                    None, 'own' (a matrix of its own) or 'C' (the address of C: in place)
  stats_rows                                the value passed with `stats`
  offset                                    every operand starts 16 bytes into its allocation
  srcs                                      where it was seen (recorded run, or the kernel line an edge request is for)

Requests come from two places.  ``recorded_requests`` notes what conv_sweep.lifter_run launches at 128 and at 256 rows
(train_ops_sweep.Recorder on the egn_gemm_* entry points): the dense route in all three forms, the weight gradient
unsplit (K = 128) and in two splits (K = 256).  ``edge_requests`` is the hand-written list, each entry with the kernel
line it is there for, at the smallest shape that reaches the line.  Split counts are egn_gemm_ws_bytes' answers, tile
geometry (BM, BN, waves, STAGES) is read from the launcher's switch in the kernel's text (``tile_table``).

Each launch is run on two sets of inputs:
  exact     A, B, bias, addend integers in [-4, 4]: every partial sum stays below 2^24, fp32 is exact in any order, and
            C (and the statistics' sums, in doubles) must equal the float64 result bit for bit;
  rounding  Gaussian A; Gaussian B times a scale per output column that steps through 2^0 .. 2^-10 in blocks of 16
            columns; bias and addend O(1).  |C - C64| <= CG[form] * 2^-24 * Abs per element,
            Abs = |A||B| + |bias| + |addend| in float64.
Statistics (form 0): against the correctly rounded sums (math.fsum) of the STORED z per 128-row block,
  |s1 - want| <= 128 * 2^-53 * sum|z|,   |s2 - want| <= 128 * 2^-53 * sum z^2:
a square of an fp32 value is exact in a double, so a fixed-order double sum of 128 terms makes at most 127 roundings
of at most 2^-53 of the running sum each; derived, not measured.

CALIBRATION of CG.  Only a CPU emulation backs the constants: ``emulate`` is the arithmetic the kernel's header states,
a sequential fp32 fmaf chain in k order per split (the fused product-sum formed exactly in a double and rounded once
to fp32), the splits added in a fixed order, then bias / addend.  tests/test_gemm_sweep_cpu.py runs it on the
rounding inputs of the edge list (one request per distinct (form, M, N, K); shapes above 2^25 multiply-adds on their
first rows only) and prints the table:
  form   worst emulation ratio |err| / (2^-24 Abs)      CG
  0 NT   4.90  (256 x 256, K 64; 3.1 .. 4.6 at K 32 .. 160 on one tile)              20
  1 NN   5.23  (128 x 128, K 96; 3.4 .. 4.5 elsewhere)                               21
  2 TN   4.97  (2048 x 2048, K 64; 4.7 at K 224 unsplit, 2.7 at K 256 in 2 splits,
               1.5 at K 512 in 4, 0.4 at K 4096 in 32)                              20
The ratio does not grow with K (the products have zero mean: the rounding errors of a long chain average out faster
than Abs grows).  CG is about 4x the worst ratio: v_mfma_f32_16x16x4_f32 adds four products per step in an order of
its own, which the emulation cannot know.  The constants never come from the kernel's output.
Measured on the MI355X (tests/test_gpu_gemm_sweep.py, worst kernel ratio per form over all requests):
  0 NT   5.20  (edge, 128 x 128, K 64, variant 1; recorded 4.32 at 128 x 1024 x 1024, variant 3)
  1 NN   6.73  (edge, 256 x 256, K 96, all three pitched, variant 0; recorded 6.69 at 256 x 1024, K 96)
  2 TN   6.35  (edge, 2048 x 2048, K 64, variant 1; recorded 5.35 at 1024 x 1024, K 128, unsplit)
Every element of every launch is looked at there, many times the emulation's sample: that is where the distance to
the emulation's worst comes from.  All stay below a third of their constant.
"""
import math
import os
import re
import zlib

import numpy as np
import torch

import conv_sweep as S
import train_ops_sweep as T
from egonet_amd import _lib

U = S.U
U64 = 2.0 ** -53
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CG = {0: 20.0, 1: 21.0, 2: 20.0}
FORM_NAMES = {0: 'NT', 1: 'NN', 2: 'TN'}
GK = 32                                   # k per stage
REDUCE_GRID = 2048 * 256                  # float4 outputs one trip of the reduce kernel's grid covers
BADARG = -1
EXTENT_LIMIT = 0xF0000000                 # bytes: a buffer descriptor's range, as the launcher refuses it
ENTRY_POINTS = ('egn_gemm_f32', 'egn_gemm_ex_f32', 'egn_gemm_supported', 'egn_gemm_ws_bytes', 'egn_gemm_stats_rows')


# ---------------------------------------------------------------------------------------------------------------
# geometry: from the kernel's text and the library's host queries
# ---------------------------------------------------------------------------------------------------------------
_TILES = None


def tile_table():
    """{(form, variant): dict(BM, BN, WM, WN, STAGES, PW)} from the switch in egn_gemm_ex_f32 (csrc/gemm.hip)."""
    global _TILES
    if _TILES is None:
        with open(os.path.join(_ROOT, 'egonet_amd', 'csrc', 'gemm.hip')) as fh:
            text = fh.read()
        pat = r'(?:case (\d+)|default): (?:return|rc =) gemm_launch<(true|false), (true|false), (\d+), (\d+), (\d+), (\d+), (\d+)>'
        out = {}
        for case, akc, bkc, bm, bn, wm, wn, stages in re.findall(pat, text):
            form = {('true', 'true'): 0, ('true', 'false'): 1, ('false', 'false'): 2}[(akc, bkc)]
            bm, bn, wm, wn, stages = int(bm), int(bn), int(wm), int(wn), int(stages)
            pieces = (bm + bn) * GK * 4 // 1024                      # DMA instructions per stage
            assert pieces % (wm * wn) == 0
            out[(form, int(case) if case else 0)] = dict(BM=bm, BN=bn, WM=wm, WN=wn, STAGES=stages,
                                                         PW=pieces // (wm * wn))
        _TILES = out
    return _TILES


def variants(form):
    return sorted(v for f, v in tile_table() if f == form)


def ws_bytes(r):
    return int(_lib.lib().egn_gemm_ws_bytes(r['form'], r['M'], r['N'], r['K']))


def splits(r):
    need = ws_bytes(r)
    return need // (r['M'] * r['N'] * 4) if need else 1


def supported(r):
    return int(_lib.lib().egn_gemm_supported(r['form'], r['M'], r['N'], r['K'], r['lda'], r['ldb'], r['ldc']))


def geometry(r):
    """tiles, splits, stages per split (nks), and what the variant's template carries."""
    t = tile_table()[(r['form'], r['variant'])]
    sp = splits(r)
    return dict(t, tiles=(r['M'] // t['BM']) * (r['N'] // t['BN']), splits=sp, nks=r['K'] // sp // GK)


def extents(r):
    """(rows, row length) of A and of B as they lie."""
    form, M, N, K = r['form'], r['M'], r['N'], r['K']
    return ((K, M) if form == 2 else (M, K)), ((N, K) if form == 0 else (K, N))


# ---------------------------------------------------------------------------------------------------------------
# requests
# ---------------------------------------------------------------------------------------------------------------
KEY_FIELDS = ('form', 'M', 'N', 'K', 'lda', 'ldb', 'ldc', 'variant', 'bias', 'addend', 'stats', 'stats_rows', 'ws',
              'offset')


def req_key(r):
    return tuple(r[k] for k in KEY_FIELDS)


def _req(form, M, N, K, why, variant=0, lda=None, ldb=None, ldc=None, bias=False, addend=None, stats=False,
         offset=False, ws=None):
    r = dict(form=form, M=M, N=N, K=K, variant=variant, bias=bool(bias), addend=addend, stats=bool(stats),
             offset=bool(offset), srcs=[why])
    (_, la), (_, lb) = extents(r)
    r.update(lda=la if lda is None else lda, ldb=lb if ldb is None else ldb, ldc=N if ldc is None else ldc)
    r['stats_rows'] = M // 128 + 1 if stats else 0           # one more than needed: the extra row stays untouched
    r['ws'] = (ws_bytes(r) > 0) if ws is None else bool(ws)
    return r


def edge_requests():
    """The hand-written list (kernel lines: csrc/gemm.hip)."""
    E = []
    for form in (0, 1):
        for v in variants(form):
            add = lambda *a, **k: E.append(_req(form, *a, variant=v, **k))
            # the stage ring: `if (s < nks)` of the prologue (K = 32: one stage, fewer than STAGES - 1 issued), K = 64 and
            # 96 at the ring depth, 128 and 160 the first wrap of `stg`; PW selects the vmcnt literal of gemm_wait_vm
            for K in (32, 64, 96, 128, 160):
                add(128, 128, K, 'stage ring: K = %d, one tile (7 surplus blocks return early)' % K)
            # `if (split >= g.splits) return` / `if (t >= ntiles) return`: tile counts that are no multiple of 8
            add(128, 384, 32, '3 tiles (6 at BN = 64): rounded-up grid')
            add(256, 384, 64, '6 tiles (12 at BN = 64): rounded-up grid')
            add(384, 384, 32, '9 tiles (18 at BN = 64): rounded-up grid')
            add(1152, 128, 32, '9 tiles along M (18 at BN = 64)')
            # pvoff: (r0 + row) * ld, a_kstep / b_kstep with an MC operand; the epilogue's row * ldc
            add(256, 256, 96, 'lda = K + 4', lda=96 + 4)
            add(256, 256, 96, 'lda = K + 36', lda=96 + 36)
            add(256, 256, 96, 'ldb padded by 4', ldb=(96 if form == 0 else 256) + 4)
            add(256, 256, 96, 'ldc = N + 4', ldc=256 + 4, stats=form == 0, bias=form == 0)
            add(256, 256, 96, 'all three pitched', lda=96 + 36, ldb=(96 if form == 0 else 256) + 4, ldc=256 + 4)
            # egn_rsrc on a base that is 16-byte aligned and no more
            add(256, 256, 96, 'operands 16 bytes into their allocations', offset=True, bias=True, stats=form == 0,
                addend='own' if form == 1 else None)
            if form == 0:
                # the NT epilogue: `if (g.bias)`, `if (g.stats != nullptr)`, `bj = g.bias ? ... : 0.f`; at BN = 64 two
                # column tiles write one 128-column run of a statistics row
                for bias in (False, True):
                    for stats in (False, True):
                        add(256, 256, 64, 'NT epilogue: bias %d, stats %d' % (bias, stats), bias=bias, stats=stats)
            else:
                # the NN epilogue: `if (g.addend)` reads row * ldc, also where it is C itself; `if (g.bias)`
                for addend in (None, 'own', 'C'):
                    add(256, 256, 64, 'NN epilogue: addend %s' % addend, addend=addend)
                    add(256, 256, 64, 'NN epilogue: addend %s, ldc = N + 4' % addend, addend=addend, ldc=256 + 4)
                add(256, 256, 64, 'NN epilogue: bias', bias=True)
                add(256, 256, 64, 'NN epilogue: bias and addend in place', bias=True, addend='C')
    for v in variants(2):
        add = lambda *a, **k: E.append(_req(2, *a, variant=v, **k))
        for M, N in ((128, 1024), (1024, 128)):
            # splits == 1 below 256 tiles: K < 256 is never halved (and 224 / 2 is no multiple of 32); straight to C
            for K in (32, 96, 224):
                add(M, N, K, 'unsplit TN, K = %d: stores to C with ldc' % K)
            add(M, N, 96, 'unsplit TN, ldc = N + 4', ldc=N + 4)
            # the loop of egn_gemm_ws_bytes at 8 tiles: 2, 2, 4, 8, 16, 32 splits (asserted from the query)
            for K in (256, 320, 512, 1024, 2048, 4096):
                add(M, N, K, 'split TN, K = %d: slabs with ld N, reduce writes with ldc' % K)
        add(256, 512, 256, 'split TN pitched in all three dimensions', lda=256 + 4, ldb=512 + 4, ldc=512 + 4)
        add(2176, 1024, 256, '136 tiles, two splits: the second trip of the reduce kernel\'s loop')
        add(2048, 2048, 64, '256 tiles: never split')
    return E


# a recorded note's positional arguments (train_ops_sweep.Recorder names them a0, a1, ... for entry points it has no
# table for; pointers land in `null` or `alias`)
_POS = {
    'egn_gemm_f32': dict(form=0, A=1, B=2, C=3, bias=4, M=5, N=6, K=7, lda=8, ldb=9, ldc=10, variant=11, ws=12,
                         ws_bytes=13),
    'egn_gemm_ex_f32': dict(form=0, A=1, B=2, C=3, bias=4, addend=5, stats=6, stats_rows=7, M=8, N=9, K=10, lda=11,
                            ldb=12, ldc=13, variant=14, ws=15, ws_bytes=16),
}


def from_note(note):
    """A recorded launch as a request; None for the host-only queries.  An aliasing the replay has no case for
    (anything but addend == C) is kept in 'alias' and fails the replay."""
    pos = _POS.get(note['name'])
    if pos is None:
        return None
    name_of = {'a%d' % i: k for k, i in pos.items()}
    s = {name_of[a]: v for a, v in note['s'].items() if a in name_of}
    null = {name_of[a] for a in note['null'] if a in name_of}
    alias = tuple(tuple(sorted(name_of.get(a, a) for a in grp)) for grp in note['alias'])
    has = lambda a: a in pos and a not in null
    r = dict(form=s['form'], M=s['M'], N=s['N'], K=s['K'], lda=s['lda'], ldb=s['ldb'], ldc=s['ldc'],
             variant=s['variant'], bias=has('bias'), stats=has('stats'), stats_rows=s.get('stats_rows', 0),
             addend=None, ws=has('ws'), offset=False, srcs=[note['src']])
    if has('addend'):
        r['addend'] = 'C' if ('C', 'addend') in alias else 'own'
    r['alias'] = tuple(g for g in alias if g != ('C', 'addend'))
    return r


def merged(reqs):
    seen, out = {}, []
    for r in reqs:
        k = req_key(r) + (r.get('alias', ()),)
        if k in seen:
            seen[k]['srcs'] += r['srcs']
            continue
        seen[k] = dict(r, srcs=list(r['srcs']))
        out.append(seen[k])
    return out


RECORDED_ROWS = (128, 256)


def recorded_requests(device='cuda', handle=None):
    """(every note, the distinct launches as requests) of one lifter step with update=False at 128 and at 256 rows,
    autotune off (as train_ops_sweep.recorded_requests)."""
    g = torch.Generator().manual_seed(0)
    prev = os.environ.get('EGONET_AMD_AUTOTUNE')
    os.environ['EGONET_AMD_AUTOTUNE'] = '0'
    try:
        with T.Recorder(handle=handle, names=ENTRY_POINTS) as rec:
            for rows in RECORDED_ROWS:
                rec.src = 'train-lifter/b%d' % rows
                tr, step = S.lifter_run(rows, device, g, update=False)     # built inside: the step keeps the proxy
                step()
                if device != 'cpu':
                    torch.cuda.synchronize()
                del tr, step
    finally:
        if prev is None:
            del os.environ['EGONET_AMD_AUTOTUNE']
        else:
            os.environ['EGONET_AMD_AUTOTUNE'] = prev
    return rec.notes, merged([r for r in map(from_note, rec.notes) if r is not None])


def dense_route_taken(reqs, rows):
    """What the recorded runs have to hold for the sweep to mean anything: at least one launch of each form per run,
    the weight gradient unsplit at K = 128 and in two splits at K = 256.  Returns the list of what is missing."""
    miss = []
    for b in rows:
        mine = [r for r in reqs if 'train-lifter/b%d' % b in r['srcs']]
        for form in (0, 1, 2):
            if not any(r['form'] == form for r in mine):
                miss.append('no form %d launch at %d rows' % (form, b))
    for K, sp in ((128, 1), (256, 2)):
        if not any(r['form'] == 2 and r['K'] == K and splits(r) == sp for r in reqs):
            miss.append('no weight gradient with K = %d in %d split(s)' % (K, sp))
    return miss


# ---------------------------------------------------------------------------------------------------------------
# coverage, from the request list alone
# ---------------------------------------------------------------------------------------------------------------
RASTER_CASES = (
    (0, 384, 384, 32, '9 tiles'),
    (1, 256, 384, 64, '6 tiles'),
    (2, 128, 1024, 1024, '8 tiles x 8 splits'),
)


def raster_requests():
    """What the child process of the raster switch runs (EGONET_AMD_GEMM_RASTER=0: `split = b / (8 * per)`)."""
    return [_req(form, M, N, K, 'raster 0: ' + why) for form, M, N, K, why in RASTER_CASES]


def coverage(reqs):
    """{branch: True / False} for every branch the sweep is there for; all must be True."""
    G = [(r, geometry(r)) for r in reqs]
    cov = {}
    for (form, v), t in sorted(tile_table().items()):
        mine = [(r, g) for r, g in G if r['form'] == form and r['variant'] == v]
        tag = 'form %d variant %d: ' % (form, v)
        cov[tag + 'launched'] = bool(mine)
        nks = {g['nks'] for r, g in mine}
        st = t['STAGES']
        cov[tag + 'one stage'] = 1 in nks
        cov[tag + 'at the ring depth'] = st in nks
        cov[tag + 'first wrap of stg'] = any(n > st for n in nks)
        if form < 2:
            cov[tag + 'K = 32 .. 160'] = {1, 2, 3, 4, 5} <= nks
            cov[tag + 'tile counts 1, 3, 6, 9 (x2 at BN = 64)'] = \
                {1, 3, 6, 9} <= {g['tiles'] * t['BN'] // 128 for r, g in mine} and all(
                    g['tiles'] % 8 for r, g in mine if g['tiles'] * t['BN'] // 128 in (1, 3, 6, 9))
            cov[tag + 'offset operands'] = any(r['offset'] for r, g in mine)
        for what in ('lda', 'ldb', 'ldc'):
            cov[tag + what + ' pitched'] = any(_pitched(r, what) for r, g in mine)
        if form == 0:
            for bias in (False, True):
                for stats in (False, True):
                    cov[tag + 'bias %d stats %d' % (bias, stats)] = any(r['bias'] == bias and r['stats'] == stats
                                                                        for r, g in mine)
            cov[tag + 'stats with ldc > N'] = any(r['stats'] and _pitched(r, 'ldc') for r, g in mine)
        if form == 1:
            for addend in (None, 'own', 'C'):
                cov[tag + 'addend %s' % addend] = any(r['addend'] == addend for r, g in mine)
                if addend:
                    cov[tag + 'addend %s with ldc > N' % addend] = any(r['addend'] == addend and _pitched(r, 'ldc')
                                                                       for r, g in mine)
            cov[tag + 'bias'] = any(r['bias'] for r, g in mine)
        if form == 2:
            cov[tag + 'unsplit, K < 256'] = any(g['splits'] == 1 and r['K'] < 256 for r, g in mine)
            cov[tag + 'unsplit, K < 256, ldc > N'] = any(g['splits'] == 1 and r['K'] < 256 and _pitched(r, 'ldc')
                                                        for r, g in mine)
            cov[tag + 'unsplit, 256 tiles'] = any(g['splits'] == 1 and g['tiles'] >= 256 for r, g in mine)
            cov[tag + 'splits 2 .. 32 at 8 tiles'] = {2, 4, 8, 16, 32} <= {g['splits'] for r, g in mine
                                                                          if g['tiles'] == 8}
            cov[tag + 'split with all three pitched'] = any(g['splits'] > 1 and all(_pitched(r, w) for w in
                                                                                     ('lda', 'ldb', 'ldc'))
                                                            for r, g in mine)
            cov[tag + 'second trip of the reduce loop'] = any(g['splits'] > 1 and r['M'] * r['N'] // 4 > REDUCE_GRID
                                                              for r, g in mine)
    t2 = tile_table()[(0, 2)]
    cov['stats at BN = 64'] = t2['BN'] == 64 and any(r['form'] == 0 and r['variant'] == 2 and r['stats'] for r in reqs)
    cov['stats without bias'] = any(r['stats'] and not r['bias'] for r in reqs)
    rg = [geometry(r) for r in raster_requests()]
    cov['raster 0: 9 tiles NT, 6 tiles NN, 8 tiles x 8 splits TN'] = \
        [(r['form'], g['tiles'], g['splits']) for r, g in zip(raster_requests(), rg)] == [(0, 9, 1), (1, 6, 1), (2, 8, 8)]
    return cov


def _pitched(r, what):
    (_, la), (_, lb) = extents(r)
    return r[what] > {'lda': la, 'ldb': lb, 'ldc': r['N']}[what]


# ---------------------------------------------------------------------------------------------------------------
# inputs and the float64 reference
# ---------------------------------------------------------------------------------------------------------------
CASES = ('exact', 'rounding')
SCALE_STEPS, SCALE_BLOCK = 11, 16


def column_scale(N):
    """2^0 .. 2^-10 in blocks of 16 output columns."""
    return 2.0 ** -((torch.arange(N) // SCALE_BLOCK) % SCALE_STEPS).float()


def inputs(r, case):
    """{'A', 'B', 'bias', 'addend'}: fp32 CPU tensors without their pitch (A and B as they lie: ``extents``), from a
    seed derived from the request."""
    g = torch.Generator().manual_seed(zlib.crc32(repr((req_key(r), case)).encode()))
    (ra, la), (rb, lb) = extents(r)
    M, N = r['M'], r['N']
    x = {}
    if case == 'exact':
        draw = lambda *shape: torch.randint(-4, 5, shape, generator=g).float()
        x['A'], x['B'] = draw(ra, la), draw(rb, lb)
    else:
        draw = lambda *shape: torch.randn(*shape, generator=g)
        sc = column_scale(N)
        x['A'] = draw(ra, la)
        x['B'] = draw(rb, lb) * (sc[:, None] if r['form'] == 0 else sc[None, :])
    if r['bias']:
        x['bias'] = draw(N)
    if r['addend']:
        x['addend'] = draw(M, N)
    return x


def operands(r, x, dt=torch.float64):
    """a [M][K], b [K][N] in ``dt`` on the inputs' device."""
    a, b = x['A'].to(dt), x['B'].to(dt)
    return (a.t() if r['form'] == 2 else a), (b.t() if r['form'] == 0 else b)


def epilogue(r, x, c, absolute=False):
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    if 'bias' in x:
        c = c + f(x['bias'].to(c.dtype))
    if 'addend' in x:
        c = c + f(x['addend'].to(c.dtype))
    return c


def reference(r, x):
    """(C64, Abs) on the inputs' device: a plain float64 matmul, and the same on absolute values."""
    a, b = operands(r, x)
    return epilogue(r, x, a @ b), epilogue(r, x, a.abs() @ b.abs(), absolute=True)


def stats_reference(z, nrow):
    """(sums, sums of squares, sum|z|) per 128-row block of the stored z [M][N], float64 [nrow][N] each; the first two
    correctly rounded (math.fsum: exact accumulation, one rounding)."""
    zd = z.detach().double().cpu().reshape(nrow, 128, -1).numpy()
    s1 = np.array([[math.fsum(col) for col in blk.T] for blk in zd])
    s2 = np.array([[math.fsum(col) for col in (blk * blk).T] for blk in zd])        # squares of fp32: exact in double
    sa = np.abs(zd).sum(1)
    return torch.from_numpy(s1), torch.from_numpy(s2), torch.from_numpy(sa)


def stats_failures(z, stats, nrow):
    """The statistics table [nrow][2][N] (doubles) against the stored z: list of failure strings."""
    s1, s2, sa = stats_reference(z, nrow)
    st = stats.detach().cpu().double().view(nrow, 2, -1)
    fails = []
    for which, want, scale in ((0, s1, sa), (1, s2, s2)):
        err = (st[:, which] - want).abs()
        bad = ~(err <= 128 * U64 * scale)
        if bool(bad.any()):
            i = int(err.reshape(-1).argmax())
            fails.append('stats[%d]: %d entries outside 128 x 2^-53 x %s (worst %.3g at block %d column %d, want %.17g)'
                         % (which, int(bad.sum()), 'sum z^2' if which else 'sum|z|', float(err.reshape(-1)[i]),
                            i // want.shape[1], i % want.shape[1], float(want.reshape(-1)[i])))
    return fails


def judge(r, case, got, want, Abs):
    """(worst ratio or 0, failure strings) of a result [M][N] under the case's rule."""
    if not bool(torch.isfinite(got).all()):
        return float('inf'), ['%d elements not written / not finite' % int((~torch.isfinite(got)).sum())]
    if case == 'exact':
        bad = got.double() != want
        if bool(bad.any()):
            i = int(bad.reshape(-1).nonzero()[0])
            return float('inf'), ['exact case: %d elements differ, first at (%d, %d): %r for %r'
                                  % (int(bad.sum()), i // r['N'], i % r['N'], float(got.reshape(-1)[i]),
                                     float(want.reshape(-1)[i]))]
        return 0.0, []
    q = S.ratio(got, want, Abs)
    w = float(q.max())
    if not w <= CG[r['form']]:
        i = int(q.reshape(-1).argmax())
        return w, ['rounding case: error %.2f x 2^-24 Abs > %g at (%d, %d)' % (w, CG[r['form']], i // r['N'], i % r['N'])]
    return w, []


def old_tolerance(want, K):
    """The max-norm tolerance of tests/test_gpu_gemm.py."""
    return 2e-6 * K ** 0.5 * float(want.abs().max()) + 1e-5


# ---------------------------------------------------------------------------------------------------------------
# the fp32 emulation (the kernel's header: "an fp32 fmaf chain in k order per split, splits added in a fixed order")
# ---------------------------------------------------------------------------------------------------------------
EMULATION_BUDGET = 1 << 25           # multiply-adds per request; above it the first rows only


def emulated_rows(r):
    return max(8, min(r['M'], EMULATION_BUDGET // (r['N'] * r['K'])))


def _chain(a, b):
    """Sequential fmaf chain over k in fp32: acc = fl32(acc + a_k b_k), the product-sum formed in a double (the
    product of two fp32 values is exact there; the sum is rounded to double and then to fp32, which differs from a true
    fmaf only when the double lands exactly on an fp32 tie)."""
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    ad, bd = a.double(), b.double()
    for k in range(a.shape[1]):
        acc = (acc.double() + ad[:, k, None] * bd[None, k, :]).float()
    return acc


def emulate(r, x, nsplit=None, rows=None):
    """fp32 C[:rows] the way the header states it."""
    a, b = operands(r, x, torch.float32)
    rows = r['M'] if rows is None else rows
    a = a[:rows]
    sp = splits(r) if nsplit is None else nsplit
    ks = r['K'] // sp
    c = None
    for s in range(sp):
        part = _chain(a[:, s * ks:(s + 1) * ks], b[s * ks:(s + 1) * ks])
        c = part if c is None else c + part
    if 'bias' in x:
        c = c + x['bias']
    if 'addend' in x:
        c = c + x['addend'][:rows]
    return c


# ---------------------------------------------------------------------------------------------------------------
# reference-side slips: what a subtly wrong kernel would return, each computed in float64 so that only the slip
# separates it from the reference
# ---------------------------------------------------------------------------------------------------------------
def tf32(t):
    """Round an fp32 tensor to TF32's 10-bit mantissa (nearest even)."""
    b = t.contiguous().view(torch.int32)
    b = (b + 0xfff + ((b >> 13) & 1)) & ~0x1fff
    return b.view(torch.float32)


def stored(c, ldc, ld_used):
    """What reading [M][ldc] finds after rows were written ``ld_used`` floats apart (NaN where nothing was written)."""
    M, N = c.shape
    flat = torch.full((M * max(ldc, ld_used),), float('nan'), dtype=c.dtype)
    flat[:M * ld_used].view(M, ld_used)[:, :N] = c
    return flat[:M * ldc].view(M, ldc)[:, :N].clone()


def slips(r, x, nsplit):
    """{name: wrong C (float64 [M][N])} for a request; ``nsplit``: the split count the slab slips assume."""
    a, b = operands(r, x)
    M, N, K = r['M'], r['N'], r['K']
    want = epilogue(r, x, a @ b)
    out = {}
    nst = K // GK
    s = nst // 2
    a2 = a.clone()
    a2[:, s * GK:(s + 1) * GK] = 0
    out['a 32-deep stage dropped'] = epilogue(r, x, a2 @ b)
    if nst >= 2:
        a2, b2 = a.clone(), b.clone()
        s = max(nst // 2, 1)
        a2[:, s * GK:(s + 1) * GK] = a[:, (s - 1) * GK:s * GK]
        b2[s * GK:(s + 1) * GK] = b[(s - 1) * GK:s * GK]
        out['a stage used twice (in place of the next)'] = epilogue(r, x, a2 @ b2)
    if nsplit > 1:
        ks = K // nsplit
        s = nsplit // 2
        slab = a[:, s * ks:(s + 1) * ks] @ b[s * ks:(s + 1) * ks]
        out['one of %d split slabs dropped' % nsplit] = want - slab
        out['one of %d split slabs added twice' % nsplit] = want + slab
        if 'bias' in x:
            out['bias added once per split'] = want + (nsplit - 1) * x['bias'].double()
    if N >= SCALE_BLOCK * SCALE_STEPS:
        lo = SCALE_BLOCK * (SCALE_STEPS - 1)          # the first block of the lowest scale
        xt = dict(x, A=tf32(x['A']), B=tf32(x['B']))
        at, bt = operands(r, xt)
        wrong = want.clone()
        wrong[:, lo:lo + SCALE_BLOCK] = epilogue(r, x, at @ bt)[:, lo:lo + SCALE_BLOCK]
        out['operands rounded to TF32 in the 16 lowest-scale columns'] = wrong
    if r['form'] in (1, 2):
        # an M-contiguous operand: lane idx holds rows 4 idx + j of a 64-row group; the slip reads them as 16 j + idx
        idx, j = torch.arange(16)[:, None], torch.arange(4)[None, :]
        src, dst = (4 * idx + j).reshape(-1), (16 * j + idx).reshape(-1)
        wrong = want.clone()
        if r['form'] == 2:
            w = wrong.view(M // 64, 64, N)
            w[:, dst] = want.view(M // 64, 64, N)[:, src]
        else:
            w = wrong.view(M, N // 64, 64)
            w[:, :, dst] = want.view(M, N // 64, 64)[:, :, src]
        out['row interleave 4 idx + j taken as 16 j + idx'] = wrong
    if r['ldc'] > N:
        out['C addressed with N in place of ldc'] = stored(want, r['ldc'], N)
        if 'addend' in x:
            ad = stored(x['addend'].double(), N, r['ldc'])          # row m read at m * N of a matrix stored with ldc
            out['addend addressed with N in place of ldc'] = epilogue(r, dict(x, addend=ad), a @ b)
    return out


def stats_slips(r, x, z):
    """{name: wrong statistics table [nrow][2][N]} of the stored z (fp32 [M][N])."""
    nrow = r['M'] // 128
    t = tile_table()[(r['form'], r['variant'])]

    def table(zz, rows=slice(None)):
        zz = zz.double().view(nrow, 128, -1)[:, rows]
        return torch.stack([zz.sum(1), (zz * zz).sum(1)], 1)
    out = {}
    if 'bias' in x:
        out['stats without the bias'] = table(z - x['bias'])
    tm = 128 // t['WM']
    out['stats missing one wave row'] = table(z, slice(0, 128 - tm))
    return out
