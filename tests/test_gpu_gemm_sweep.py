"""Every launch of csrc/gemm.hip that the lifter's training step makes on its dense route, and the edges of the kernel and
its launcher, element by element against float64.

The requests are those of tests/gemm_sweep.py: what one lifter step launches at 128 and at 256 rows, each distinct
launch replayed through egn_gemm_ex_f32 with the same NULL pattern and the same aliasing, and the hand-written edge
list.  Every request runs on two sets of inputs (gemm_sweep.CASES), and every launch is checked for:
  1. exact inputs: C equals the float64 product bit for bit; rounding inputs: |C - C64| <= CG[form] * 2^-24 * Abs on
     every element;
  2. every element of [M][N] written (C pre-filled with NaN); pad columns N .. ldc - 1, the floats in front of an offset
     operand, the guard bands around C, the statistics table and the workspace unchanged;
  3. the statistics table (form 0) against the stored z per 128-row block (gemm_sweep.stats_failures), bit for bit on the
     exact inputs, its extra row untouched;
  4. A, B, bias and a separate addend unchanged, their pad columns NaN (a read past the row length shows in C);
  5. the same bits from a second launch, for C and for the statistics;
  6. the workspace exactly egn_gemm_ws_bytes long.
A summary per form (requests, launches, worst |err| / (2^-24 Abs) and where) is printed.
"""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import gemm_sweep as G
from egonet_amd import _lib
from sweep_guards import _guarded, _guards_intact

pytestmark = pytest.mark.gpu

LEAD = 7.0                    # what the 16 bytes in front of an offset operand hold
HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _pitched(t, ld, off):
    """A device copy of the CPU matrix t [rows][n] with rows ``ld`` apart, NaN in the pad columns, ``off`` floats into
    its allocation.  The allocation ends with the last row's pitch: the size the kernel's descriptor spans."""
    rows, n = t.shape
    buf = torch.full((off + rows * ld,), float('nan'), device='cuda')
    buf[:off] = LEAD
    buf[off:].view(rows, ld)[:, :n] = t.cuda()
    return buf, buf[off:]


def _out(numel, dtype, off):
    """(whole, lead, body): ``body`` sits ``off`` elements behind the front guard band."""
    whole, body = _guarded(numel + off, dtype, None)
    return whole, body[:off], body[off:]


def _replay(r, case, x=None):
    """Both launches of one request on one set of inputs: (worst ratio, [failure strings], C [M][N] of the first)."""
    L = _lib.lib()
    form, M, N, K, ldc = r['form'], r['M'], r['N'], r['K'], r['ldc']
    fails = []
    if r.get('alias'):
        return 0.0, ['aliasing %s: the replay has no case for it' % (r['alias'],)], None
    if x is None:
        x = G.inputs(r, case)
    off = 4 if r['offset'] else 0
    Abuf, A = _pitched(x['A'], r['lda'], off)
    Bbuf, B = _pitched(x['B'], r['ldb'], off)
    bias = _pitched(x['bias'][None], N, off) if r['bias'] else None
    own = _pitched(x['addend'], ldc, off) if r['addend'] == 'own' else None
    ins = [('A', Abuf), ('B', Bbuf)] + ([('bias', bias[0])] if bias else []) + ([('addend', own[0])] if own else [])
    keep = {k: v.clone() for k, v in ins}
    xd = {k: v.cuda() for k, v in x.items()}
    want, Abs = G.reference(r, xd)
    Cwhole, Clead, C = _out(M * ldc, torch.float32, off)
    C0 = torch.full((M, ldc), float('nan'), device='cuda')
    if r['addend'] == 'C':
        C0[:, :N] = xd['addend']
    nrow = M // 128
    if r['stats']:
        srows = max(r['stats_rows'], nrow) + 1
        Swhole, Slead, St = _out(srows * 2 * N, torch.float64, off // 2)
    need = G.ws_bytes(r)
    if r['ws']:
        Wwhole, _, W = _out(max(need // 4, 4), torch.float32, 0)
    args = [form, _lib.ptr(A), _lib.ptr(B), _lib.ptr(C), _lib.ptr(bias[1]) if bias else None,
            _lib.ptr(C) if r['addend'] == 'C' else (_lib.ptr(own[1]) if own else None),
            _lib.ptr(St) if r['stats'] else None, r['stats_rows'], M, N, K, r['lda'], r['ldb'], ldc, r['variant'],
            _lib.ptr(W) if r['ws'] else None, need, _lib.current_stream()]
    worst, first = 0.0, None
    for rep in range(2):
        Clead.fill_(LEAD)
        C.copy_(C0.view(-1))
        if r['stats']:
            Slead.fill_(LEAD)
            St.fill_(float('nan'))
        if r['ws']:
            W.fill_(float('nan'))
        rc = L.egn_gemm_ex_f32(*args)
        torch.cuda.synchronize()
        if rc != 0:
            fails.append('launch %d returned %d (%s)' % (rep, rc, L.egn_strerror(rc).decode()))
            break
        if not _guards_intact(Cwhole) or not bool((Clead == LEAD).all()):
            fails.append('write in front of / behind C')
        if r['ws'] and not _guards_intact(Wwhole):
            fails.append('write outside the workspace of %d bytes' % need)
        if r['ws'] and need == 0 and not bool(torch.isnan(W).all()):
            fails.append('workspace written though egn_gemm_ws_bytes is 0')
        for k, v in ins:
            if not torch.equal(_bits(v), _bits(keep[k])):
                fails.append('input %s changed' % k)
        Cm = C.view(M, ldc)
        got = Cm[:, :N]
        if ldc > N and not torch.equal(_bits(Cm[:, N:]), _bits(C0[:, N:])):
            fails.append('pad columns of C written')
        stats = None
        if r['stats']:
            if not _guards_intact(Swhole) or not bool((Slead == LEAD).all()):
                fails.append('write in front of / behind the statistics table')
            stats = St.view(-1, 2, N)
            if not bool(torch.isnan(stats[nrow:]).all()):
                fails.append('statistics rows beyond M / 128 written')
            stats = stats[:nrow]
        if rep == 0:
            worst, f = G.judge(r, case, got, want, Abs)
            fails += f
            if stats is not None:
                if not bool(torch.isfinite(stats).all()):
                    fails.append('%d statistics entries not written' % int((~torch.isfinite(stats)).sum()))
                else:
                    fails += G.stats_failures(got, stats, nrow)
                    if case == 'exact':
                        s1, s2, _ = G.stats_reference(got, nrow)
                        sc = stats.cpu()
                        if not (torch.equal(sc[:, 0], s1) and torch.equal(sc[:, 1], s2)):
                            fails.append('exact case: statistics differ from the float64 sums')
            first = (got.clone(), None if stats is None else stats.clone())
        else:
            if not torch.equal(_bits(got), _bits(first[0])):
                fails.append('second launch: different bits in C')
            if stats is not None and not torch.equal(_bits(stats), _bits(first[1])):
                fails.append('second launch: different bits in the statistics')
    return worst, fails, (first[0] if first else None)


def _sweep(reqs, origin, per):
    fails = []
    for r in reqs:
        ent = per.setdefault(r['form'], dict(requests=0, launches=0, worst=0.0, where=''))
        ent['requests'] += 1
        for case in G.CASES:
            w, f, _ = _replay(r, case)
            ent['launches'] += 2
            if case == 'rounding' and w >= ent['worst']:
                ent['worst'], ent['where'] = w, '%s %dx%dx%d variant %d (%s)' % (origin, r['M'], r['N'], r['K'],
                                                                                   r['variant'], r['srcs'][0])
            fails += ['form %d variant %d %dx%dx%d ld %d/%d/%d %s (%s %s): %s'
                      % (r['form'], r['variant'], r['M'], r['N'], r['K'], r['lda'], r['ldb'], r['ldc'], case, origin,
                         r['srcs'][0], m) for m in f]
    return fails


def _report(per):
    for form, v in sorted(per.items()):
        print('form %d %s  %4d requests %5d launches  worst %5.2f (CG %g)  %s'
              % (form, G.FORM_NAMES[form], v['requests'], v['launches'], v['worst'], G.CG[form], v['where']))


def test_the_lifter_steps_dense_launches_match_float64():
    notes, reqs = G.recorded_requests('cuda')
    launches = [n for n in notes if n['name'] in ('egn_gemm_f32', 'egn_gemm_ex_f32')]
    print('\nrecorded: %d launches of gemm.hip, %d distinct' % (len(launches), len(reqs)))
    for r in reqs:
        print('   form %d variant %d %4d x %4d x %4d ld %d/%d/%d bias %d addend %s stats %d ws %d (%d splits)  %s'
              % (r['form'], r['variant'], r['M'], r['N'], r['K'], r['lda'], r['ldb'], r['ldc'], r['bias'], r['addend'],
                 r['stats'], r['ws'], G.splits(r), ', '.join(sorted(set(r['srcs'])))))
    miss = G.dense_route_taken(reqs, G.RECORDED_ROWS)
    assert not miss, miss
    # the fusions the step asks for are among them: statistics from the forward, the skip path in the data gradient
    assert any(r['stats'] for r in reqs) and any(r['addend'] for r in reqs)
    per = {}
    fails = _sweep(reqs, 'recorded', per)
    _report(per)
    assert not fails, '%d failures:\n%s' % (len(fails), '\n'.join(fails[:40]))


@pytest.mark.parametrize('form', [0, 1, 2])
def test_every_edge_request_matches_float64(form):
    reqs = [r for r in G.edge_requests() if r['form'] == form]
    assert {r['variant'] for r in reqs} == set(G.variants(form))
    per = {}
    fails = _sweep(reqs, 'edge', per)
    print()
    _report(per)
    torch.cuda.empty_cache()
    assert not fails, '%d failures:\n%s' % (len(fails), '\n'.join(fails[:40]))


def test_workspace_and_argument_refusals():
    """The split weight gradient takes a workspace of exactly egn_gemm_ws_bytes (checked between guard bands by every
    split request above); one float short or NULL is refused, as is a bias with form 2.  Nothing refused is launched:
    C keeps its NaNs."""
    L = _lib.lib()
    st = _lib.current_stream()
    r = G._req(2, 128, 1024, 256, 'refusals')
    need = G.ws_bytes(r)
    assert need == 2 * 128 * 1024 * 4
    A, B = torch.zeros(256, 128, device='cuda'), torch.zeros(256, 1024, device='cuda')
    Cwhole, C = _guarded(128 * 1024, torch.float32, float('nan'))
    Wwhole, W = _guarded(need // 4, torch.float32, float('nan'))
    bias = torch.zeros(1024, device='cuda')
    call = lambda b, ws, nbytes: L.egn_gemm_ex_f32(2, _lib.ptr(A), _lib.ptr(B), _lib.ptr(C), b, None, None, 0, 128, 1024,
                                                   256, 128, 1024, 1024, 0, ws, nbytes, st)
    assert call(None, _lib.ptr(W), need - 4) == G.BADARG
    assert call(None, None, need) == G.BADARG
    assert call(None, None, 0) == G.BADARG
    assert call(_lib.ptr(bias), _lib.ptr(W), need) == G.BADARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(C).all()) and bool(torch.isnan(W).all())
    assert call(None, _lib.ptr(W), need) == 0
    torch.cuda.synchronize()
    assert bool((C == 0).all()) and _guards_intact(Cwhole) and _guards_intact(Wwhole)


@pytest.mark.parametrize('form', [0, 1, 2])
def test_the_launcher_refuses_what_the_query_refuses(form):
    """A leading dimension below the row it strides, zero, negative; an operand at the extent limit.  The launcher is
    called only after the query has answered 0, so nothing that would write out of place is ever launched."""
    L = _lib.lib()
    st = _lib.current_stream()
    M, N, K = (128, 1024, 64) if form == 2 else (256, 384, 64)
    r = G._req(form, M, N, K, 'refusals')
    (ra, la), (rb, lb) = G.extents(r)
    A, B = torch.zeros(ra, la, device='cuda'), torch.zeros(rb, lb, device='cuda')
    Cwhole, C = _guarded(M * N, torch.float32, float('nan'))
    ext = dict(lda=la, ldb=lb, ldc=N)
    tried = 0
    for what, e in ext.items():
        for ld in (e - 4, 0, -4):
            a = dict(ext, **{what: ld})
            assert L.egn_gemm_supported(form, M, N, K, a['lda'], a['ldb'], a['ldc']) == 0, (what, ld)
            assert L.egn_gemm_ex_f32(form, _lib.ptr(A), _lib.ptr(B), _lib.ptr(C), None, None, None, 0, M, N, K, a['lda'],
                                     a['ldb'], a['ldc'], 0, None, 0, st) == G.BADARG, (what, ld)
            tried += 1
    rows = G.EXTENT_LIMIT // 4 // 1024
    big = {0: (rows, 128, 1024, 1024, 1024, 128), 1: (rows, 128, 1024, 1024, 128, 128),
           2: (1024, 128, rows, 1024, 128, 128)}[form]
    assert L.egn_gemm_supported(form, *big) == 0
    assert L.egn_gemm_ex_f32(form, _lib.ptr(A), _lib.ptr(B), _lib.ptr(C), None, None, None, 0, *big, 0, None, 0,
                             st) == G.BADARG
    torch.cuda.synchronize()
    assert tried == 9 and bool(torch.isnan(C).all()) and _guards_intact(Cwhole)


def test_the_older_block_order_computes_the_same_bits():
    """EGONET_AMD_GEMM_RASTER=0 (read once per process, kept in the product) in a fresh child process: 9 tiles in form
    0, 6 in form 1, 8 tiles x 8 splits in form 2, on both sets of inputs, bit for bit what this process computes in
    the default order.  This process launches first and only compares afterwards: a child that ends in a fault or
    runs out of time ends the session, with nothing more started on the GPU."""
    assert os.environ.get('EGONET_AMD_GEMM_RASTER', '1') != '0', 'the suite itself runs in the default order'
    mine = {}
    for k, r in enumerate(G.raster_requests()):
        for case in G.CASES:
            w, f, got = _replay(r, case)
            assert not f, f
            mine['%d-%s' % (k, case)] = got.cpu()
    torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'raster0.pt')
        env = dict(os.environ, EGONET_AMD_GEMM_RASTER='0')
        try:
            p = subprocess.run([sys.executable, os.path.join(HERE, 'gemm_raster_case.py'), out], env=env,
                               capture_output=True, text=True, timeout=240)
        except subprocess.TimeoutExpired:
            pytest.exit('the raster case did not end in 240 s: nothing more is started on the GPU', returncode=1)
        if p.returncode < 0 or p.returncode in (134, 139) or 'illegal memory access' in p.stderr:
            pytest.exit('the raster case ended in a fault (%d): nothing more is started on the GPU\n%s'
                        % (p.returncode, p.stderr[-2000:]), returncode=1)
        assert p.returncode == 0 and 'gemm raster case ok' in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
        theirs = torch.load(out)
    assert sorted(theirs) == sorted(mine)
    for k in sorted(mine):
        assert torch.equal(_bits(theirs[k]), _bits(mine[k])), k
