"""The GEMM sweep's own parts, without a GPU: the request list against the branches it is there for, the calibration of
its constants on an fp32 emulation, reference-side slips outside the bound (and which of them the max-norm tolerance
of tests/test_gpu_gemm.py lets through), the statistics bound, the recorder's notes as requests, and the refusals of
egn_gemm_supported (a host-only query)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import gemm_sweep as G
import train_ops_sweep as T
from egonet_amd import _lib


def _text():
    import os
    with open(os.path.join(G._ROOT, 'egonet_amd', 'csrc', 'gemm.hip')) as fh:
        return fh.read()


def test_tile_table_is_the_launchers_switch():
    t = G.tile_table()
    assert {f: len(G.variants(f)) for f in (0, 1, 2)} == {0: 4, 1: 3, 2: 2}, t
    assert all(G.variants(f) == list(range(len(G.variants(f)))) for f in (0, 1, 2))
    literals = {int(v) for v in re.findall(r'vmcnt\((\d+)\)', _text())}
    for (form, v), g in sorted(t.items()):
        assert (g['STAGES'] - 2) * g['PW'] in literals, (form, v, g)
        print('form %d variant %d: %dx%d, %d x %d waves, %d stages, %d DMA pieces per wave -> vmcnt(%d)'
              % (form, v, g['BM'], g['BN'], g['WM'], g['WN'], g['STAGES'], g['PW'], (g['STAGES'] - 2) * g['PW']))
    # every combination of ring depth and pieces per wave the file instantiates is in the list
    assert {(g['STAGES'], g['PW']) for g in t.values()} == {(3, 4), (3, 8), (3, 6), (2, 4), (3, 12), (2, 8)}


def test_the_request_list_reaches_every_branch():
    E = G.edge_requests()
    assert len({G.req_key(r) for r in E}) == len(E)
    assert all(G.supported(r) == 1 for r in E)
    cov = G.coverage(E)
    for k, v in cov.items():
        print('%-70s %s' % (k, 'reached' if v else 'NOT REACHED'))
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    # the split counts are the query's: the K list of the edge requests walks its loop from 2 to 32 at 8 tiles
    for v in G.variants(2):
        got = [G.splits(r) for r in E if r['form'] == 2 and r['variant'] == v and (r['M'], r['N']) == (128, 1024)
               and r['K'] >= 256]
        print('form 2 variant %d, 128 x 1024, K 256 .. 4096: splits %s' % (v, got))
        assert got == sorted(got) and got[0] == 2 and got[-1] == 32
    # the row tests/test_gpu_gemm.py has at 64 tiles and K = 256 runs in two splits
    assert G.splits(G._req(2, 1024, 1024, 256, '')) == 2
    # smallest shapes: no edge request above 2^24 outputs x K except the three the reduce loop / 256 tiles need
    big = [r for r in E if r['M'] * r['N'] * r['K'] > 1 << 29]
    assert {(r['M'], r['N'], r['K']) for r in big} <= {(2176, 1024, 256), (128, 1024, 4096), (1024, 128, 4096)}, big


def _distinct_shapes(E):
    seen, out = set(), []
    for r in E:
        k = (r['form'], r['M'], r['N'], r['K'], r['bias'], r['addend'] is not None)
        if k not in seen:
            seen.add(k)
            out.append(r)
    return out


def test_calibration_of_the_constants_on_the_fp32_emulation():
    """CG[form] is about 4x the worst ratio of the emulation on the edge list's rounding inputs; the exact case is exact
    in the emulation too (the claim the exact rule rests on)."""
    worst = {f: (0.0, None) for f in (0, 1, 2)}
    for r in _distinct_shapes(G.edge_requests()):
        rows = G.emulated_rows(r)
        x = G.inputs(r, 'rounding')
        want, Abs = G.reference(r, x)
        q = float(G.S.ratio(G.emulate(r, x, rows=rows), want[:rows], Abs[:rows]).max())
        if q > worst[r['form']][0]:
            worst[r['form']] = (q, (r['M'], r['N'], r['K'], G.splits(r)))
        if r['K'] in (32, 160, 4096) and r['M'] * r['N'] <= 128 * 1024:
            x = G.inputs(r, 'exact')
            want, _ = G.reference(r, x)
            assert torch.equal(G.emulate(r, x, rows=rows).double(), want[:rows]), r
            assert float(want.abs().max()) < 2 ** 24
    print('\nform  worst emulation ratio   at (M, N, K, splits)        CG')
    for f in (0, 1, 2):
        print('%d %s  %6.2f                  %-26s %g' % (f, G.FORM_NAMES[f], worst[f][0], worst[f][1], G.CG[f]))
    for f in (0, 1, 2):
        assert 3.0 * worst[f][0] <= G.CG[f] <= 6.0 * worst[f][0], (f, worst[f], G.CG[f])


SLIP_REQUESTS = [
    G._req(0, 256, 256, 96, 'NT pitched', ldc=260, bias=True, stats=True),
    G._req(1, 256, 256, 64, 'NN pitched, addend', ldc=260, addend='own'),
    G._req(2, 128, 1024, 1024, 'TN, 8 splits'),
    G._req(2, 128, 1024, 4096, 'TN, 32 splits: a slip is smallest here'),
    dict(G._req(2, 128, 1024, 1024, 'TN, 8 splits, with a bias (reference side only: the launcher refuses it)'),
         bias=True),
]
WANTED_SLIPS = ('a 32-deep stage dropped', 'a stage used twice', 'split slabs dropped', 'split slabs added twice',
                'bias added once per split', 'TF32', 'row interleave', 'C addressed with N', 'addend addressed with N')


def test_every_slip_breaks_the_exact_case_or_the_bound():
    seen, accepted_by_old = set(), []
    for r in SLIP_REQUESTS:
        sp = G.splits(r)
        xs = {case: G.inputs(r, case) for case in G.CASES}
        refs = {case: G.reference(r, xs[case]) for case in G.CASES}
        wrong = {case: G.slips(r, xs[case], sp) for case in G.CASES}
        # unslipped, the emulation passes both rules on these very inputs
        rows = G.emulated_rows(r)
        for case in G.CASES:
            w, f = G.judge(r, case, G.emulate(r, xs[case], rows=rows), refs[case][0][:rows], refs[case][1][:rows])
            assert not f, (r['srcs'], case, f)
        for name in wrong['exact']:
            seen.add(name)
            caught = []
            for case in G.CASES:
                want, Abs = refs[case]
                got = wrong[case][name]
                if case == 'exact':
                    if not torch.equal(torch.nan_to_num(got, nan=1e30), want):
                        caught.append('exact')
                else:
                    q = G.S.ratio(torch.nan_to_num(got, nan=1e30), want, Abs)
                    if float(q.max()) > G.CG[r['form']]:
                        caught.append('bound (%.3g x)' % float(q.max()))
                    err = float((torch.nan_to_num(got, nan=1e30) - want).abs().max())
                    if err < G.old_tolerance(want, r['K']):
                        accepted_by_old.append((name, r['srcs'][0]))
            print('%-62s %-48s caught by: %s' % (name, r['srcs'][0][:48], ', '.join(caught) or 'NOTHING'))
            assert caught, (name, r['srcs'])
    for w in WANTED_SLIPS:
        assert any(w in s for s in seen), w
    print('the max-norm tolerance of tests/test_gpu_gemm.py (2e-6 sqrt(K) max|want| + 1e-5) ACCEPTS:')
    for name, src in accepted_by_old:
        print('    %s (%s)' % (name, src))
    # the gap this sweep closes is real: the low-scale TF32 slip passes the old tolerance
    assert any('TF32' in name for name, _ in accepted_by_old)


def _stats_in_kernel_order(z, t):
    """The NT epilogue's statistics in its own order, in doubles: a lane adds its MT x 4 rows (16 i + 4 kq + r) one after
    the other, the four kq lanes join by two butterfly steps, the WM waves of a column are added in order."""
    M, N = z.shape
    nrow, tm = M // 128, 128 // t['WM']
    zd = z.double().numpy().reshape(nrow, t['WM'], tm // 16, 4, 4, N)        # [block][wm][i][kq][r][col]
    out = np.zeros((nrow, 2, N))
    for which in (0, 1):
        v = zd * zd if which else zd
        lane = np.zeros((nrow, t['WM'], 4, N))
        for i in range(tm // 16):
            for r in range(4):
                lane = lane + v[:, :, i, :, r]
        wave = (lane[:, :, 0] + lane[:, :, 1]) + (lane[:, :, 2] + lane[:, :, 3])
        tot = np.zeros((nrow, N))
        for k in range(t['WM']):
            tot = tot + wave[:, k]
        out[:, which] = tot
    return torch.from_numpy(out)


@pytest.mark.parametrize('variant', [0, 2])
def test_statistics_bound_holds_in_the_kernels_order_and_sees_the_slips(variant):
    r = G._req(0, 256, 256, 96, 'stats', variant=variant, bias=True, stats=True)
    t = G.tile_table()[(0, variant)]
    for case in G.CASES:
        x = G.inputs(r, case)
        if case == 'rounding':
            x['bias'] = x['bias'] + 1000.0                 # a mean 1e3 x the deviation: the sums' hardest column
        z = G.emulate(r, x)
        nrow = r['M'] // 128
        assert not G.stats_failures(z, _stats_in_kernel_order(z, t), nrow)
        if case == 'exact':                                # integers: the double sums are exact
            s1, s2, _ = G.stats_reference(z, nrow)
            st = _stats_in_kernel_order(z, t)
            assert torch.equal(st[:, 0], s1) and torch.equal(st[:, 1], s2)
        wrong = G.stats_slips(r, x, z)
        assert set(wrong) == {'stats without the bias', 'stats missing one wave row'}
        for name, table in wrong.items():
            f = G.stats_failures(z, table, nrow)
            print('%-30s %-9s %s' % (name, case, f[0][:100] if f else 'NOT CAUGHT'))
            assert f, (name, case)


class _Stub(object):
    """Stands in for the library: every entry point answers 0."""
    def __getattr__(self, name):
        return lambda *a: 0


def test_recorded_notes_become_requests_with_their_null_pattern_and_aliasing():
    p = lambda v: C.c_void_p(v)
    with T.Recorder(handle=_Stub(), names=G.ENTRY_POINTS) as rec:
        L = _lib.lib()
        rec.src = 'train-lifter/b128'
        L.egn_gemm_supported(0, 128, 1024, 1024, 1024, 1024, 1024)
        L.egn_gemm_ex_f32(0, p(0x1000), p(0x2000), p(0x3000), p(0x4000), None, p(0x5000), 1, 128, 1024, 1024, 1024, 1024,
                          1024, 3, None, 0, p(0x99))
        L.egn_gemm_ex_f32(1, p(0x1000), p(0x2000), p(0x3000), None, p(0x3000), None, 0, 128, 1024, 1024, 1024, 1024,
                          1024, 0, None, 0, None)
        L.egn_gemm_ex_f32(1, p(0x1000), p(0x2000), p(0x3000), None, p(0x6000), None, 0, 128, 1024, 1024, 1024, 1024,
                          1024, 0, None, 0, None)
        L.egn_gemm_f32(2, p(0x1000), p(0x2000), p(0x3000), None, 1024, 1024, 128, 1024, 1024, 1024, 1, p(0x7000), 64, None)
        L.egn_gemm_f32(2, p(0x1000), p(0x2000), p(0x3000), None, 1024, 1024, 128, 1024, 1024, 1024, 1, p(0x7000), 64, None)
        rec.src = 'train-lifter/b256'
        L.egn_gemm_f32(2, p(0x1000), p(0x2000), p(0x3000), None, 1024, 1024, 256, 1024, 1024, 1024, 1, p(0x7000), 1 << 23,
                       None)
        L.egn_gemm_ex_f32(1, p(0x1000), p(0x1000), p(0x3000), None, None, None, 0, 128, 1024, 1024, 1024, 1024, 1024, 0,
                          None, 0, None)
    assert len(rec.notes) == 8
    reqs = G.merged([r for r in map(G.from_note, rec.notes) if r is not None])
    assert len(reqs) == 6                                  # the query dropped, the repeated launch merged
    fwd, inplace, own, wg128, wg256, odd = reqs
    assert (fwd['form'], fwd['variant'], fwd['bias'], fwd['stats'], fwd['stats_rows'], fwd['addend'], fwd['ws']) == \
        (0, 3, True, True, 1, None, False)
    assert inplace['addend'] == 'C' and own['addend'] == 'own' and not inplace['alias'] and not own['alias']
    assert (wg128['form'], wg128['K'], wg128['ws'], wg128['bias'], len(wg128['srcs'])) == (2, 128, True, False, 2)
    assert G.splits(wg128) == 1 and G.splits(wg256) == 2
    assert odd['alias'] == (('A', 'B'),)                   # an aliasing the replay has no case for stays visible
    miss = G.dense_route_taken(reqs, G.RECORDED_ROWS)
    assert miss == ['no form 0 launch at 256 rows'], miss  # (the stub's second run made only two of the three forms ...)


def _query(form, M, N, K, lda, ldb, ldc):
    return int(_lib.lib().egn_gemm_supported(form, M, N, K, lda, ldb, ldc))


REFUSAL_SHAPES = [(0, 256, 384, 64), (1, 256, 384, 64), (2, 128, 1024, 64)]


@pytest.mark.parametrize('form,M,N,K', REFUSAL_SHAPES)
def test_the_query_refuses_a_leading_dimension_below_the_row_it_strides(form, M, N, K):
    """lda = 0 or ldc = 0 put every row on row 0, ldc < N makes rows overwrite each other; negative multiples of 4
    passed the `& 3` test as well.  Host-only: nothing is launched."""
    r = G._req(form, M, N, K, '')
    (_, la), (_, lb) = G.extents(r)
    ext = dict(lda=la, ldb=lb, ldc=N)
    assert ext == {0: dict(lda=K, ldb=K, ldc=N), 1: dict(lda=K, ldb=N, ldc=N), 2: dict(lda=M, ldb=N, ldc=N)}[form]
    assert _query(form, M, N, K, la, lb, N) == 1
    for what, e in ext.items():
        for ld, want in ((e + 4, 1), (e, 1), (e - 4, 0), (0, 0), (-4, 0), (-e, 0), (e + 2, 0)):
            a = dict(ext, **{what: ld})
            assert _query(form, M, N, K, a['lda'], a['ldb'], a['ldc']) == want, (what, ld, want)


def test_the_query_refuses_the_byte_extents_the_launcher_refuses():
    """egn_gemm_ex_f32 refuses an operand of 0xF0000000 bytes or more (a buffer descriptor's range); the query has to
    say so first, or train_lifter._gemm raises where it should fall back to the conv-kernel route."""
    lim = G.EXTENT_LIMIT // 4                               # floats
    # A: rows x lda (form 2: K rows), B: rows x ldb (form 0: N rows)
    rows = lim // 1024
    assert rows % 128 == 0 and rows * 1024 == lim
    assert _query(0, rows, 128, 1024, 1024, 1024, 128) == 0 and _query(0, rows - 128, 128, 1024, 1024, 1024, 128) == 1
    assert _query(0, 128, rows, 1024, 1024, 1024, rows) == 0 and _query(0, 128, rows - 128, 1024, 1024, 1024, rows) == 1
    assert _query(1, rows, 128, 1024, 1024, 128, 128) == 0 and _query(1, rows - 128, 128, 1024, 1024, 128, 128) == 1
    assert _query(1, 128, 1024, rows, rows, 1024, 1024) == 0 and _query(1, 128, 1024, rows - 128, rows, 1024, 1024) == 1
    assert _query(2, 1024, 128, rows, 1024, 128, 128) == 0 and _query(2, 1024, 128, rows - 128, 1024, 128, 128) == 1
    assert _query(2, 128, 1024, rows, 128, 1024, 1024) == 0 and _query(2, 128, 1024, rows - 128, 128, 1024, 1024) == 1
    # by the pitch alone
    ld = lim // 128
    assert _query(0, 128, 128, 32, ld, 32, 128) == 0 and _query(0, 128, 128, 32, ld - 4, 32, 128) == 1
    assert _query(0, 128, 128, 32, 32, ld, 128) == 0 and _query(0, 128, 128, 32, 32, ld - 4, 128) == 1
    # the lifter's shapes are still taken: the bench batch, and the rows the recorded runs use
    for B in (128, 256, 4096):
        assert _query(0, B, 1024, 1024, 1024, 1024, 1024) == 1
        assert _query(1, B, 1024, 1024, 1024, 1024, 1024) == 1
        assert _query(1, B, 1024, 96, 96, 1024, 1024) == 1
        assert _query(2, 1024, 1024, B, 1024, 1024, 1024) == 1
