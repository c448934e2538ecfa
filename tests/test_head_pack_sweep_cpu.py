"""tests/head_pack_sweep.py without a GPU: the ledger of the training steps' entry points, the references against
independent statements (torch autograd of F.pixel_shuffle + the criteria, F.avg_pool2d, F.pixel_unshuffle, the
reference's cross-ratio fixture, the host packers of filters.py), the fp32 emulations' ratios that the constants come
from, the share of undecided elements per case, what the edge list covers (from the request list and the kernels' text)
and the mutants."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_pack_sweep as HP
from egonet_amd import _lib

_TESTS = os.path.dirname(os.path.abspath(__file__))
EDGES = HP.edge_requests()
SMALL = [r for r in EDGES if not r['opt'].get('big') and not r['opt'].get('refuse')]
_CACHE = {}


def _case(r):
    """(inputs, reference) of an edge request, computed once and left unchanged."""
    k = id(r)
    if k not in _CACHE:
        x = HP.inputs(r)
        _CACHE[k] = (x, HP.reference(r, x))
    return _CACHE[k]


# ---------------------------------------------------------------------------------------------------------------
# the ledger
# ---------------------------------------------------------------------------------------------------------------
def test_every_entry_point_of_a_training_step_has_one_owner():
    called = HP.called_entries()
    assert called, 'no entry point found in the step modules'
    unowned = sorted(called - HP.QUERIES - set(HP.OWNERS))
    assert not unowned, 'called by a training step, owned by no sweep: %s' % unowned
    assert not HP.QUERIES & set(HP.OWNERS)
    for name, f in HP.OWNERS.items():
        assert os.path.exists(os.path.join(_TESTS, f)), (name, f)
    # the owning sweep's helper module really names the entry point (a rename there breaks the ledger here)
    helper = {'test_gpu_conv_sweep.py': ('conv_sweep.py', 'test_gpu_conv_sweep.py'),
              'test_gpu_wgrad_sweep.py': ('wgrad_sweep.py', 'test_gpu_wgrad_sweep.py'),
              'test_gpu_train_ops_sweep.py': ('train_ops_sweep.py',),
              'test_gpu_gemm_sweep.py': ('gemm_sweep.py', 'test_gpu_gemm_sweep.py'),
              'test_gpu_program_ops_sweep.py': ('program_ops_sweep.py', 'test_gpu_program_ops_sweep.py'),
              HP.GPU_TEST: ('head_pack_sweep.py',)}
    for name, f in sorted(HP.OWNERS.items()):
        text = ''.join(open(os.path.join(_TESTS, h)).read() for h in helper[f])
        assert name in text, '%s is not named in %s' % (name, helper[f])
    # this sweep's names: every one is called by a step module, defined in the library and on the edge list
    mine = {k for k, f in HP.OWNERS.items() if f == HP.GPU_TEST}
    assert mine == set(HP.LAUNCHING) and mine <= called, sorted(mine - called)
    assert set(HP.SIZES) <= called | {'egn_wino_weight_floats', 'egn_wino4_pack_weight_floats'}
    csrc = ''.join(HP.kernel_text(f) for f in ('heads.hip', 'cross_ratio.hip', 'filter_pack.hip'))
    for name in list(HP.LAUNCHING) + list(HP.SIZES):
        assert re.search(r'extern "C" [\w ]+ %s\(' % name, csrc), name
        assert name in _lib.SIGNATURES, name
    on_list = {r['name'] for r in EDGES}
    assert set(HP.LAUNCHING) - {HP.BATCH} <= on_list and HP.BATCH_EDGES
    print('\n%d entry points called by the step modules: %d queries, %d owned by %d sweeps'
          % (len(called), len(called & HP.QUERIES), len(called & set(HP.OWNERS)), len(set(HP.OWNERS.values()))))


def test_every_edge_request_names_a_line_of_its_kernel():
    for r in EDGES + HP.query_grid():
        f, text = r['line']
        assert text in HP.kernel_text(f), (f, text)
    hd, fp = HP.kernel_text('heads.hip'), HP.kernel_text('filter_pack.hip')
    assert '(size_t)TW * (cs + 1) * 4 > %d' % HP.LDS_LIMIT in hd and 'int TW = 16;' in hd
    assert 'if (g > 4096) g = 4096;' in hd and 'g < 4096 ? g : 4096' in fp and 'if (g > 16384) g = 16384;' in fp
    assert len(re.findall(r'__launch_bounds__\(256\)', hd + fp)) == 6


# ---------------------------------------------------------------------------------------------------------------
# the references against independent statements
# ---------------------------------------------------------------------------------------------------------------
def _torch_crit(crit):
    return (F.mse_loss, F.l1_loss, F.smooth_l1_loss)[crit]


def test_pixshuf_reference_is_autograd_of_pixel_shuffle_and_the_criterion():
    n = 0
    for r in SMALL:
        if r['name'] != HP.PIX or r['s']['cs'] > 64:
            continue
        s = r['s']
        x, ref = _case(r)
        cc = s['C'] * s['up'] ** 2
        xp = x['x'].reshape(s['N'], s['H'], s['W'], s['cs'])[..., :cc].double().clone().requires_grad_(True)
        maps = F.pixel_shuffle(xp.permute(0, 3, 1, 2), s['up'])
        t = x['tgt'].reshape(s['N'], s['C'], s['H'] * s['up'], s['W'] * s['up']).double()
        w = x['tw'].reshape(s['N'], s['C'], 1, 1).double() if 'tw' in x else 1.0
        loss = s['weight'] * _torch_crit(s['crit'])(maps * w, t * w) + float(x['loss'][0])
        loss.backward()
        lv = float(loss.detach())
        assert abs(lv - float(ref["loss"][0])) <= 1e-12 * max(1.0, abs(lv)), r["srcs"]
        if 'dx' in ref:
            want = ref['dx'][0].reshape(s['N'], s['H'], s['W'], s['cs'])
            assert bool((want[..., cc:] == 0).all())
            keep = ref['dx'][2]
            err = (want[..., :cc] - xp.grad).abs()
            if r['opt'].get('content') == 'ints':
                tol = 2.0 ** -24 * xp.grad.abs() + 1e-300          # (the exact case holds float32(c' inv) w)
            else:
                tol = 1e-12 * xp.grad.abs().max()
            assert bool((err <= tol).all()), (r['srcs'], float(err.max()))
            assert keep is None or s['crit'] == 1
        n += 1
    assert n > 30


def test_pool_and_unshuffle_references_are_torchs():
    for r in SMALL:
        s = r['s']
        x, ref = _case(r)
        if r['name'] == HP.APF:
            xs = x['x'].reshape(s['N'], s['H'], s['W'], s['cs']).double().permute(0, 3, 1, 2)
            want = F.avg_pool2d(xs, s['k']).permute(0, 2, 3, 1).reshape(-1)
            assert float((ref['y'][0] - want).abs().max()) <= 1e-14 * float(want.abs().max() + 1), r['srcs']
        elif r['name'] == HP.APB:
            k = s['k']
            xs = torch.zeros(s['N'], s['cs'], s['H'], s['W'], dtype=torch.float64, requires_grad=True)
            dy = x['dy'].reshape(s['N'], s['H'] // k, s['W'] // k, s['cs']).double().permute(0, 3, 1, 2)
            (F.avg_pool2d(xs, k) * dy).sum().backward()
            want = xs.grad.permute(0, 2, 3, 1).reshape(-1) + (x['dx'].double() if s['accumulate'] else 0.0)
            assert float((ref['dx'][0] - want).abs().max()) <= 1e-14 * float(want.abs().max() + 1), r['srcs']
            if not s['accumulate'] and k & (k - 1) == 0:
                assert bool((ref['dx'][1] == 0).all())                  # the exact case
        elif r['name'] == HP.UNS:
            xs = x['x'].reshape(s['N'], s['C'], s['H'] * s['up'], s['W'] * s['up'])
            want = torch.zeros(s['N'], s['H'], s['W'], s['cs'], dtype=torch.float64)
            want[..., :s['C'] * s['up'] ** 2] = F.pixel_unshuffle(xs, s['up']).permute(0, 2, 3, 1).double()
            assert torch.equal(ref['y'][0], want.reshape(-1)), r['srcs']


def test_cross_ratio_reference_is_the_reference_fixture():
    from conftest import golden
    g = golden('cr_loss.npz')
    for tag in ('rand', 'wide', 'cluster'):
        coords = torch.from_numpy(g[tag + '/coords'])
        n = coords.shape[0]
        for spec, crit in (('mse', 0), ('l1', 1), ('sl1', 2)):
            for thres in (0.15, 0.1):
                r = HP._cre('fixture', 'if (e >= N * L) return;', n, 33, 12, idx='bbox12', crit=crit, thres=thres)
                x = HP.inputs(r)
                assert np.array_equal(x['idx'].reshape(12, 4).numpy(), g['cr_indices'])
                x['coords'] = coords.reshape(-1).clone()
                ref = HP.reference(r, x)
                key = '%s/%s/%g' % (tag, spec, thres)
                mask = ref['ws'][0].reshape(n, 12, 10)[..., 9]
                assert np.array_equal(mask.numpy(), g[key + '/mask'][..., 0].astype(np.float64)), key
                np.testing.assert_allclose(float(ref['loss'][0]), float(g[key + '/loss']), rtol=5e-6)
                want = g[key + '/grad'].reshape(-1)
                np.testing.assert_allclose(ref['dcoords'][0].numpy(), want, rtol=0,
                                           atol=5e-6 * max(1.0, float(np.abs(want).max())))


def test_planted_cross_ratios_are_exact_in_fp32():
    """Collinear 0, 1, 2, 3 eighths with target 4/3: cr = 1 in fp32, every gradient exactly 0; the square with target
    sqrt(2): cr = 2.  (0, 1, 3, 4 has cross ratio (3 x 3) / (2 x 4) = 9/8, not 4/3.)"""
    assert (3 * 3) / (2 * 4) != 4 / 3 and (2 * 2) / (1 * 3) == 4 / 3
    for r in EDGES:
        plant = r['opt'].get('plant')
        if r['name'] != HP.CRE or plant not in ('cr1', 'cr2', 'num0', 'four', 'thres_eq', 'den0'):
            continue
        x, ref = _case(r)
        emu = HP.emulate(r, x)
        ws32, ws64 = emu['ws'].reshape(-1, 10)[0], ref['ws'][0].reshape(-1, 10)[0]
        assert not ref['_undecided'], r['srcs']
        if plant == 'cr1':
            assert float(ws32[9]) == 1 and bool((ws32[:9] == 0).all()), (r['srcs'], ws32)
        elif r['opt'].get('exact0'):
            assert float(ws32[9]) == 1 and bool((ws32[:9] == 0).all()) and bool((ws64[:9] == 0).all()), (r['srcs'], ws64)
            assert bool((ref['ws'][1].reshape(-1, 10)[0] == 0).all())               # nothing allowed: exact
        elif plant == 'cr2':
            v1 = {0: 1.0, 1: 1.0, 2: 0.5}[r['s']['crit']]
            assert float(ws32[9]) == 1 and float(ws32[8]) == v1 and float(ws64[8]) == v1, (r['srcs'], ws32)
        elif plant == 'num0':
            assert float(ws64[9]) == 1 and bool((ws64[:8] == 0).all()) and float(ws64[8]) > 0, (r['srcs'], ws64)
            assert bool(torch.isfinite(ref['dcoords'][0]).all())
        elif plant == 'den0':
            assert float(ws64[9]) == 1 and not np.isfinite(float(ref['loss'][0]))
        else:
            assert bool((ws64 == 0).all()) and ref['_kept'] == 1, (r['srcs'], ws64)


def test_layout_references_are_the_host_packers():
    n = 0
    for r in SMALL:
        if r['name'] not in HP.PACKERS:
            continue
        x, ref = _case(r)
        want = ref['dst'][0]
        host = HP.host_pack(r, x)
        code, co, ci, taps = HP.pack_code(r)
        assert want.numel() == host.numel() == HP.layout_floats(code, co, ci, taps), (r['name'], r['s'])
        if r['opt'].get('content') == 'ints':     # (the host packers multiply by float64's 1 / 6: 1e-14 where U is 0)
            assert float((want.float() - host).abs().max()) < 1e-9, (r['name'], r['s'])
        else:
            assert torch.equal(want.float(), host), (r['name'], r['s'])
        if r['opt'].get('content') == 'ints':
            assert torch.equal(want, want.round()) and float(want.abs().max()) < 2 ** 24      # G g G^T: integers
        n += 1
    assert n > 50


# ---------------------------------------------------------------------------------------------------------------
# the emulations' ratios: where the constants come from
# ---------------------------------------------------------------------------------------------------------------
EXTRA_ULPS = {HP.APF: 2.0, HP.APB: 2.0, HP.CRE: 2.0 * 3, HP.PIX: 0.0}      # 2 per non-power-of-two division


def test_constants_are_four_times_the_emulations_worst_ratio():
    """cross_ratio: the six sqrtf feed only the mask; every value has three divisions on its path (by |BC|^2 |AD|^2, by
    target^2, by |PQ|^2).  avgpool: the division by k^2.  pixshuf: none (inv is a double, formed on the host)."""
    worst, where, left = {}, {}, {}
    for r in SMALL:
        if r['name'] in HP.PACKERS or r['name'] == HP.UNS:
            continue
        x, ref = _case(r)
        if ref.get('_undecided'):
            assert r['opt'].get('edge_mask'), 'undecided mask in a case that does not plant it: %s' % r['srcs']
            continue
        emu = HP.emulate(r, x)
        w, fails, lo = HP.check(r, emu, ref)
        assert not fails, (r['name'], r['s'], r['srcs'], fails)
        assert lo <= HP.L1_CAP, (r['srcs'], lo)
        left[r['name']] = max(left.get(r['name'], 0.0), lo)
        for a, v in w.items():
            k = (r['name'], a)
            if v >= worst.get(k, -1.0):
                worst[k], where[k] = v, '%s %s' % (r['s'], r['srcs'][0])
    print()
    for k in sorted(worst):
        print('%-24s %-8s emulation worst %.2f   C %g   (%s)' % (k[0], k[1], worst[k], HP.C_BOUND[k[0]], where[k]))
    for name, lo in sorted(left.items()):
        print('%-24s largest share of undecided elements in a case: %.5f (cap %g)' % (name, lo, HP.L1_CAP))
    for name in (HP.PIX, HP.APF, HP.APB, HP.CRE):
        top = max(v for k, v in worst.items() if k[0] == name)
        want = 4.0 * top + EXTRA_ULPS[name]
        assert want <= HP.C_BOUND[name] <= max(want * 1.25, want + 1.0), (name, top, want, HP.C_BOUND[name])


# ---------------------------------------------------------------------------------------------------------------
# coverage, from the request list and the kernels' text
# ---------------------------------------------------------------------------------------------------------------
def test_the_edge_list_reaches_every_path():
    live = [r for r in EDGES if not r['opt'].get('refuse')]
    pix = [r for r in live if r['name'] == HP.PIX]
    plans = [HP.pixshuf_plan(r) for r in pix]
    for vec in (False, True):                     # both template instances: one tile, several, a ragged last one
        mine = [p for p in plans if p[0] == vec]
        assert any(p[2] == 1 for p in mine), vec
        assert any(p[2] > 1 and p[3] == p[1] for p in mine), vec
        assert any(p[2] > 1 and p[3] < p[1] for p in mine), vec
    # both sides of every TW step the launcher can take for cs <= 1024
    steps = [cs for cs in range(4, 1028, 4) if HP.pixshuf_tw(cs) != HP.pixshuf_tw(cs - 4)]
    assert steps == [1016]
    for cs in steps:
        for up in (1, 2):
            assert {r['s']['cs'] for r in pix if r['s']['up'] == up} >= {cs - 4, cs}
    assert {(r['s']['crit'], 'tw' in r['null']) for r in pix} == {(c, t) for c in (0, 1, 2) for t in (False, True)}
    assert any(dict(r['opt'].get('off', ())).get('tgt') for r in pix) and any('dx' in r['null'] for r in pix)
    assert any(r['opt'].get('loss0') for r in pix)
    # stage 1 / stage 2 trips of a block
    nq = [min(p[1], r['s']['W']) * r['s']['cs'] // 4 for r, p in zip(pix, plans)]
    assert min(nq) < 256 and max(nq) > 512
    assert any(r['s']['C'] * r['s']['up'] ** 2 * min(p[1], r['s']['W']) > 4 * 256 for r, p in zip(pix, plans))
    # every layout code 0 .. 5, single and batched
    assert {HP.pack_code(r)[0] for r in live if r['name'] in HP.PACKERS} == set(range(6))
    assert {c for _, rows in HP.BATCH_EDGES for (_, _, _, c) in rows} == set(range(6))
    for _, rows in HP.BATCH_EDGES:
        HP.table_begins(rows)
    # every branch of egn_pack_matrix_f32
    mx = [r for r in EDGES if r['name'] == HP.PMX]
    assert {(r['s']['transpose'], r['s']['ld'] > (r['s']['cout'] if r['s']['transpose'] else r['s']['cin']))
            for r in mx if not r['opt'].get('refuse')} == {(0, False), (0, True), (1, False), (1, True)}
    assert {tuple(sorted(r['null'])) for r in mx if r['opt'].get('refuse')} >= {('src',), ('dst',), ()}
    # a second trip of each stride loop
    s_ = lambda name: [r['s'] for r in live if r['name'] == name]                # noqa: E731
    assert any(s['N'] * s['H'] * s['W'] * s['cs'] // 4 > HP.HEADS_GRID for s in s_(HP.UNS))
    assert any(s['N'] * (s['H'] // s['k']) * (s['W'] // s['k']) * s['cs'] // 4 > HP.HEADS_GRID for s in s_(HP.APF))
    assert any(s['N'] * s['H'] * s['W'] * s['cs'] // 4 > HP.HEADS_GRID for s in s_(HP.APB))
    units = lambda r: HP.layout_floats(*HP.pack_code(r)) // HP.unit_floats(HP.pack_code(r)[0])     # noqa: E731
    assert any(units(r) >= HP.PACK_ONE_GRID + 64 for r in live if r['name'] == HP.PMX)
    assert any(HP.table_begins(rows)[1] > HP.PACK_BATCH_GRID for _, rows in HP.BATCH_EDGES)
    cr = s_(HP.CRE)
    assert any(s['N'] * s['L'] > 512 for s in cr) and any(256 < s['N'] * s['L'] <= 512 for s in cr)
    assert any(s['N'] * s['K'] > 256 for s in cr)
    # a joint on three lines and one on none
    r = next(r for r in live if r['opt'].get('idx') == 'shared')
    idx = HP.cr_idx(r)
    assert int((idx == 0).any(1).sum()) >= 3 and not bool((idx == r['s']['K'] - 1).any())
    assert len({int(np.where(row == 0)[0][0]) for row in idx if (row == 0).any()}) >= 3
    assert int(idx.min()) >= 0 and all(int(HP.cr_idx(r).max()) < r['s']['K'] for r in live if r['name'] == HP.CRE)
    # avgpool: cropped windows, a divisor that is no power of two, k 1, both accumulate values
    ap = s_(HP.APB)
    assert any(s['H'] % s['k'] and s['W'] % s['k'] for s in ap) and any(s['k'] == 3 for s in ap)
    assert {s['accumulate'] for s in ap} == {0, 1} and any(s['k'] == 1 for s in ap) and {4, 260} <= {s['cs'] for s in ap}
    # the query grid holds accepted and refused shapes of both Winograd layouts, both directions
    grid = HP.query_grid()
    for name in (HP.PW2, HP.PW4):
        ans = {(bool(HP.layout_floats(*HP.pack_code(r))), r['s']['dgrad']) for r in grid if r['name'] == name}
        assert ans == {(True, 0), (True, 1), (False, 0), (False, 1)}
    print('\n%d edge requests (%d refusals), %d query-grid shapes, %d batch tables'
          % (len(EDGES), len(EDGES) - len(live), len(grid), len(HP.BATCH_EDGES)))


# ---------------------------------------------------------------------------------------------------------------
# the mutants
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mut', HP.MUTANTS)
def test_a_wrong_kernel_breaks_the_exact_case_or_the_bound(mut):
    flagged = []
    for r in SMALL:
        if r['name'] not in HP.mutant_targets(mut):
            continue
        x, ref = _case(r)
        if ref.get('_undecided'):
            continue
        _, fails, _ = HP.check(r, HP.emulate(r, x, mut), ref)
        if fails:
            flagged.append((r['srcs'][0], fails[0]))
    print('\n%s: flagged by %d requests%s' % (mut, len(flagged), ': ' + flagged[0][0] if flagged else ''))
    if mut in HP.BITS_ONLY:
        assert not flagged, 'believed visible only in the last bits, yet caught: say so in the docstring (%s)' % flagged[:2]
    else:
        assert flagged, mut


# ---------------------------------------------------------------------------------------------------------------
# the recorder, on a stand-in for the library
# ---------------------------------------------------------------------------------------------------------------
def test_recorder_keeps_names_doubles_nulls_and_alignment():
    class Stub(object):
        def __getattr__(self, name):
            return lambda *a: 0
    import ctypes as C
    with HP.HeadRecorder(handle=Stub()) as rec:
        rec.src = 'stub'
        L = _lib.lib()
        L.egn_cross_ratio_f32(C.c_void_p(4096), 3, 33, C.c_void_p(8192), 12, 4.0 / 3.0, 0.15, 2, 0.05, None,
                              C.c_void_p(12288), C.c_void_p(16384), None)
        L.egn_pixshuf_loss_f32(C.c_void_p(4096), C.c_void_p(8196), None, 2, 3, 18, 3, 2, 12, 0, 0.5, C.c_void_p(4096),
                               C.c_void_p(12288), None)
        L.egn_add_f32(None, None, None, 4, None)                 # not this sweep's: forwarded, not noted
    a, b = rec.notes
    assert a['s']['target_cr'] == 4.0 / 3.0 and a['s']['thres'] == float(np.float32(0.15)) and a['s']['L'] == 12
    assert a['null'] == frozenset(['dcoords']) and a['opt'] == {}
    assert b['opt'] == {'off': (('tgt', 1),)} and b['null'] == frozenset(['tw']) and b['alias'] == (('dx', 'x'),)
    assert HP.pixshuf_plan(dict(b, opt=b['opt']))[0] is False
    m = HP.T.merged(rec.notes + rec.notes)
    assert len(m) == 2 and m[0]['srcs'] == ['stub', 'stub']
