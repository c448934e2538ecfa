"""What tests/program_ops_sweep.py claims, as far as a machine without a GPU can hold it to it: the recorder finds the
seven kinds, the edge list points at kernel lines that exist, the constants are 4x what the emulations measure, the
exact inputs stay below 2^24, the checker flags every wrong kernel of ``MUTANTS``, and every op kind a program can
hold has a test file that owns it."""
import os

import pytest

import program_ops_sweep as P

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def edges():
    return P.merged(P.edge_requests())


def test_the_recorder_finds_all_seven_kinds_and_every_request_is_well_formed():
    ops, kinds = P.recorded_kinds()
    reqs = P.recorded_requests()
    per = {k: [r for r in reqs if r['kind'] == k] for k in P.KINDS}
    print('\nrecorded: %d ops of the seven kinds, %d distinct' % (len(ops), len(reqs)))
    for k in P.KINDS:
        print('   %-8s %3d distinct' % (k, len(per[k])))
        assert per[k], 'no %s op in any recording' % k
    assert {r['mode'] for r in per['decode']} == {0, 1, 2}
    assert {(r['fused'], r['res'], r['relu1']) for r in per['pwpair']} == set(P.PW_FORMS)
    assert any(r['M'] > P.pw_clamp(P.NOMINAL_G) for r in per['pwpair'])
    for r in reqs:
        assert r['srcs'] and r['lead'] == 0 and set(r['null']) <= set(P.IN_NAMES[r['kind']] + P.OUT_NAMES[r['kind']])
        q = P.replayed(r, P.NOMINAL_G)
        n = P.out_numel(q)
        assert all(v > 0 for v in n.values()) and set(n) == set(P.OUT_NAMES[r['kind']]) - set(r['null'])
        if r['kind'] == 'pwpair':
            assert q['M'] % 32 == 0 and 0 < q['M'] <= P.pw_clamp(P.NOMINAL_G)
            assert ('res' in r['null']) == (not r['res']) and ('hn' in r['null']) == (not r['fused'])
        elif r['kind'] == 'fuse':
            assert 1 <= len(r['shifts']) <= 4 and 0 in r['shifts'] and r['cs'] % 4 == 0 and r['C'] <= r['cs']
            assert all(r['H'] % (1 << s) == 0 and r['W'] % (1 << s) == 0 for s in r['shifts'])
        elif r['kind'] == 'pixshuf':
            assert r['cs'] >= r['C'] * r['up'] ** 2
        elif r['kind'] == 'ramps':
            assert r['c0'] + 2 <= r['cs']
        elif r['kind'] == 'decode':
            assert r['idx'] and not r['null']
        else:
            assert r['cs'] >= r['C']


def test_every_edge_request_names_a_line_of_its_kernel(edges):
    texts = {}
    for r in edges:
        name, line = r['line']
        texts.setdefault(name, P.kernel_text(name))
        assert line in texts[name], (r['kind'], r['srcs'][0], name, line)
    G = P.NOMINAL_G
    pw = [r for r in edges if r['kind'] == 'pwpair']
    assert {r['M'] for r in pw} == {32, 64, 32 * G, 32 * (G + 1), 32 * (2 * G + 3)}
    for M in {r['M'] for r in pw}:
        assert set(P.PW_FORMS) <= {(r['fused'], r['res'], r['relu1']) for r in pw if r['M'] == M}
    assert len({(r['fused'], r['res'], r['relu1']) for r in pw if r['M'] == 32 * (G + 1)}) == 8
    assert any(r['lead'] == 4 for r in pw)
    dec = [r for r in edges if r['kind'] == 'decode']
    assert {(r['N'], r['K'], r['H'], r['W']) for r in dec if r['idx']} == {s[0] for s in P.DECODE_SHAPES}
    vec = {(r['H'], r['W'], r['lead']): P.decode_vec_path(r) for r in dec}
    assert vec[(4, 4, 0)] and vec[(64, 64, 0)] and vec[(32, 128, 0)] and vec[(128, 32, 0)]
    assert not (vec[(1, 1, 0)] or vec[(5, 7, 0)] or vec[(64, 65, 0)] or vec[(128, 128, 0)] or vec[(6, 6, 1)])
    for k, total in (('fuse', lambda r: r['N'] * r['H'] * r['W'] * r['cs'] // 4),
                     ('to_nhwc', lambda r: r['N'] * r['H'] * r['W'] * r['cs'] // 4),
                     ('to_nchw', lambda r: r['N'] * r['C'] * r['H'] * r['W']),
                     ('pixshuf', lambda r: r['N'] * r['C'] * r['H'] * r['W'] * r['up'] ** 2),
                     ('ramps', lambda r: r['N'] * r['H'] * r['W'])):
        big = [total(r) for r in edges if r['kind'] == k and total(r) > P.GRID_CAP]
        assert big and all(t % P.GRID_CAP and t < 2 * P.GRID_CAP for t in big), (k, big)
    assert any(r['c0'] + 2 == r['cs'] for r in edges if r['kind'] == 'ramps')


def test_the_emulations_stay_at_a_quarter_of_their_constants(edges):
    """The table of the helper's docstring."""
    worst = {}
    for r in edges:
        if r['kind'] not in ('pwpair', 'decode'):
            continue
        q = P.emulated(r)
        x = P.inputs(q, 'rounding')
        w, fails, notes = P.check(q, 'rounding', x, P.emulate(q, 'rounding', x))
        assert not fails, (r['srcs'][0], fails)
        for name, v in ((('decode mode %d' % r['mode'], w),) if r['kind'] == 'decode' else
                        (('pwpair out', notes['out']), ('pwpair hn', notes.get('hn', 0.0)))):
            if v >= worst.get(name, (0.0, ''))[0]:
                worst[name] = (v, '%s %s' % ({k: r[k] for k in ('M', 'fused', 'res', 'relu1', 'N', 'K', 'H', 'W', 'mode',
                                                                  'content') if k in r}, r['srcs'][0]))
    print()
    for name, (v, where) in sorted(worst.items()):
        print('%-14s worst emulation ratio %.2f   %s' % (name, v, where))
    assert max(worst['pwpair out'][0], worst['pwpair hn'][0]) <= P.C_PW / 4
    assert max(worst['decode mode 1'][0], worst['decode mode 2'][0]) <= P.C_DEC / 4


def test_the_exact_inputs_stay_below_two_to_the_24(edges):
    seen = set()
    for r in edges:
        if r['kind'] not in ('pwpair', 'fuse') or (r['kind'] == 'pwpair' and r['lead']):
            continue
        q = P.emulated(r)
        x = P.inputs(q, 'exact')
        for t in x.values():
            assert bool((t == t.round()).all()) and float(t.abs().max()) <= 4
        if r['kind'] == 'pwpair':
            (o64, A), hn = P.pw_reference(q, x)
            assert float(A.max()) <= 64 * 16 + 8
            if hn is not None:
                assert float(hn[1].max()) < 2 ** 24
                seen.add('hn')
        w, fails, _ = P.check(q, 'exact', x, P.emulate(q, 'exact', x))
        assert not fails and w == 0.0, (r['srcs'][0], fails)
    assert 'hn' in seen


def test_the_mixed_sign_maps_are_conditioned_below_8(edges):
    mixed = [r for r in edges if r['kind'] == 'decode' and r['content'] == 'mixed']
    assert len(mixed) == len(P.DECODE_SHAPES) and all(r['mode'] == 2 for r in mixed)
    worst = max(P.mixed_conditioning(r, P.inputs(r, 'rounding')['hm']) for r in mixed)
    print('\nworst sum|v| / |sum v| of the mixed-sign maps: %.2f' % worst)
    assert worst <= 8.0
    for r in edges:
        if r['kind'] == 'decode' and r['mode'] == 2 and r['content'] not in ('mixed', 'nonpos', 'neginf_some',
                                                                             'all_neginf'):
            assert float(P.inputs(r, 'rounding')['hm'].min()) >= 0.0


def test_the_decode_bound_is_below_the_older_tolerances(edges):
    for mode, old in ((1, 1e-3), (2, 1e-4)):
        r = [q for q in edges if q['kind'] == 'decode' and (q['H'], q['W'], q['mode'], q['content']) ==
             (64, 64, mode, 'peaks')][0]
        b = float(P.decode_reference(r, P.inputs(r, 'rounding')['hm'])['bound'].max())
        print('\nmode %d, 64 x 64 peaks: bound %.3g pixels (tests/test_gpu_decode.py: %g)' % (mode, b, old))
        assert b < old


@pytest.mark.parametrize('kind', [k for k in P.KINDS if P.MUTANTS[k]])
def test_the_checker_flags_every_wrong_kernel(kind, edges):
    mine = [r for r in edges if r['kind'] == kind]
    if kind == 'pwpair':            # one request per form at two tiles and at the eight-form size, on 64 rows
        mine = [dict(r, M=64) for r in mine if r['M'] == 32 * (P.NOMINAL_G + 1) and not r['lead']]
    for mut in P.MUTANTS[kind]:
        hit = 0
        for r in mine:
            if not P.mutant_applies(mut, r):
                continue
            flagged = False
            for case in P.cases_of(r):
                x = P.inputs(r, case)
                assert not P.check(r, case, x, P.emulate(r, case, x))[1], (r['srcs'][0], case)
                flagged = flagged or bool(P.check(r, case, x, P.emulate(r, case, x, mut))[1])
            assert flagged, '%s not flagged on %s' % (mut, r['srcs'][0])
            hit += 1
        print('%s / %s: flagged on %d requests' % (kind, mut, hit))
        assert hit, '%s: no edge request it applies to' % mut


def test_every_op_kind_a_program_can_hold_has_an_owner():
    pushed = P.pushed_kinds() - {'fork', 'join'}
    assert pushed == set(P.OWNERS), (sorted(pushed), sorted(P.OWNERS))
    for kind, name in P.OWNERS.items():
        assert os.path.isfile(os.path.join(HERE, name)), (kind, name)
    assert {P.OWNERS[k] for k in P.KINDS} == {P.GPU_TEST}
    seen = set()
    for prec in P.PRECISIONS:
        _, kinds = P.recorded_kinds(prec, modes=(1,))
        kinds = kinds - {'fork', 'join'}
        assert kinds <= set(P.OWNERS), (prec, sorted(kinds - set(P.OWNERS)))
        seen |= kinds
    print('\nkinds recorded over %s: %s' % (', '.join(P.PRECISIONS), ', '.join(sorted(seen))))
    assert set(P.KINDS) <= seen and {'conv', 'convh', 'convh2', 'convhx'} <= seen      # ('convpair': by the device's tuner)
