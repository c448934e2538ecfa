"""Every launch of csrc/heads.hip, csrc/cross_ratio.hip and csrc/filter_pack.hip that a native training step makes,
and the edges of their kernels and launchers, against float64 (tests/head_pack_sweep.py has the requests, the
references and the bounds).  Per launch:
  1. |got - want64| <= C_BOUND[entry] * 2^-24 * A for every output, exact where A = 0, not finite where float64 is not;
  2. every element written (outputs pre-filled with NaN), the zero padding of a packed filter included;
  3. no write outside the outputs (sweep_guards bands), the cross-ratio workspace a band of exactly
     egn_cross_ratio_ws_bytes;
  4. inputs unchanged bit for bit, with NaN in front of and behind them and wherever the kernel must not look;
  5. the same bits from a second launch (the pixshuf loss scalar, added atomically by many blocks: twice the bound);
  6. a size query equal to what the launch writes; a refused request returns EGN_E_BADARG and writes nothing.
The batch packer's tables (the recorded one, read back from the device, and the edge list's) are replayed into guarded
NaN-filled buffers; each descriptor's output equals, bit for bit, what the single-filter entry point writes."""
import ctypes as C

import numpy as np
import pytest
import torch

import head_pack_sweep as HP
from egonet_amd import _lib
from egonet_amd.train_common import PackedFilters
from sweep_guards import _guarded, _guards_intact

pytestmark = pytest.mark.gpu

LEAD, TAIL = 16, 64
_DT = {'loss': torch.float64, 'idx': torch.int32}
_PER = {}


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _input(t, off):
    """(whole, body): the operand with LEAD + off NaN floats in front of it and TAIL behind."""
    fill = float('nan') if t.dtype.is_floating_point else 0
    whole = torch.full((LEAD + off + t.numel() + TAIL,), fill, dtype=t.dtype, device='cuda')
    body = whole[LEAD + off:LEAD + off + t.numel()]
    body.copy_(t)
    return whole, body


def _note(name, origin, launches, worst, where):
    ent = _PER.setdefault(name, dict(recorded=0, edge=0, launches=0, worst=0.0, where=''))
    ent[origin] += 1
    ent['launches'] += launches
    for a, v in worst.items():
        if v >= ent['worst']:
            ent['worst'], ent['where'] = v, '%s %s' % (a, where)


def _call(r, ptrs):
    args = []
    for a, role in HP.ARGS[r['name']]:
        args.append(r['s'][a] if role is None else ptrs.get(a))
    args.append(_lib.current_stream())
    rc = getattr(_lib.lib(), r['name'])(*args)
    torch.cuda.synchronize()
    return rc


def _refused(r):
    """A request the launcher must reject on the host: EGN_E_BADARG, every operand's bits as they were."""
    off = dict(r['opt'].get('off', ()))
    bufs, ptrs = {}, {}
    for a, role in HP.ARGS[r['name']]:
        if role is None or a in r['null']:
            continue
        dt = _DT.get(a, torch.float32)
        whole = (torch.zeros(1 << 18, dtype=dt, device='cuda') if dt == torch.int32
                 else torch.full((1 << 18,), float('nan'), dtype=dt, device='cuda'))
        bufs[a] = whole
        ptrs[a] = C.c_void_p(whole.data_ptr() + 4 * off.get(a, 0))
    keep = {a: _bits(b).clone() for a, b in bufs.items()}
    rc = _call(r, ptrs)
    fails = []
    if rc != -1:
        fails.append('returned %d, want EGN_E_BADARG' % rc)
    for a, b in bufs.items():
        if not torch.equal(_bits(b), keep[a]):
            fails.append('%s written by a refused call' % a)
    return fails


def _replay(r):
    """Both launches of one request -> ({output: worst ratio}, [failures])."""
    L = _lib.lib()
    name, s = r['name'], r['s']
    if r['alias']:
        return {}, ['aliased operands %s: the sweep has no replay for them' % (r['alias'],)]
    x = HP.inputs(r)
    ref = HP.reference(r, x)
    off = dict(r['opt'].get('off', ()))
    fails, ins, outs, ptrs = [], {}, {}, {}
    for a, role in HP.ARGS[name]:
        if role is None or a in r['null']:
            continue
        if role == 'in':
            whole, body = _input(x[a], off.get(a, 0))
            ins[a] = (whole, _bits(whole).clone())
            ptrs[a] = _lib.ptr(body)
            assert body.data_ptr() % 16 == 4 * (off.get(a, 0) % 4)
        else:
            if role == 'ws':
                numel = L.egn_cross_ratio_ws_bytes(s['N'], s['L']) // 4
                if numel != ref[a][0].numel():
                    fails.append('egn_cross_ratio_ws_bytes says %d floats, the kernel writes %d' % (numel, ref[a][0].numel()))
            else:
                numel = ref[a][0].numel()
            whole, body = _guarded(numel, _DT.get(a, torch.float32), None)
            outs[a] = (whole, body, x[a].cuda() if a in x else None)
            ptrs[a] = _lib.ptr(body)
    if name in HP.PACKERS:
        q = HP.query(L, r)
        if q is not None and q != ref['dst'][0].numel():
            fails.append('the size query says %d floats, the layout has %d' % (q, ref['dst'][0].numel()))
    undecided = ref.get('_undecided', False)
    if undecided and not r['opt'].get('edge_mask'):
        fails.append('a line within rounding of the threshold in a case that does not plant one')
    worst, first = {}, {}
    for rep in range(2):
        for whole, body, init in outs.values():
            if init is not None:
                body.copy_(init)
            else:
                body.fill_(float('nan'))
        rc = _call(r, ptrs)
        if rc != 0:
            fails.append('launch %d returned %d' % (rep, rc))
            break
        for a, (whole, was) in ins.items():
            if not torch.equal(_bits(whole), was):
                fails.append('input %s changed' % a)
        got = {}
        for a, (whole, body, init) in outs.items():
            if not _guards_intact(whole):
                fails.append('write outside %s' % a)
            got[a] = body.cpu()
            if not undecided and bool((~torch.isfinite(got[a]) & torch.isfinite(ref[a][0].to(got[a].dtype))).any()):
                fails.append('%s: elements not written / not finite' % a)
        if undecided:
            if not all(bool(torch.isfinite(got[a]).all()) for a in got):
                fails.append('an output not written')
        elif rep == 0:
            worst, f, _ = HP.check(r, got, ref)
            fails += f
        if rep == 0:
            first = got
        else:
            for a in got:
                if a == 'loss' and name == HP.PIX:
                    _, f, _ = HP.check(r, {'loss': got[a]}, {'loss': ref['loss']}, scale=2.0)
                    fails += ['second launch: ' + m for m in f]
                elif not torch.equal(_bits(got[a]), _bits(first[a])):
                    fails.append('second launch: different bits in %s' % a)
    return worst, fails


def _sweep(reqs, origin):
    fails = []
    for r in reqs:
        tag = '%s %s null %s opt %s (%s: %s)' % (r['name'], r['s'], sorted(r['null']), r['opt'], origin, r['srcs'][0])
        if r['opt'].get('refuse'):
            f = _refused(r)
            _note(r['name'], origin, 1, {}, '')
        else:
            w, f = _replay(r)
            _note(r['name'], origin, 2, w, '%s %s' % (origin, r['srcs'][0]))
        fails += ['%s: %s' % (tag, m) for m in f]
    torch.cuda.empty_cache()
    return fails


def _print(names):
    for k in names:
        v = _PER.get(k)
        if v:
            print('%-38s %3d recorded %3d edge %4d launches  worst %6.2f (C %4.1f)  %s'
                  % (k, v['recorded'], v['edge'], v['launches'], v['worst'], HP.C_BOUND.get(k, float('nan')), v['where']))


@pytest.fixture(scope='module')
def recorded():
    return HP.recorded_requests('cuda')


def test_every_recorded_launch_matches_float64(recorded):
    notes, reqs, tables = recorded
    fails = _sweep(reqs, 'recorded')
    print('\nhead / pack sweep: %d recorded launches, %d distinct' % (len(notes), len(reqs)))
    _print(HP.LAUNCHING)
    assert not fails, '%d failures:\n%s' % (len(fails), '\n'.join(fails[:40]))
    seen = {n['name'] for n in notes}
    assert set(HP.LAUNCHING) - set(HP.EDGE_ONLY) <= seen, sorted(set(HP.LAUNCHING) - seen)
    pix = [r for r in reqs if r['name'] == HP.PIX]
    assert {r['s']['up'] for r in pix} >= {2, 4} and {('tw' in r['null']) for r in pix} == {True, False}
    assert {r['s']['crit'] for r in reqs if r['name'] == HP.CRE} == {0, 2}
    assert tables and all(n > 1 for _, n, _, _ in tables)


@pytest.mark.parametrize('name', [n for n in HP.LAUNCHING if n != HP.BATCH])
def test_every_edge_request_matches_float64(name):
    reqs = [r for r in HP.edge_requests() if r['name'] == name]
    assert reqs
    fails = _sweep(reqs, 'edge')
    print()
    _print([name])
    assert not fails, '%d failures:\n%s' % (len(fails), '\n'.join(fails[:40]))


def test_size_queries_and_launches_agree_around_the_accepted_shapes():
    L = _lib.lib()
    fails, yes, no = [], 0, 0
    for r in HP.query_grid():
        code, co, ci, taps = HP.pack_code(r)
        fl = HP.layout_floats(code, co, ci, taps)
        q = HP.query(L, r)
        tag = '%s %s' % (r['name'], r['s'])
        if fl:
            yes += 1
            if q != fl:
                fails.append('%s: the query says %d, the layout has %d floats' % (tag, q, fl))
            _, f = _replay(r)
        else:
            no += 1
            if q > 0:       # (not launched: the buffers below are sized for a call that is refused)
                fails.append('%s: the query says %d for a shape the layout does not take' % (tag, q))
                continue
            f = _refused(r)
        fails += ['%s: %s' % (tag, m) for m in f]
    print('\nquery grid: %d accepted shapes packed and checked, %d refused' % (yes, no))
    assert yes and no and not fails, '\n'.join(fails[:40])


# ---------------------------------------------------------------------------------------------------------------
# the batch packer
# ---------------------------------------------------------------------------------------------------------------
def _single(w, co, ci, taps, code, dst):
    L, st = _lib.lib(), _lib.current_stream()
    dg = code & HP.FP_DGRAD
    if code & HP.FP_WINO4:
        return L.egn_wino4_pack_weight_f32(_lib.ptr(w), co, ci, dg, _lib.ptr(dst), st)
    if code & HP.FP_WINO2:
        return L.egn_wino_pack_weight_f32(_lib.ptr(w), co, ci, dg, _lib.ptr(dst), st)
    return L.egn_pack_conv_weight_f32(_lib.ptr(w), co, ci, taps, 1, dg, _lib.ptr(dst), st)


def _run_table(rows, total):
    """rows [(Cout, Cin, taps, code, begin)] -> failures."""
    L = _lib.lib()
    g = torch.Generator().manual_seed(len(rows))
    weights, bufs, fails = {}, [], []
    desc = np.zeros(len(rows), dtype=np.dtype(PackedFilters._DESC, align=True))
    if desc.dtype.itemsize != L.egn_pack_desc_bytes():
        return ['egn_pack_desc_bytes %d, the table has %d per row' % (L.egn_pack_desc_bytes(), desc.dtype.itemsize)]
    end = 0
    for i, (co, ci, taps, code, begin) in enumerate(rows):
        if (co, ci, taps) not in weights:
            weights[(co, ci, taps)] = torch.randn(co * ci * taps, generator=g).cuda()
        w = weights[(co, ci, taps)]
        fl = HP.layout_floats(code, co, ci, taps)
        if not fl or begin != end:
            fails.append('row %d %s: %s' % (i, rows[i], 'no such layout' if not fl else 'begin is not the running sum %d' % end))
            return fails
        end += fl // HP.unit_floats(code)
        whole, body = _guarded(fl, torch.float32, float('nan'))
        bufs.append((whole, body))
        desc[i] = (w.data_ptr(), body.data_ptr(), co, ci, taps, code, begin)
    if end != total:
        return ['total %d, the rows have %d units' % (total, end)]
    table = torch.from_numpy(desc.view(np.uint8)).cuda()
    keep = table.clone()
    for rep in range(2):
        rc = L.egn_pack_conv_weights_batch_f32(_lib.ptr(table), len(rows), total, _lib.current_stream())
        torch.cuda.synchronize()
        if rc != 0:
            return ['launch returned %d' % rc]
    if not torch.equal(table, keep):
        fails.append('the table changed')
    one = {}
    for i, (co, ci, taps, code, begin) in enumerate(rows):
        whole, body = bufs[i]
        if not _guards_intact(whole):
            fails.append('row %d %s: write outside its filter' % (i, rows[i]))
        k = (co, ci, taps, code)
        if k not in one:
            one[k] = torch.full_like(body, float('nan'))
            rc = _single(weights[(co, ci, taps)], co, ci, taps, code, one[k])
            if rc != 0:
                fails.append('row %d %s: the single entry returned %d' % (i, rows[i], rc))
                continue
        if bool(torch.isnan(body).any()):
            fails.append('row %d %s: %d floats not written' % (i, rows[i], int(torch.isnan(body).sum())))
        elif not torch.equal(_bits(body), _bits(one[k])):
            fails.append('row %d %s: differs from the single entry point' % (i, rows[i]))
    torch.cuda.synchronize()
    del bufs, weights, one
    torch.cuda.empty_cache()
    return fails


def test_recorded_batch_table_packs_what_the_single_entries_pack(recorded):
    _, _, tables = recorded
    fails = []
    for src, n, total, rows in tables:
        assert len(rows) == n
        codes = sorted({c for (_, _, _, c, _) in rows})
        print('\n%s: %d descriptors, %d units, layout codes %s' % (src, n, total, codes))
        fails += ['%s: %s' % (src, m) for m in _run_table(rows, total)]
    assert not fails, '\n'.join(fails[:40])
    assert any({c for (_, _, _, c, _) in rows} >= {0, 1} for _, _, _, rows in tables)


@pytest.mark.parametrize('case', range(len(HP.BATCH_EDGES)))
def test_batch_edge_tables(case):
    why, rows = HP.BATCH_EDGES[case]
    rows, total = HP.table_begins(rows)
    fails = _run_table(rows, total)
    assert not fails, '%s:\n%s' % (why, '\n'.join(fails[:40]))


def test_batch_packer_refusals_launch_nothing():
    L, st = _lib.lib(), _lib.current_stream()
    rows, total = HP.table_begins(HP.BATCH_EDGES[0][1])
    co, ci, taps, code, _ = rows[0]
    w = torch.randn(co * ci * taps).cuda()
    whole, body = _guarded(HP.layout_floats(code, co, ci, taps), torch.float32, float('nan'))
    desc = np.zeros(1, dtype=np.dtype(PackedFilters._DESC, align=True))
    desc[0] = (w.data_ptr(), body.data_ptr(), co, ci, taps, code, 0)
    table = torch.from_numpy(desc.view(np.uint8)).cuda()
    assert L.egn_pack_conv_weights_batch_f32(None, 1, total, st) == -1                  # NULL table
    assert L.egn_pack_conv_weights_batch_f32(_lib.ptr(table), 0, total, st) == -1       # n = 0
    assert L.egn_pack_conv_weights_batch_f32(_lib.ptr(table), 1, 0, st) == -1           # total = 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(body).all()) and _guards_intact(whole)
    assert L.egn_pack_conv_weights_batch_f32(_lib.ptr(table), 1, total, st) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(body).any()) and _guards_intact(whole)
