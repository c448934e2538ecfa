"""Every launch of csrc/train_ops.hip that a native training step makes, and the edges of the kernels' thread mappings,
against float64.

The requests are those of tests/train_ops_sweep.py: what the recorded steps launch (BatchNorm statistics, the fused
BatchNorm + activation + dropout forward / backward, column sums, the loss criteria, the fuse layer's backward, zero
insertion, the optimizers, the step counters), each distinct one replayed through the same entry point with the same
NULL pattern and the same aliasing, and the hand-written edge list.  Every launch is checked for:
  1. |got - want64| <= C_BOUND[entry] * 2^-24 * A for every output, the loss scalar included (train_ops_sweep.reference);
  2. every element written (outputs pre-filled with NaN); pad columns cols <= c < ld exactly 0 for y, dz and dres (the
     kernels write whole float4 groups), left as they were for dpred (the loss kernels walk the [rows, cols] view only);
  3. no write outside the outputs, the workspace included (sentinel guard bands, bit-identical after);
  4. the same bits from a second launch (the loss scalar excepted: blocks add to it atomically in double, so both
     launches are held to the bound);
  5. inputs unchanged bit for bit, except where the request aliases them;
  6. for the dropout variants, a kept share within 4 sigma of the binomial around 1 - p.
A summary per entry point (requests, launches, worst |err| / (2^-24 A) and where) is printed with the achieved
relative variance error at column offsets of 0, 3 and 30 sigma, and written as JSON to train_ops_sweep.json in the
directory EGONET_AMD_PARITY_DIR names, if it is set.
"""
import json
import os
import time

import pytest
import torch

import train_ops_sweep as T
from egonet_amd import _lib
from sweep_guards import _guarded, _guards_intact

pytestmark = pytest.mark.gpu

_DTYPE = {'loss': torch.float64, 'zero_f64': torch.float64, 'step_dev': torch.int32}


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _replay(r, x=None):
    """Both launches of one request.  Returns ({output: worst ratio}, [failure strings], {output: what the first launch
    left}, figures about the case)."""
    L = _lib.lib()
    name, s = r['name'], r['s']
    fails, figs = [], {}
    if x is None:
        x = T.inputs(r)
    xd = {k: v.cuda() for k, v in x.items()}
    ref = T.reference(r, xd)
    # conditions on the case itself, from the reference alone, before the kernel's output is looked at
    if ref.get('_left_out', 0.0) > T.GATE_CAP:
        return {}, ['%.3f of the columns hold an undecided ReLU gate (cap %.2f)' % (ref['_left_out'], T.GATE_CAP)], {}, figs
    if '_left_out' in ref:
        figs['left_out'] = ref['_left_out']
    p = s.get('p')
    if p and '_kept' in ref:
        nel = s['rows'] * s['cols'] if 'rows' in s else s['n']
        figs['kept'] = ref['_kept']
        if abs(ref['_kept'] - (1 - p)) > 4 * (p * (1 - p) / nel) ** 0.5:
            fails.append('kept share %.4f of %d elements, p = %g' % (ref['_kept'], nel, p))
    leader = {}
    for grp in r['alias']:
        lead = next((a for a in grp if a in xd), grp[0])
        for a in grp:
            leader[a] = lead
    roles = dict(T.ARGS[name])
    written = {leader.get(a, a) for a, role in T.ARGS[name] if role in ('out', 'io', 'ws') and a not in r['null']}
    bufs = {}          # leader -> (whole, body, initial content or None = NaN)
    for a, role in T.ARGS[name]:
        if role is None or a in r['null'] or leader.get(a, a) in bufs:
            continue
        lead = leader.get(a, a)
        init = xd.get(lead)
        if init is not None:
            numel, dt = init.numel(), init.dtype
        elif role == 'ws':
            numel, dt = L.egn_colreduce_ws_bytes(s['cols']) // 4, torch.float32
        else:
            v = ref[a][2]['view']
            numel, dt = (v[0] * v[1] if v else ref[a][0].numel()), _DTYPE.get(a, torch.float32)
        whole, body = _guarded(numel, dt, None)
        bufs[lead] = (whole, body[:numel], None if init is None else init.reshape(-1))
    args = []
    for a, role in T.ARGS[name]:
        if role is None:
            args.append(s[a])
        else:
            args.append(None if a in r['null'] else _lib.ptr(bufs[leader.get(a, a)][1]))
    args.append(_lib.current_stream())
    outs = [a for a, role in T.ARGS[name] if role in ('out', 'io') and a not in r['null']]
    worst, first = {}, {}
    for rep in range(2):
        for whole, body, init in bufs.values():
            if init is not None:
                body.copy_(init)
            elif body.dtype.is_floating_point:
                body.fill_(float('nan'))
            else:
                body.fill_(-1)
        rc = getattr(L, name)(*args)
        torch.cuda.synchronize()
        if rc != 0:
            fails.append('launch %d returned %d (%s)' % (rep, rc, L.egn_strerror(rc).decode()))
            break
        for a, (whole, body, init) in bufs.items():
            if not _guards_intact(whole):
                fails.append('write outside %s' % a)
            if a not in written and not torch.equal(_bits(body), _bits(init)):
                fails.append('input %s changed' % a)
        got = {}
        for a in outs:
            body = bufs[leader.get(a, a)][1]
            want, A, how = ref[a]
            if how['view']:
                rows, ld, cols = how['view']
                m = body.view(rows, ld)
                got[a] = m[:, :cols]
                if rep == 0 and ld > cols:
                    if how['pad'] == 'zero' and bool((m[:, cols:] != 0).any()):
                        fails.append('%s: pad columns not 0' % a)
                    if how['pad'] == 'untouched' and not bool(torch.isnan(m[:, cols:]).all()):
                        fails.append('%s: pad columns written' % a)
            else:
                got[a] = body
        if rep == 0:
            for a in outs:
                if got[a].dtype.is_floating_point and not bool(torch.isfinite(got[a]).all()):
                    fails.append('%s: %d elements not written / not finite' % (a, int((~torch.isfinite(got[a])).sum())))
            worst = T.worst_ratios(got, {a: ref[a] for a in outs})
            for a, w in worst.items():
                if not w <= T.C_BOUND[name]:
                    fails.append('%s: error %.2f x 2^-24 A > %g' % (a, w, T.C_BOUND[name]))
            first = {a: got[a].clone() for a in outs}
            if r['opt'].get('offsets'):
                rows = s['rows']
                var64 = ref['_rel_var'][0]
                rel = ((got['var_unbiased'].double() * (rows - 1) / rows - var64).abs() / var64)
                figs['rel_var'] = [float(rel[k::3].max()) for k in range(3)]
        else:
            for a in outs:
                if a == 'loss':
                    w = T.worst_ratios({a: got[a]}, {a: ref[a]})[a]
                    if not w <= T.C_BOUND[name]:
                        fails.append('second launch: loss error %.2f x 2^-24 A' % w)
                elif not torch.equal(_bits(got[a]), _bits(first[a])):
                    fails.append('second launch: different bits in %s' % a)
    return worst, fails, first, figs


def _replay_counters(r):
    """egn_step_counters_i64: a device table of the counters' addresses; every counter += 1, the accumulator = 0."""
    L = _lib.lib()
    n = r['s']['n']
    x = T.inputs(r)
    fails = []
    vwhole, vals = _guarded(max(n, 1), torch.int64, None)
    twhole, table = _guarded(max(n, 1), torch.int64, 0)
    awhole, acc = _guarded(1, torch.float64, None)
    if n:
        table.copy_(vals.data_ptr() + 8 * torch.arange(n, dtype=torch.int64, device='cuda'))
    keep = table.clone()
    for rep in range(2):
        vals.fill_(-7)
        if n:
            vals.copy_(x['counters'].cuda())
        acc.fill_(3.5)
        rc = L.egn_step_counters_i64(_lib.ptr(table) if n else None, n, None if 'zero_f64' in r['null'] else _lib.ptr(acc),
                                     _lib.current_stream())
        torch.cuda.synchronize()
        if rc != 0:
            fails.append('launch %d returned %d' % (rep, rc))
            break
        if not (_guards_intact(vwhole) and _guards_intact(twhole) and _guards_intact(awhole)):
            fails.append('write outside the counters / the table / the accumulator')
        if n and not torch.equal(vals, x['counters'].cuda() + 1):
            fails.append('%d counters not incremented by exactly one' % int((vals != x['counters'].cuda() + 1).sum()))
        if not n and int(vals[0]) != -7:
            fails.append('a counter written with n = 0')
        if not torch.equal(table, keep):
            fails.append('the address table changed')
        want = 3.5 if 'zero_f64' in r['null'] else 0.0
        if float(acc[0]) != want:
            fails.append('accumulator %r, want %r' % (float(acc[0]), want))
    return {'counters': 0.0}, fails, {}, {}


def _chain(name):
    """Five launches from zero state, each checked against one float64 step from the state the launch before left:
    the counter's increment, SGD's first-step rule (state[0] <= 1) and a learning rate changed in device memory."""
    n = 5000 + 77
    kw = dict(egn_adam_step_dev_f32=dict(beta1=0.9, beta2=0.999, eps=1e-8),
              egn_adam_l2_step_dev_f32=dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2),
              egn_sgd_step_dev_f32=dict(momentum=0.9, weight_decay=1e-3))[name]
    r = T._req(name, 'five-launch chain', opt=dict(step0=0, keep_n=1), n=n, **kw)
    x = T.inputs(r)
    g = torch.Generator().manual_seed(11)
    worst, fails = {}, []
    for k, lr in enumerate((1e-3, 1e-3, 5e-4, 5e-4, 2e-3)):
        x['g'] = torch.randn(n, generator=g) * 10.0 ** (k - 3)
        x['lr_dev'] = torch.tensor([lr], dtype=torch.float32)
        w, f, got, _ = _replay(r, x)
        fails += ['launch %d: %s' % (k + 1, m) for m in f]
        for a, v in w.items():
            worst[a] = max(worst.get(a, 0.0), v)
        if f:
            break
        for a, v in got.items():
            x[a] = v.cpu()
        if int(x['step_dev'][0]) != k + 1:
            fails.append('launch %d: counter %d' % (k + 1, int(x['step_dev'][0])))
    return r, worst, fails


@pytest.fixture(scope='module')
def recorded():
    t0 = time.time()
    notes, reqs = T.recorded_requests('cuda')
    return notes, reqs, time.time() - t0


def test_every_training_op_launch_matches_float64(recorded):
    notes, reqs, t_collect = recorded
    t0 = time.time()
    per, fails, rel_var = {}, [], None
    n_launch = 0
    todo = [('recorded', r) for r in reqs] + [('edge', r) for r in T.edge_requests()]
    for origin, r in todo:
        name = r['name']
        ent = per.setdefault(name, dict(recorded=0, edge=0, launches=0, worst=0.0, where='', left_out=0.0))
        ent[origin] += 1
        if name not in T.ARGS:
            fails.append('%s (%s): recorded, but the sweep has no reference for it' % (name, r['srcs'][0]))
            continue
        try:
            w, f, _, figs = (_replay_counters if name == 'egn_step_counters_i64' else _replay)(r)
        except Exception as e:       # a request the sweep cannot replay is a failure of its own; a device error ends it
            if 'hip' in str(e).lower():
                raise
            w, f, figs = {}, ['%s: %s' % (type(e).__name__, e)], {}
        ent['launches'] += 2
        n_launch += 2
        ent['left_out'] = max(ent['left_out'], figs.get('left_out', 0.0))
        rel_var = figs.get('rel_var', rel_var)
        for a, v in w.items():
            if v >= ent['worst']:
                ent['worst'], ent['where'] = v, '%s %s %s' % (a, origin, r['srcs'][0])
        fails += ['%s %s null %s alias %s (%s %s): %s' % (name, r['s'], sorted(r['null']), r['alias'], origin,
                                                           r['srcs'][0], m) for m in f]
    for name in T.OPTIMIZERS:
        r, w, f = _chain(name)
        ent = per[name]
        ent['edge'] += 1
        ent['launches'] += 10
        n_launch += 10
        for a, v in w.items():
            if v >= ent['worst']:
                ent['worst'], ent['where'] = v, '%s edge five-launch chain' % a
        fails += ['%s chain: %s' % (name, m) for m in f]
    torch.cuda.empty_cache()
    wall = time.time() - t0
    clamped = sorted({(r['name'], r['opt']['clamped_from'], r['s']['n']) for r in reqs if 'clamped_from' in r['opt']})
    summary = dict(recorded_launches=len(notes), distinct_recorded=len(reqs), edge_requests=len(todo) - len(reqs),
                   launches_checked=n_launch, collect_s=round(t_collect, 1), sweep_s=round(wall, 1),
                   clamped=[dict(entry=a, recorded_n=b, replayed_n=c) for a, b, c in clamped],
                   entries={k: dict(v, worst=round(v['worst'], 2), bound=T.C_BOUND.get(k)) for k, v in sorted(per.items())},
                   relative_variance_error_at_0_3_30_sigma=rel_var, failures=fails[:200])
    print('\ntraining-ops sweep: %d recorded launches (%d distinct), %d edge requests, %d checked launches, '
          '%.0f s + %.0f s collection' % (len(notes), len(reqs), len(todo) - len(reqs), n_launch, wall, t_collect))
    for k, v in sorted(per.items()):
        print('%-28s %4d recorded %4d edge %5d launches  worst %6.2f (C %4.1f)  %s'
              % (k, v['recorded'], v['edge'], v['launches'], v['worst'], T.C_BOUND.get(k, float('nan')), v['where']))
    for a, b, c in clamped:
        print('clamped: %s n %d replayed with %d' % (a, b, c))
    if rel_var:
        print('one-pass variance, relative error at column offsets 0 / 3 / 30 sigma: %.2e / %.2e / %.2e' % tuple(rel_var))
    out_dir = os.environ.get('EGONET_AMD_PARITY_DIR')
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, 'train_ops_sweep.json'), 'w') as fh:
            json.dump(summary, fh, indent=1)
    assert not fails, '%d failures:\n%s' % (len(fails), '\n'.join(fails[:40]))
    # the sweep reached what it is meant to reach
    seen = {r['name'] for r in reqs}
    assert T.product_entries() <= seen, sorted(T.product_entries() - seen)
    assert any(r['s'].get('ld', 0) > r['s'].get('cols', 0) for r in reqs)
    assert any(r['alias'] for r in reqs)
    assert set(T.OPTIMIZERS) <= seen
    assert {r['s']['crit'] for r in reqs if r['name'] == 'egn_elem_loss_f32'} == {0, 1, 2}
    assert rel_var is not None
