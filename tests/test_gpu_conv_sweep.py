"""Every tile configuration the tuner can pick, on every convolution request the product makes, against float64.

``tuner.choose`` answers a shape outside the shipped table with whichever configuration the planner accepts and that
measured fastest; the training tape and the GEMM callers pick among table entries by the kinds they can feed.  So each
(request, candidate) pair of tests/conv_sweep.py runs here through the entry point the product would use -- a one-op
program for the inference engine; egn_conv2d_ex_f32 / egn_conv2d_bnstats_f32 / egn_conv2d_f32 as the tape calls them;
K-split configurations also in egn_conv2d_f32's three-launch form -- and every launch is checked for:
  1. |y - y64| <= C_BOUND[kind] * 2^-24 * A (y64: train_checks.conv_ref64, A: the same on absolute values);
  2. every element written (y pre-filled with NaN; NHWC pad channels exactly 0);
  3. no write outside y / the statistics partials / the ticket words (sentinel guard bands, bit-identical after);
  4. the same bits from a second launch (the statistics partials of a K split with ticket words excepted: their rows
     follow arrival order by design, so there both launches' totals are held to the bound of 6.);
  5. caller-owned ticket words zero again after the launch;
  6. fused BatchNorm partials that sum (in float64) to the channel sums / sums of squares of y64;
  7. the tape's in-place residual (res is y) for its data-gradient requests.
A summary per configuration (requests, worst |err| / (2^-24 A) and where) is printed, and written as JSON to
conv_sweep.json in the directory EGONET_AMD_PARITY_DIR names, if it is set.

The same launches and checks run on the hand-written edge list (conv_sweep.edge_requests, built for this device's CU
count), one case per kernel family; each case then requires that every config of its family was run in every edge class
the family admits, and adds an ``edge`` section to conv_sweep.json.  One step outside each predicate
(conv_sweep.refusal_requests) the forced config is refused and nothing is written.
"""
import ctypes as C
import json
import os
import time

import pytest
import torch

import conv_sweep as S
from egonet_amd import _lib, engine, tuner
from sweep_guards import _guarded, _guards_intact
from train_checks import conv_ref64

pytestmark = pytest.mark.gpu

class _Case(object):
    """Inputs and float64 reference of one request."""

    def __init__(self, req):
        n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, nchw = req['key']
        self.req = req
        self.ho, self.wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
        self.coutp = (cout + 15) // 16 * 16
        x, self.w, sc, sh, res = S.draw(req)                  # (seeded by the request; drawn on the CPU)
        self.x = x.cuda()
        self.sc, self.sh = sc.cuda(), sh.cuda()
        self.ny = n * self.ho * self.wo * (cout if nchw else cs_out)
        self.res = None if res is None else res.cuda()
        self.packs = {}
        # the reference, float64 on the GPU
        x64 = self.x.view(n, h, w, cs_in)[..., :cin].permute(0, 3, 1, 2).double()
        w64 = self.w.double().cuda()
        r64 = None if self.res is None else self._nchw(self.res).double()
        sc64, sh64 = self.sc.double(), self.sh.double()
        self.y64 = conv_ref64(x64, w64, stride, pad, sc64, sh64, r64, req['act'])
        self.A = S.bound_A(x64, w64, stride, pad, sc64, sh64, r64, req['act'])
        if req['stats']:
            self.sum64 = self.y64.sum((0, 2, 3))
            self.sq64 = (self.y64 ** 2).sum((0, 2, 3))
            self.sumA = self.A.sum((0, 2, 3))
            self.sqA = (2 * self.y64.abs() * self.A + S.U * self.A ** 2).sum((0, 2, 3))

    def _nchw(self, flat):
        n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, nchw = self.req['key']
        if nchw:
            return flat.view(n, cout, self.ho, self.wo)
        return flat.view(n, self.ho, self.wo, cs_out)[..., :cout].permute(0, 3, 1, 2)

    def packed(self, kind):
        if kind not in self.packs:
            self.packs[kind] = engine.pack_for_kind(self.w, kind).cuda()
        return self.packs[kind]


def _modes(req, cfg):
    """The launches of one (request, candidate) pair: (entry, with statistics, with ticket words)."""
    kind = tuner.kind_of(cfg)
    k_split = tuner.ticket_words(req['key'], cfg) > 0
    entry = req['entry']
    if entry == 'program':
        out = [('program', False, False)]
    elif entry == 'tape':               # train_hrnet._Tape._conv_launch
        rows = S.bnstats_rows(req['key'], cfg) if cfg > 0 else 0
        stats = req['stats'] and cfg > 0 and rows > 0
        if kind == 3:
            out = [('ex', stats, k_split)]
        else:
            out = [('bnstats' if stats else 'conv2d', stats, False)]
    else:
        out = [('conv2d', False, False)]
    if k_split and not req['alias'] and out[0] != ('conv2d', False, False):
        out.append(('conv2d', False, False))          # the three-launch form (egonet_hip.h: egn_conv_config_kind)
    return out


def _run_pair(case, cfg, mode, stats, tickets):
    """Both launches of one mode; returns (worst ratio, [failure strings])."""
    L = _lib.lib()
    req = case.req
    n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, nchw = req['key']
    key = req['key']
    wp = case.packed(tuner.kind_of(cfg))
    stream = _lib.current_stream()
    fails = []
    ywhole, y = _guarded(case.ny, torch.float32, None if req['alias'] else float('nan'))
    res = case.res
    if req['alias']:
        y.copy_(case.res)                 # the gradient x already holds; the conv adds to it in place
        res = y
    rows = S.bnstats_rows(key, cfg) if stats else 0
    pwhole = part = None
    if stats:
        pwhole, part = _guarded(rows * 2 * cout, torch.float64, float('nan'))
    ntk = tuner.ticket_words(key, cfg) if tickets else 0
    twhole = tk = None
    if tickets:
        twhole, tk = _guarded(ntk, torch.int32, 0)
    prog = None
    if mode == 'program':
        prog = C.c_void_p(L.egn_program_create(8))
        refs = []
        for slot, t in enumerate((case.x, wp, case.sc, case.sh, res, y)):
            if t is None:
                refs.append(_lib.NULL_REF)
                continue
            _lib.check(L.egn_program_bind(prog, slot, _lib.ptr(t)))
            refs.append(_lib.Ref(slot, 0))
        _lib.check(L.egn_program_add_conv2d(prog, *refs, n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad,
                                            req['act'], int(nchw), cfg), 'add_conv2d')

    def launch():
        if mode == 'program':
            return L.egn_program_run(prog, stream)
        if mode == 'ex':
            return L.egn_conv2d_ex_f32(_lib.ptr(case.x), _lib.ptr(wp), _lib.ptr(case.sc), _lib.ptr(case.sh),
                                       _lib.ptr(res), _lib.ptr(y), n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride,
                                       pad, req['act'], cfg, _lib.ptr(part), rows, _lib.ptr(tk), ntk, stream)
        if mode == 'bnstats':
            return L.egn_conv2d_bnstats_f32(_lib.ptr(case.x), _lib.ptr(wp), _lib.ptr(case.sc), _lib.ptr(case.sh),
                                            _lib.ptr(y), n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, cfg,
                                            _lib.ptr(part), rows, stream)
        return L.egn_conv2d_f32(_lib.ptr(case.x), _lib.ptr(wp), _lib.ptr(case.sc), _lib.ptr(case.sh), _lib.ptr(res),
                                _lib.ptr(y), n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, req['act'],
                                int(nchw), cfg, stream)

    worst = 0.0
    try:
        first = None
        for rep in range(2):
            if rep and req['alias']:
                y.copy_(case.res)
            elif rep:
                y.fill_(float('nan'))
                if stats:
                    part.fill_(float('nan'))
            rc = launch()
            torch.cuda.synchronize()
            if rc != 0:
                fails.append('launch %d returned %d (%s)' % (rep, rc, L.egn_strerror(rc).decode()))
                break
            if not _guards_intact(ywhole):
                fails.append('write outside y')
            if stats and not _guards_intact(pwhole):
                fails.append('write outside the statistics partials')
            if tickets:
                if not _guards_intact(twhole):
                    fails.append('write outside the ticket words')
                if bool((tk != 0).any()):
                    fails.append('ticket words not zero after the launch')
            if rep == 0:
                got = case._nchw(y)
                if not bool(torch.isfinite(got).all()):
                    fails.append('%d elements not written / not finite' % int((~torch.isfinite(got)).sum()))
                if not nchw and cs_out > cout and bool((y.view(-1, cs_out)[:, cout:] != 0).any()):
                    fails.append('pad channels not 0')
                r = S.ratio(got, case.y64, case.A)
                worst = float(r.max())
                if not worst <= S.C_BOUND[tuner.kind_of(cfg)]:
                    fails.append('error %.1f x 2^-24 A > %g' % (worst, S.C_BOUND[tuner.kind_of(cfg)]))
                if stats:
                    tot = part.view(rows, 2, cout).sum(0)
                    c = S.C_BOUND[tuner.kind_of(cfg)] * S.U
                    if not bool(((tot[0] - case.sum64).abs() <= c * case.sumA).all()) or \
                            not bool(((tot[1] - case.sq64).abs() <= c * case.sqA).all()):
                        fails.append('fused BatchNorm statistics off')
                first = (y.clone(), part.clone() if stats else None)
            else:
                if not torch.equal(y.view(torch.int32), first[0].view(torch.int32)):
                    fails.append('second launch: different bits')
                if stats and tickets:
                    # the K split with ticket words: the half that finishes second stores an output pair and owns its
                    # statistics, so WHICH block's row holds them follows arrival order (csrc/conv_wino4.hip, ST):
                    # the rows may differ in bits, their float64 totals must still meet the bound
                    tot = part.view(rows, 2, cout).sum(0)
                    c = S.C_BOUND[tuner.kind_of(cfg)] * S.U
                    if not bool(((tot[0] - case.sum64).abs() <= c * case.sumA).all()) or \
                            not bool(((tot[1] - case.sq64).abs() <= c * case.sqA).all()):
                        fails.append('second launch: fused BatchNorm statistics off')
                elif stats and not torch.equal(part.view(torch.int64), first[1].view(torch.int64)):
                    fails.append('second launch: different statistics bits')
    finally:
        if prog is not None:
            torch.cuda.synchronize()
            L.egn_program_destroy(prog)
    return worst, fails


@pytest.fixture(scope='module')
def sweep_pairs():
    t0 = time.time()
    reqs = S.inference_requests() + S.tape_requests('cuda')
    return reqs, S.pairs(reqs), time.time() - t0


def test_every_candidate_config_matches_float64(sweep_pairs):
    reqs, prs, t_collect = sweep_pairs
    t0 = time.time()
    groups = {}
    for p in prs:
        groups.setdefault((p['key'], p['act'], p['entry'], p['alias'], p['stats']), []).append(p)
    per_cfg, per_entry, fails = {}, {}, []
    kinds_worst = {}
    n_launch = 0
    for gk, ps in groups.items():
        case = _Case(ps[0])
        for p in ps:
            cfg = p['cfg']
            ent = per_cfg.setdefault(cfg, dict(requests=0, launches=0, worst=0.0, where=''))
            ent['requests'] += 1
            for mode, stats, tickets in _modes(p, cfg):
                worst, f = _run_pair(case, cfg, mode, stats, tickets)
                n_launch += 1
                k_split = tuner.ticket_words(p['key'], cfg) > 0
                name = mode + ('+stats' if stats else '') + ('+tickets' if tickets else '') + \
                    ('(3 launches)' if k_split and mode == 'conv2d' else '')
                per_entry[name] = per_entry.get(name, 0) + 1
                ent['launches'] += 1
                if worst >= ent['worst']:
                    ent['worst'], ent['where'] = worst, '%s %s act %d %s' % (name, p['srcs'][0], p['act'],
                                                                             'alias' if p['alias'] else '')
                k = tuner.kind_of(cfg)
                kinds_worst[k] = max(kinds_worst.get(k, 0.0), worst)
                for msg in f:
                    fails.append('cfg %d %s key %s act %d alias %d (%s): %s'
                                 % (cfg, name, p['key'], p['act'], p['alias'], p['srcs'][0], msg))
        del case
        torch.cuda.empty_cache()
    wall = time.time() - t0
    L = _lib.lib()
    summary = dict(requests=len(reqs), distinct_requests=len(groups), pairs=len(prs), launches_checked=n_launch,
                   collect_s=round(t_collect, 1), sweep_s=round(wall, 1), entries=per_entry,
                   worst_ratio_per_kind={S.KIND_NAMES.get(k, str(k)): round(v, 2) for k, v in kinds_worst.items()},
                   bound_per_kind={S.KIND_NAMES[k]: v for k, v in S.C_BOUND.items()},
                   configs={str(c): dict(v, worst=round(v['worst'], 2)) for c, v in sorted(per_cfg.items())},
                   failures=fails[:200])
    print('\nconv sweep: %d requests (%d distinct), %d pairs, %d checked launches, %.0f s + %.0f s collection'
          % (len(reqs), len(groups), len(prs), n_launch, wall, t_collect))
    print('entries: %s' % per_entry)
    for c, v in sorted(per_cfg.items()):
        buf = C.create_string_buffer(96)
        if c > 0:
            L.egn_conv_config_name(c, buf, 96)
        print('cfg %2d %-44s %5d requests %5d launches  worst %7.2f  %s'
              % (c, buf.value.decode() or 'cost model', v['requests'], v['launches'], v['worst'], v['where']))
    print('worst |err| / (2^-24 A) per kind: %s (bounds %s)' % (summary['worst_ratio_per_kind'],
                                                                summary['bound_per_kind']))
    out_dir = os.environ.get('EGONET_AMD_PARITY_DIR')
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, 'conv_sweep.json'), 'w') as fh:
            json.dump(summary, fh, indent=1)
    assert not fails, '%d failing launches:\n%s' % (len(fails), '\n'.join(fails[:40]))
    # the sweep reached what it is meant to reach
    product = [0] + list(range(1, 31)) + [42, 44, 51, 52, 56, 57, 59, 60, 61, 62, 64, 70, 79, 80, 82, 83, 84, 85, 86]
    assert all(per_cfg.get(c, {}).get('requests', 0) > 0 for c in product), \
        sorted(c for c in product if c not in per_cfg)
    assert {'program', 'ex', 'bnstats', 'conv2d'} <= {k.split('+')[0].split('(')[0] for k in per_entry}, per_entry
    assert any(k.startswith('ex') and 'tickets' in k for k in per_entry), per_entry
    assert any(p['alias'] for p in prs)


# ---------------------------------------------------------------------------------------------------------------
# the edge list (conv_sweep.edge_requests): every config at the edges of its tile mapping
# ---------------------------------------------------------------------------------------------------------------
def _device_cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture(scope='module')
def edge_pairs():
    cus = _device_cus()
    reqs = S.edge_requests(cus)
    return cus, reqs, S.pairs(reqs)


def _mode_name(p, cfg, mode, stats, tickets):
    k_split = tuner.ticket_words(p['key'], cfg) > 0
    return mode + ('+stats' if stats else '') + ('+tickets' if tickets else '') + \
        ('(3 launches)' if k_split and mode == 'conv2d' else '')


@pytest.mark.parametrize('family', S.FAMILIES)
def test_every_candidate_config_at_its_edges_matches_float64(edge_pairs, family):
    """The pairs of the edge list whose config is of ``family``, through the same _Case / _run_pair as the recorded
    corpus (the seven checks of this file's docstring); then: with this device's CU count, every config of the family
    was run in every edge class its predicate admits."""
    cus, reqs, prs = edge_pairs
    t0 = time.time()
    mine = [p for p in prs if S.family_of(p['cfg']) == family]
    groups = {}
    for p in mine:
        groups.setdefault((p['key'], p['act'], p['entry'], p['alias'], p['stats']), []).append(p)
    per_cfg, per_entry, fails, kinds_worst, reached = {}, {}, [], {}, {}
    n_launch = 0
    for gk, ps in groups.items():
        case = _Case(ps[0])
        for p in ps:
            cfg = p['cfg']
            ent = per_cfg.setdefault(cfg, dict(requests=0, launches=0, worst=0.0, where=''))
            ent['requests'] += 1
            reached.setdefault(cfg, set()).update(S.edge_classes(p, cfg, cus))
            for mode, stats, tickets in _modes(p, cfg):
                worst, f = _run_pair(case, cfg, mode, stats, tickets)
                n_launch += 1
                name = _mode_name(p, cfg, mode, stats, tickets)
                per_entry[name] = per_entry.get(name, 0) + 1
                ent['launches'] += 1
                if worst >= ent['worst']:
                    ent['worst'], ent['where'] = worst, '%s %s act %d %s' % (name, p['srcs'][0], p['act'],
                                                                             'alias' if p['alias'] else '')
                k = tuner.kind_of(cfg)
                if worst >= kinds_worst.get(k, (0.0, ''))[0]:
                    kinds_worst[k] = (worst, 'cfg %d %s key %s' % (cfg, p['srcs'][0], p['key']))
                for msg in f:
                    fails.append('cfg %d %s key %s act %d alias %d (%s): %s'
                                 % (cfg, name, p['key'], p['act'], p['alias'], p['srcs'][0], msg))
        del case
    torch.cuda.empty_cache()
    wall = time.time() - t0
    L = _lib.lib()
    print('\nconv edge sweep, %s: %d CUs, %d pairs of %d requests, %d checked launches, %.1f s'
          % (family, cus, len(mine), len(groups), n_launch, wall))
    print('entries: %s' % per_entry)
    for c, v in sorted(per_cfg.items()):
        buf = C.create_string_buffer(96)
        if c > 0:
            L.egn_conv_config_name(c, buf, 96)
        print('cfg %2d %-44s %5d requests %5d launches  worst %7.2f  %s'
              % (c, buf.value.decode() or 'cost model', v['requests'], v['launches'], v['worst'], v['where']))
    for k, (v, where) in sorted(kinds_worst.items()):
        print('worst |err| / (2^-24 A), %s: %.2f (bound %g) at %s' % (S.KIND_NAMES[k], v, S.C_BOUND[k], where))
    summary = dict(cus=cus, pairs=len(mine), launches_checked=n_launch, sweep_s=round(wall, 1), entries=per_entry,
                   worst_ratio_per_kind={S.KIND_NAMES[k]: dict(ratio=round(v, 2), where=where)
                                         for k, (v, where) in kinds_worst.items()},
                   configs={str(c): dict(v, worst=round(v['worst'], 2), classes=sorted(reached.get(c, ())))
                            for c, v in sorted(per_cfg.items())},
                   failures=fails[:200])
    out_dir = os.environ.get('EGONET_AMD_PARITY_DIR')
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        path, doc = os.path.join(out_dir, 'conv_sweep.json'), {}
        if os.path.isfile(path):
            with open(path) as fh:
                doc = json.load(fh)
        doc.setdefault('edge', {})[family] = summary
        with open(path, 'w') as fh:
            json.dump(doc, fh, indent=1)
    assert not fails, '%d failing launches:\n%s' % (len(fails), '\n'.join(fails[:40]))
    # every selectable config of the family, in every class the family admits
    cfgs = [c for c in S.selectable_configs() if S.family_of(c) == family]
    assert cfgs
    missing = [(c, k) for c in cfgs for k in sorted(S.FAMILY_CLASSES[family])
               if k not in reached.get(c, ()) and (c, k) not in S.NOT_REACHABLE and (family, k) not in S.NOT_REACHABLE]
    assert not missing, missing


def test_one_step_outside_each_predicate_is_refused_and_writes_nothing():
    """conv_sweep.refusal_requests: egn_conv2d_f32 with the config forced returns non-zero before anything launches;
    the output keeps its sentinel."""
    L = _lib.lib()
    stream = _lib.current_stream()
    fails = []
    for cfg, key, act, clause, at in S.refusal_requests():
        n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, nchw = key
        ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
        ny = n * ho * wo * (cout if nchw else cs_out)
        coutp = (cout + 15) // 16 * 16
        x = torch.ones(n * h * w * cs_in, device='cuda')
        wp = torch.ones(max((cin + 15) // 16 * kh * kw * 4 * coutp * 4, cout * cin * 48), device='cuda')
        sc, sh = torch.ones(coutp + 16, device='cuda'), torch.zeros(coutp + 16, device='cuda')
        res = torch.ones(ny, device='cuda') if has_res else None
        ywhole, y = _guarded(ny, torch.float32, -7777.0)
        rc = L.egn_conv2d_f32(_lib.ptr(x), _lib.ptr(wp), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(res), _lib.ptr(y), n, h, w,
                              cin, cs_in, cout, cs_out, kh, kw, stride, pad, act, int(nchw), cfg, stream)
        torch.cuda.synchronize()
        if rc == 0:
            fails.append('cfg %d took %s (%s)' % (cfg, key, clause[1]))
        if not bool((y == -7777.0).all()) or not _guards_intact(ywhole):
            fails.append('cfg %d wrote on refusing %s' % (cfg, key))
    assert not fails, '\n'.join(fails)
