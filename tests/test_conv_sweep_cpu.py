"""Host side of the conv configuration sweep (tests/test_gpu_conv_sweep.py), no GPU: the error bound it applies
separates honest fp32 arithmetic from the slips a kernel makes, and the request corpus is what it claims to be."""
import ctypes as C
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_sweep as S
from egonet_amd import _lib, engine, tuner
from tools import wino43_error_study as W
from train_checks import conv_ref64

MATS = {1: W.mats([0.0, 1.0, -1.0]), 3: W.mats([0.0, 1.0, -1.0, 2.0, -2.0])}


def _case(seed, n=2, cin=32, cout=48, hw=16, kh=3, stride=1):
    g = torch.Generator().manual_seed(seed)
    x = S.act_like(n, hw, hw, cin, cin, g).permute(0, 3, 1, 2).contiguous()          # NCHW fp32
    w = S.filt(cout, cin, kh, kh, g)
    sc = torch.where(torch.rand(cout, generator=g) < 0.3, -1.0, 1.0) * (0.5 + torch.rand(cout, generator=g))
    sh = 0.5 * torch.randn(cout, generator=g)
    ho = (hw + 2 * (kh // 2) - kh) // stride + 1
    res = S.act_like(n, ho, ho, cout, cout, g).permute(0, 3, 1, 2).contiguous()
    return x, w, sc, sh, res


def _fp32(kind, x, w, stride, pad):
    """Honest fp32 convolution of a kernel kind: torch's fp32 conv2d (direct) or the Winograd emulation of
    tools/wino43_error_study.py (fp32 transforms, products and sums; filter transform in float64, rounded once)."""
    if kind == 0:
        return F.conv2d(x, w, None, stride, pad).double()
    AT, G, BT = MATS[kind]
    out = [torch.from_numpy(W.conv_wino(np.pad(xi.numpy(), ((0, 0), (1, 1), (1, 1))), w.double().numpy(), AT, G, BT)
                            .astype(np.float64)) for xi in x]
    return torch.stack(out)


def _epilogue32(z, sc, sh, res, act):
    y = z.float() * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) + res
    return torch.relu(y) if act == engine.ACT_RELU else y


def _worst(kind, y, x, w, stride, pad, sc, sh, res, act):
    x64, w64 = x.double(), w.double()
    want = conv_ref64(x64, w64, stride, pad, sc.double(), sh.double(), res.double(), act)
    A = S.bound_A(x64, w64, stride, pad, sc.double(), sh.double(), res.double(), act)
    return float(S.ratio(y, want, A).max()) / S.C_BOUND[kind]


def _tf32(t):
    b = t.float().contiguous().view(torch.int32)
    return ((b + 0x1000) & ~0x1FFF).view(torch.float32)


MUTATIONS = ['tf32', 'drop_last_chunk', 'row_shift', 'taps_transposed']
SHAPES = {0: [(3, 1), (3, 2), (1, 1)], 1: [(3, 1)], 3: [(3, 1)]}       # (kh, stride) per kind


@pytest.mark.parametrize('kind', [0, 1, 3])
def test_bound_passes_honest_fp32_and_rejects_slips(kind):
    """Honest fp32 sits inside C_BOUND[kind] * 2^-24 * A on every element; each deliberate slip lands outside."""
    for kh, stride in SHAPES[kind]:
        for seed in range(2):
            x, w, sc, sh, res = _case(seed + 10 * kind, kh=kh, stride=stride)
            pad = kh // 2
            act = engine.ACT_RELU

            def run(xx, ww):
                return _epilogue32(_fp32(kind, xx, ww, stride, pad), sc, sh, res, act)
            honest = _worst(kind, run(x, w), x, w, stride, pad, sc, sh, res, act)
            assert honest <= 1.0, (kind, kh, stride, honest)
            for mut in MUTATIONS:
                if mut == 'taps_transposed' and kh == 1:
                    continue                        # (one tap: nothing to transpose)
                if mut == 'tf32':
                    y = run(_tf32(x), _tf32(w))
                elif mut == 'drop_last_chunk':
                    xm = x.clone()
                    xm[:, -16:] = 0
                    y = run(xm, w)
                elif mut == 'row_shift':
                    y = run(x, w).clone()
                    r = y.shape[2] // 2
                    y[:, :, r] = torch.roll(y[:, :, r], 1, dims=-1)
                else:
                    y = run(x, w.transpose(2, 3).contiguous())
                got = _worst(kind, y, x, w, stride, pad, sc, sh, res, act)
                assert got > 1.0, (kind, kh, stride, mut, got, honest)


def test_corpus_is_real_and_without_duplicates():
    reqs = S.inference_requests()
    prs = S.pairs(reqs)
    keys = {(p['key'], p['act'], p['entry'], p['alias'], p['stats'], p['cfg']) for p in prs}
    assert len(keys) == len(prs)
    distinct = {(p['key'], p['act']) for p in prs}
    assert len(distinct) >= 300, len(distinct)
    cfgs = {p['cfg'] for p in prs}
    # the inference programs reach the direct, F(2x2,3x3) and F(4x4,3x3) families, the K split, the stem, the 1x1 row
    # GEMM and the stride-2 kernel
    assert {0, 1, 30, 51, 59, 64, 70, 79, 80, 83, 84, 85, 86} <= cfgs, sorted(cfgs)
    assert any(r['key'][12] for r in reqs)                                        # NCHW head outputs
    assert any(r['act'] & engine.ACT_RES_AFTER for r in reqs)                     # the lifter's residual
    assert any((r['key'][7], r['key'][8]) in ((4, 4), (4, 3)) for r in reqs)     # the valid head convolutions
    assert {70, 20} <= {r['key'][0] for r in reqs}
    for p in prs:                     # a candidate's filter is one the caller can feed, and the planner takes the key
        assert tuner.kind_of(p['cfg']) in p['kinds'] and tuner.usable(p['key'], p['cfg'], p['kinds']), p


_KEY = re.compile(r'n(\d+)_h(\d+)_w(\d+)_ci(\d+)\.(\d+)_co(\d+)\.(\d+)_k(\d+)x(\d+)_s(\d+)_p(\d+)_r(\d+)_o(\d+)$')


def _table():
    """(shape_key arguments, entry) of every shape of the shipped table."""
    tab = tuner._load()
    assert tab
    for key, ent in tab.items():
        m = _KEY.match(key)
        assert m, key
        v = [int(t) for t in m.groups()]
        args = tuple(v[:11]) + (bool(v[11]), bool(v[12]))
        assert tuner.shape_key(*args) == key
        yield args, ent


def test_every_tabled_config_is_a_candidate():
    """Whatever the shipped table can hand out for a shape is a candidate the sweep runs for it (tuner.tune times
    exactly tuner.candidates; tuner._pick falls back to any of them)."""
    for args, ent in _table():
        cand = set(tuner.candidates(args, tuner.ALL_KINDS))
        # (ids retired since the table was measured have kind -1: tuner._pick never returns them)
        ids = {c for c in {int(k) for k in ent.get('ms', {})} | {int(ent['cfg'])} if tuner.kind_of(c) >= 0}
        assert ids and ids <= cand, (args, sorted(ids - cand))


def test_tape_candidates_follow_the_tape_rules():
    """What train_hrnet._Tape._conv_launch tells the tuner: no kind 2, no K split for the in-place residual."""
    key = (8, 16, 16, 192, 192, 192, 192, 3, 3, 1, 1, True, False)
    free = tuner.candidates(key, tuner.TAPE_F43, 1 << 16)
    alias = tuner.candidates(key, tuner.TAPE_F43, 1 << 16, inplace_res=True)
    assert 84 in free and 84 not in alias and set(alias) < set(free)
    assert 84 not in tuner.candidates(key, tuner.TAPE_F43, tuner.ticket_words(key, 84) - 1)     # too few ticket words
    assert all(_lib.lib().egn_conv_config_kind(c) != 2 for c in free if c)
    assert set(tuner.candidates(key, tuner.DIRECT, 1 << 16)) == {c for c in free if tuner.kind_of(c) == 0}


PROFILES = {                                    # what each caller passes to tuner.choose
    'program, plain epilogue': dict(kinds=tuner.ALL_KINDS),
    'program, other epilogue': dict(kinds=tuner.DIRECT),
    'tape forward': dict(kinds=tuner.TAPE_F43, ticket_cap=1 << 16),
    'tape aliased data gradient': dict(kinds=tuner.TAPE_F43, ticket_cap=1 << 16, inplace_res=True),
    'direct only': dict(kinds=tuner.DIRECT),
}


def test_choose_answers_with_a_candidate(monkeypatch):
    """With autotuning off, what ``choose`` hands each kind of caller for each tabled shape is one of ``candidates``
    for that caller -- the set the sweep runs."""
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    for name in ('EGONET_AMD_WINO', 'EGONET_AMD_F43', 'EGONET_AMD_F43_MATCH', 'EGONET_AMD_SKIP_CFG'):
        monkeypatch.delenv(name, raising=False)
    picked = set()
    for args, _ in _table():
        for who, prof in PROFILES.items():
            cfg = tuner.choose('cpu', args, **prof)
            assert cfg in tuner.candidates(args, **prof), (who, args, cfg)
            picked.add((who, tuner.kind_of(cfg)))
    assert ('tape forward', 3) in picked and ('program, plain epilogue', 3) in picked       # (not vacuous)


# ---------------------------------------------------------------------------------------------------------------
# the edge list (conv_sweep.edge_requests)
# ---------------------------------------------------------------------------------------------------------------
CUS = S.NOMINAL_CUS


@pytest.fixture(scope='module')
def edges():
    reqs = S.edge_requests(CUS)
    return reqs, S.pairs(reqs)


@pytest.fixture(scope='module')
def recorded():
    reqs = S.inference_requests()
    return reqs, S.pairs(reqs)


def _pair_id(p):
    return (p['key'], p['act'], p['entry'], p['alias'], p['stats'], p['cfg'])


def _reached(prs):
    """{cfg: the edge classes its pairs are in}, with the nominal CU count."""
    out = {}
    for p in prs:
        if p['cfg'] > 0:
            out.setdefault(p['cfg'], set()).update(S.edge_classes(p, p['cfg'], CUS))
    return out


def test_every_edge_request_plans_and_names_a_line_of_its_kernel(edges):
    reqs, prs = edges
    texts = {}
    L = _lib.lib()
    for r in reqs:
        name, line = r['line']
        texts.setdefault(name, S.kernel_text(name))
        assert line in texts[name], (r['src'], name, line)
        assert r['why'] and r['family']
        assert L.egn_conv_plan_query(*r['key'][:11], int(r['key'][12]), 0, (C.c_int * 12)()) == 0, r['src']
        assert r['entry'] in ('program', 'tape', 'conv2d')
        if r['entry'] == 'program':
            assert r['kinds'] == engine.Program._conv_kinds(dict(act=r['act'])) and r['ticket_cap'] is None
        elif r['entry'] == 'tape':
            assert r['ticket_cap'] == S.TAPE_TICKETS and r['kinds'] in (tuner.TAPE_WINO, tuner.TAPE_F43, tuner.DIRECT)
            assert (r['kinds'] == tuner.DIRECT) == (r['act'] not in (engine.ACT_NONE, engine.ACT_RELU))
            assert not r['stats'] or (r['act'] == engine.ACT_NONE and not r['key'][11])
        else:
            assert r['kinds'] == tuner.DIRECT
        assert r['alias'] == r['inplace_res'] and (not r['alias'] or (r['entry'] == 'tape' and r['key'][11]))
    for (who, k), (name, clause) in S.NOT_REACHABLE.items():
        texts.setdefault(name, S.kernel_text(name))
        assert clause in texts[name], (who, k, name, clause)
        assert who in S.FAMILIES or who in S.selectable_configs(), who
    entries = {(r['family'], r['entry']) for r in reqs}
    assert {('Staged/Dma', 'program'), ('Staged/Dma', 'tape'), ('Staged/Dma', 'conv2d'), ('F(2x2)', 'tape'),
            ('F(4x4)', 'tape'), ('F(4x4)', 'program')} <= entries
    assert any(r['kinds'] == tuner.TAPE_WINO for r in reqs) and any(r['kinds'] == tuner.TAPE_F43 for r in reqs)


def test_every_config_is_run_in_every_class_its_family_admits(edges):
    """The coverage guard: a config row without edge requests, or a class nobody reaches, fails here."""
    reqs, prs = edges
    reached = _reached(prs)
    cfgs = S.selectable_configs()                          # derived from the loaded library
    assert {S.family_of(c) for c in cfgs} == set(S.FAMILIES) == set(S.FAMILY_CLASSES)
    missing, contradicted = [], []
    for c in cfgs:
        fam = S.family_of(c)
        for k in sorted(S.FAMILY_CLASSES[fam]):
            excused = (c, k) in S.NOT_REACHABLE or (fam, k) in S.NOT_REACHABLE
            if k in reached.get(c, ()) and excused:
                contradicted.append((c, k))
            elif k not in reached.get(c, ()) and not excused:
                missing.append((c, k))
        # nothing is reached that the family's row does not admit (the table would be wrong)
        assert reached.get(c, set()) <= S.FAMILY_CLASSES[fam], (c, sorted(reached[c] - S.FAMILY_CLASSES[fam]))
    assert not missing, 'unreached and unexplained: %s' % missing
    assert not contradicted, 'NOT_REACHABLE, yet reached: %s' % contradicted
    for fam in S.FAMILIES:                                 # the residual-free / plain-epilogue families admit no more
        if fam not in ('Staged', 'Dma'):
            assert (fam, 'ragged_k') in S.NOT_REACHABLE or 'ragged_k' in S.FAMILY_CLASSES[fam]


def test_the_edge_list_reaches_what_the_recorded_corpus_does_not(edges, recorded):
    """Per family, the classes reached by the recorded inference corpus against those of the edge list (printed); at
    least one class per family only the edge list reaches; and no (request, config) pair is in both."""
    e_reqs, e_prs = edges
    r_reqs, r_prs = recorded
    both = S.pairs(r_reqs + e_reqs)
    assert len(both) == len(r_prs) + len(e_prs), 'an edge request repeats a recorded one'
    assert len({_pair_id(p) for p in both}) == len(both)
    assert sum(len(p['srcs']) for p in e_prs) == len(e_prs), 'the edge list repeats itself'
    r_reached, e_reached = _reached(r_prs), _reached(e_prs)
    print('\nfamily   class                recorded configs / edge configs (of the family\'s selectable ones)')
    for fam in S.FAMILIES:
        cfgs = [c for c in S.selectable_configs() if S.family_of(c) == fam]
        only_edge = []
        for k in sorted(S.FAMILY_CLASSES[fam]):
            nr = sum(k in r_reached.get(c, ()) for c in cfgs)
            ne = sum(k in e_reached.get(c, ()) for c in cfgs)
            print('%-8s %-20s %3d / %3d of %d%s' % (fam, k, nr, ne, len(cfgs), '   <- edge list only' if ne and not nr else ''))
            if ne and not nr:
                only_edge.append(k)
        assert only_edge, 'the recorded corpus already reaches every class of %s' % fam


def _emulated(req, kind, x, w, sc, sh, res, images=None):
    """Honest fp32 of one request for a kernel kind: (y NCHW fp32, want float64, A); ``images``: the first few only
    (the Winograd emulation walks the tiles in Python)."""
    n, h, wd, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, nchw = req['key']
    ho, wo = (h + 2 * pad - kh) // stride + 1, (wd + 2 * pad - kw) // stride + 1
    m = n if images is None else min(n, images)
    xn = x[:m, :, :, :cin].permute(0, 3, 1, 2).contiguous()
    rn = None
    if res is not None:
        rn = (res.view(n, cout, ho, wo) if nchw else res.view(n, ho, wo, cs_out)[..., :cout].permute(0, 3, 1, 2))[:m]
    z = _fp32(kind, xn, w, stride, pad)
    return _finish32(z, sc[:cout], sh[:cout], rn, req['act']), _reference(xn, w, stride, pad, sc, sh, rn, req['act'])


def _finish32(z, sc, sh, rn, act):
    y = z.float() * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    after = bool(act & engine.ACT_RES_AFTER)
    if rn is not None and not after:
        y = y + rn
    a = act & 0xf
    y = torch.relu(y) if a == engine.ACT_RELU else torch.sigmoid(y) if a == engine.ACT_SIGMOID else \
        torch.where(y > 0, y, 0.01 * y) if a == engine.ACT_LEAKY else y
    return y + rn if rn is not None and after else y


def _reference(xn, w, stride, pad, sc, sh, rn, act):
    x64, w64, r64 = xn.double(), w.double(), None if rn is None else rn.double()
    return (conv_ref64(x64, w64, stride, pad, sc.double(), sh.double(), r64, act),
            S.bound_A(x64, w64, stride, pad, sc.double(), sh.double(), r64, act))


def _kinds_of(req):
    return sorted({tuner.kind_of(c) for c in tuner.candidates(req['key'], req['kinds'], req['ticket_cap'], req['inplace_res'])})


EMU_IMAGES = 4          # images of a request the Winograd emulations run (the direct one runs them all)


def test_the_bound_holds_for_honest_fp32_on_every_edge_input(edges):
    """C_BOUND was calibrated on 3x3 layers with Cin 16 .. 192; the edge list leaves that range (Cin 1, 49 taps, 2 x 2
    maps, sigmoid).  The honest-fp32 emulation of each kind a request can be answered with, on the request's own
    inputs (conv_sweep.draw, as the GPU test draws them), must lie inside the unchanged bound."""
    reqs, prs = edges
    worst, near = {}, []
    seen = set()
    for r in reqs:
        rid = (r['key'], r['act'], r['entry'], r['stats'])
        if rid in seen:
            continue
        seen.add(rid)
        x, w, sc, sh, res = S.draw(r)
        for kind in _kinds_of(r):
            y, (want, A) = _emulated(r, kind, x, w, sc, sh, res, None if kind == 0 else EMU_IMAGES)
            v = float(S.ratio(y, want, A).max())
            assert v <= S.C_BOUND[kind], (S.KIND_NAMES[kind], r['src'], r['key'], v)
            if v >= worst.get(kind, (0.0, None))[0]:
                worst[kind] = (v, r)
            if v > S.C_BOUND[kind] / 3:
                near.append((S.KIND_NAMES[kind], round(v, 1), r['src'], r['key']))
    print()
    for kind, (v, r) in sorted(worst.items()):
        print('%-11s worst emulation ratio %7.2f of %g   %s %s act %d' % (S.KIND_NAMES[kind], v, S.C_BOUND[kind], r['src'],
                                                                         r['key'], r['act']))
    for t in near:
        print('above a third of its constant: %s %s %s %s' % t)
    assert set(worst) == {0, 1, 3}


def _edge_req(reqs, family, why):
    (r,) = [q for q in reqs if q['family'] == family and q['why'] == why]
    return r


EDGE_MUTATIONS = ['drop_partial_chunk', 'last_column_from_neighbour', 'clamped_padding', 'image_past_ragged_group',
                  'stats_over_whole_tile']


@pytest.mark.parametrize('mut', EDGE_MUTATIONS)
def test_slips_only_an_edge_shape_shows_are_caught(edges, mut):
    """Each slip, applied to the honest emulation of an edge request, lands outside the bound (or in a guard band); the
    honest emulation of the same request passes."""
    from sweep_guards import GUARD, SENT32, _guards_intact
    reqs, _ = edges
    if mut in ('drop_partial_chunk', 'last_column_from_neighbour'):
        r = _edge_req(reqs, 'Staged/Dma', 'ragged in x, y, n, K and Cout')
    elif mut == 'clamped_padding':
        r = _edge_req(reqs, 'Staged/Dma', 'map one pixel wide')
    elif mut == 'image_past_ragged_group':
        r = _edge_req(reqs, 'F(2x2)', 'ragged image group, map smaller than 8 x 8')
    else:
        r = _edge_req(reqs, 'F(2x2)', '16 x 16 and 8 x 16 tiles, partial both ways, statistics')
    n, h, wd, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, nchw = r['key']
    x, w, sc, sh, res = S.draw(r)
    y, (want, A) = _emulated(r, 0, x, w, sc, sh, res)
    C0 = S.C_BOUND[0]
    assert float(S.ratio(y, want, A).max()) <= C0
    rn = None if res is None else res.view(n, h, wd, cs_out)[..., :cout].permute(0, 3, 1, 2)
    xn = x[..., :cin].permute(0, 3, 1, 2).contiguous()
    if mut == 'drop_partial_chunk':
        assert cin % 16
        xm = xn.clone()
        xm[:, cin // 16 * 16:] = 0
        bad = _finish32(_fp32(0, xm, w, stride, pad), sc[:cout], sh[:cout], rn, r['act'])
    elif mut == 'last_column_from_neighbour':
        assert wd % 8 and wd % 16
        bad = y.clone()
        bad[..., -1] = bad[..., -2]
    elif mut == 'clamped_padding':
        assert wd == 1
        bad = _finish32(F.conv2d(F.pad(xn, (pad,) * 4, mode='replicate'), w).double(), sc[:cout], sh[:cout], rn, r['act'])
    elif mut == 'image_past_ragged_group':
        assert n % 4 and n % 2                     # ragged on the four-image and on the two-image kernels
        per = h * wd * cs_out
        whole = torch.full((n * per + 2 * GUARD,), SENT32, dtype=torch.int32)
        assert _guards_intact(whole)
        body = whole[GUARD:GUARD + (n + 1) * per].view(torch.float32)       # the group's next image slot is written too
        body[:n * per] = y.permute(0, 2, 3, 1).reshape(-1)
        body[n * per:] = 0.0
        assert not _guards_intact(whole)
        return
    else:
        # statistics of a ragged pair: the sum over the in-map outputs meets check 6's bound, the sum over whole tiles
        # (outputs past the map's edge still see its last row / column through the filter) does not
        assert r['stats'] and h % 16 and wd % 16
        sum64, sumA = want.sum((0, 2, 3)), A.sum((0, 2, 3))
        sq64, sqA = (want ** 2).sum((0, 2, 3)), (2 * want.abs() * A + S.U * A ** 2).sum((0, 2, 3))
        c = S.C_BOUND[1] * S.U
        yd = y.double()
        assert bool(((yd.sum((0, 2, 3)) - sum64).abs() <= c * sumA).all())
        assert bool((((yd ** 2).sum((0, 2, 3)) - sq64).abs() <= c * sqA).all())
        th = (h + 15) // 16 * 16
        tw = (wd + 15) // 16 * 16
        tile = F.conv2d(F.pad(xn, (1, 1 + tw - wd, 1, 1 + th - h)), w).double()       # every output of the 16 x 16 tiles
        assert tile.shape[-2:] == (th, tw) and float(S.ratio(tile[..., :h, :wd], want, A).max()) <= C0
        assert not bool(((tile.sum((0, 2, 3)) - sum64).abs() <= c * sumA).all())
        assert not bool((((tile ** 2).sum((0, 2, 3)) - sq64).abs() <= c * sqA).all())
        return
    assert float(S.ratio(bad, want, A).max()) > C0, mut


def test_one_step_outside_each_predicate_is_refused():
    """conv_sweep.refusal_requests on the host: the planner refuses the config for the shape, and the tuner does not
    hand it out."""
    L = _lib.lib()
    every = frozenset((0, 1, 2, 3))
    texts = {}
    rows = S.refusal_requests()
    assert {S.family_of(c) for c, *_ in rows} >= {'C48', 'F(2x2)', 'Stem', 'F(4x4)', 'Fc', 'S2r'}
    for cfg, key, act, (name, clause), at in rows:
        texts.setdefault(name, S.kernel_text(name))
        assert clause in texts[name], (cfg, name, clause)
        assert tuner.kind_of(cfg) >= 0
        plans = L.egn_conv_plan_query(*key[:11], int(key[12]), cfg, (C.c_int * 12)()) == 0
        takes = L.egn_conv_plan_takes(*key[:11], int(key[11]), int(key[12]), cfg) == 0
        cand = tuner.candidates(key, every, 1 << 20)
        if at == 'plan':
            assert not plans and not takes and cfg not in cand, (cfg, key, clause)
        elif at == 'residual':
            assert not takes and cfg not in cand, (cfg, key, clause)
            assert cfg in tuner.candidates(key[:11] + (False, False), every, 1 << 20), (cfg, key)   # (one step inside)
        else:
            # the activation is no part of a planner query or of the tuner's key: the launcher refuses (GPU test)
            assert at == 'launch' and (act & 0xf) not in (engine.ACT_NONE, engine.ACT_RELU)
