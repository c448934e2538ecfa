"""Every op of an inference program that is not a convolution -- 'pwpair', 'fuse', 'to_nhwc', 'to_nchw', 'pixshuf',
'ramps', 'decode' -- as the product records it and at the edges of its kernel, element by element against float64 /
the index formula.

The requests, inputs, references and bounds are those of tests/program_ops_sweep.py.  Every request runs through its
direct entry point on each of its input sets, and every launch is checked for:
  1. outputs pre-filled with NaN (a sentinel where only part is written): every element that should be written is,
     under the rule of the input set (bit equality / the element-wise bound), nothing else changes;
  2. guard bands around every written buffer, and the floats in front of an operand that starts inside its allocation;
  3. inputs bit-identical afterwards;
  4. NaN in the input pad the kernel must not read (pad channels of 'to_nchw' / 'pixshuf', 64 floats behind every input):
     a read of it shows in the output;
  5. the same bits from a second launch.
Every distinct recorded request runs once more as a one-op program inside a fork / join on lane 1: the bits of the
direct entry point, one launch counted.  A summary per kind (requests, launches, worst |err| / (2^-24 A) and where) is
printed.
"""
import ctypes

import pytest
import torch

import program_ops_sweep as P
from egonet_amd import _lib
from sweep_guards import _guarded, _guards_intact

pytestmark = pytest.mark.gpu

LEAD = 7.0                    # what the floats in front of an offset operand hold
TAIL = 64                     # NaN floats behind every input


def _G():
    return 2 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Buffers(object):
    """Device storage of one request on one set of inputs."""

    def __init__(self, r, x):
        self.r = r
        lead_out = r['lead'] if r['kind'] == 'pwpair' else 0
        self.ins, self.outs = {}, {}
        for name, t in x.items():
            whole = torch.full((r['lead'] + t.numel() + TAIL,), float('nan'), device='cuda')
            whole[:r['lead']] = LEAD
            whole[r['lead']:r['lead'] + t.numel()] = t.cuda()
            self.ins[name] = (whole, whole[r['lead']:r['lead'] + t.numel()], whole.clone())
        for name, numel in P.out_numel(r).items():
            whole, body = _guarded(numel + lead_out, torch.float32, None)
            self.outs[name] = (whole, body[:lead_out], body[lead_out:])

    def prefill(self):
        for whole, lead, body in self.outs.values():
            lead.fill_(LEAD)
            body.fill_(P.SENTINEL if self.r['kind'] == 'ramps' else float('nan'))

    def tensor(self, name):
        if name in self.ins:
            return self.ins[name][1]
        return self.outs[name][2] if name in self.outs else None

    def ptr(self, name):
        t = self.tensor(name)
        return None if t is None else _lib.ptr(t)

    def got(self):
        return {name: v[2].clone() for name, v in self.outs.items()}

    def intact(self):
        fails = []
        for name, (whole, lead, body) in self.outs.items():
            if not _guards_intact(whole) or not bool((lead == LEAD).all()):
                fails.append('write in front of / behind %s' % name)
        for name, (whole, view, keep) in self.ins.items():
            if not torch.equal(_bits(whole), _bits(keep)):
                fails.append('input %s changed' % name)
        return fails


def _same_bits(first, got, what):
    return ['%s: different bits in %s' % (what, n) for n in first if not torch.equal(_bits(first[n]), _bits(got[n]))]


def _direct(r, case):
    """Both launches of one request on one set of inputs: (worst ratio, failures, notes, buffers, first result)."""
    x = P.inputs(r, case)
    B = _Buffers(r, x)
    st = _lib.current_stream()
    worst, fails, notes, first = 0.0, [], {}, None
    for rep in range(2):
        B.prefill()
        rc = P.call_direct(r, B.ptr, st)
        torch.cuda.synchronize()
        if rc != 0:
            fails.append('launch %d returned %d (%s)' % (rep, rc, _lib.lib().egn_strerror(rc).decode()))
            break
        fails += B.intact()
        got = B.got()
        if rep == 0:
            worst, f, notes = P.check(r, case, x, got)
            fails += f
            first = got
        else:
            fails += _same_bits(first, got, 'second launch')
    return worst, fails, notes, B, first


def _as_program(r, B, first):
    """The request as a one-op program inside a fork / join on lane 1, on the buffers of the direct launches."""
    L = _lib.lib()
    names = [n for n in P.IN_NAMES[r['kind']] + P.OUT_NAMES[r['kind']] if B.tensor(n) is not None]
    prog = ctypes.c_void_p(L.egn_program_create(len(names) + 1))
    assert prog
    fails = []
    try:
        for slot, n in enumerate(names):
            _lib.check(L.egn_program_bind(prog, slot, _lib.ptr(B.tensor(n))))
        ref = lambda n: _lib.Ref(names.index(n), 0) if n in names else _lib.NULL_REF
        _lib.check(L.egn_program_fork(prog))
        _lib.check(L.egn_program_set_lane(prog, 1))
        _lib.check(P.add_to_program(r, prog, ref), 'add')
        _lib.check(L.egn_program_tag(prog, b'the.swept.op', 0.0, 0.0))
        _lib.check(L.egn_program_join(prog))
        B.prefill()
        n0 = L.egn_launch_count()
        _lib.check(L.egn_program_run(prog, _lib.current_stream()), 'run')
        torch.cuda.synchronize()
        if L.egn_launch_count() - n0 != 1:
            fails.append('program: %d launches counted' % (L.egn_launch_count() - n0))
        fails += B.intact() + _same_bits(first, B.got(), 'program')
    finally:
        L.egn_program_destroy(prog)
    return fails


def _describe(r):
    return ' '.join('%s %s' % (k, r[k]) for k in sorted(r) if k not in ('kind', 'srcs', 'line', 'null', 'lead')) + \
        (' null %s' % (r['null'],) if r['null'] else '') + (' lead %d' % r['lead'] if r['lead'] else '')


def _sweep(reqs, origin, program):
    ent = dict(requests=0, launches=0, worst=0.0, where='-', bound=0.0)
    fails = []
    for r in reqs:
        ent['requests'] += 1
        for case in P.cases_of(r):
            w, f, notes, B, first = _direct(r, case)
            ent['launches'] += 2
            if program and first is not None and case == 'rounding':
                f += _as_program(r, B, first)
                ent['launches'] += 1
            if w >= ent['worst'] and w > 0:
                ent['worst'], ent['where'] = w, '%s %s (%s)' % (origin, _describe(r), r['srcs'][0])
            ent['bound'] = max(ent['bound'], notes.get('bound_max', 0.0))
            fails += ['%s %s %s (%s %s): %s' % (r['kind'], _describe(r), case, origin, r['srcs'][0], m) for m in f]
            del B, first
    return ent, fails


def _report(kind, ent):
    const = {'pwpair': 'C %g' % P.C_PW, 'decode': 'C %g' % P.C_DEC, 'fuse': 'C = nterms'}.get(kind, 'bit for bit')
    print('%-8s %4d requests %5d launches  worst %5.2f (%s)  %s' % (kind, ent['requests'], ent['launches'], ent['worst'],
                                                                    const, ent['where']))
    if kind == 'decode':
        print('         largest soft-arg-max allowance of any map: %.3g pixels (tests/test_gpu_decode.py: 1e-3 / 1e-4)'
              % ent['bound'])


@pytest.mark.parametrize('kind', P.KINDS)
def test_every_recorded_request_matches_float64(kind):
    G = _G()
    reqs = P.merged([P.replayed(r, G) for r in P.recorded_requests() if r['kind'] == kind])
    assert reqs
    ent, fails = _sweep(reqs, 'recorded', program=True)
    print()
    _report(kind, ent)
    torch.cuda.empty_cache()
    assert not fails, '%d failures:\n%s' % (len(fails), '\n'.join(fails[:40]))


@pytest.mark.parametrize('kind', P.KINDS)
def test_every_edge_request_matches_float64(kind):
    reqs = [r for r in P.merged(P.edge_requests(_G())) if r['kind'] == kind]
    assert reqs
    ent, fails = _sweep(reqs, 'edge', program=False)
    print()
    _report(kind, ent)
    torch.cuda.empty_cache()
    assert not fails, '%d failures:\n%s' % (len(fails), '\n'.join(fails[:40]))


def _refused(r, x, call=None, swap=None):
    """The call is refused and nothing is launched: every output keeps its pre-fill, the guard bands theirs.  Buffers
    are those of the sound request ``r``; ``call``: the request passed instead; ``swap``: {operand: the operand whose
    address it gets, 'absent' for NULL}."""
    B = _Buffers(r, x)
    B.prefill()
    ptr = lambda n: B.ptr((swap or {}).get(n, n))
    rc = P.call_direct(call or r, ptr, _lib.current_stream())
    torch.cuda.synchronize()
    fill = P.SENTINEL if r['kind'] == 'ramps' else float('nan')
    want = torch.full((1,), fill, device='cuda').view(torch.int32)
    untouched = all(bool((_bits(v[2]) == want).all()) for v in B.outs.values())
    return rc != 0 and untouched and not B.intact()


def test_the_pw_pair_refuses_what_it_cannot_run():
    """M % 32, M <= 0, res == out, h == hn, w1 without hn and the reverse: refused, nothing launched.  (The 2 GB limit
    is not tried on the GPU.)"""
    base = [r for r in P.edge_requests(_G()) if r['kind'] == 'pwpair' and r['M'] == 64 and r['fused'] and r['res']][0]
    x = P.inputs(base, 'exact')
    assert _refused(base, x, call=dict(base, M=48))
    assert _refused(base, x, call=dict(base, M=0))
    assert _refused(base, x, call=dict(base, M=-32))
    assert _refused(base, x, swap={'res': 'out'})
    assert _refused(base, x, swap={'h': 'hn'})
    assert _refused(base, x, swap={'hn': 'absent'})
    assert _refused(base, x, swap={'w1': 'absent'})
    w, fails, _, _, _ = _direct(base, 'exact')
    assert not fails, fails


def test_a_program_op_that_aliases_res_and_out_is_never_launched():
    L = _lib.lib()
    r = [q for q in P.edge_requests(_G()) if q['kind'] == 'pwpair' and q['M'] == 64 and q['fused'] and q['res']][0]
    B = _Buffers(r, P.inputs(r, 'exact'))
    B.prefill()
    names = list(P.IN_NAMES['pwpair'] + P.OUT_NAMES['pwpair'])
    prog = ctypes.c_void_p(L.egn_program_create(len(names) + 1))
    assert prog
    try:
        for slot, n in enumerate(names):
            _lib.check(L.egn_program_bind(prog, slot, _lib.ptr(B.tensor(n))))
        ref = lambda n: _lib.Ref(names.index('out' if n == 'res' else n), 0)
        rc = P.add_to_program(r, prog, ref)
        if rc == 0:
            rc = L.egn_program_run(prog, _lib.current_stream())
        torch.cuda.synchronize()
        assert rc != 0
        assert all(bool(torch.isnan(v[2]).all()) for v in B.outs.values()) and not B.intact()
    finally:
        L.egn_program_destroy(prog)


def test_the_elementwise_launchers_refuse_what_they_cannot_run():
    """fuse: H or W not divisible by 2^s, 0 and 5 terms, cs % 4; ramps: c0 + 2 > cs; the layout changes: cs below what
    is read or written.  Refused, nothing launched."""
    L = _lib.lib()
    st = _lib.current_stream()
    f = P._req('fuse', 'refusals', N=1, H=6, W=8, C=8, cs=8, shifts=(0, 1), relu=1)
    x = P.inputs(f, 'exact')
    assert _refused(f, x, call=dict(f, H=5))
    assert _refused(f, x, call=dict(f, W=7))
    assert _refused(f, x, call=dict(f, shifts=(0, 2)))                      # 6 >> 2 << 2 != 6
    assert _refused(f, x, call=dict(f, cs=6, C=6))
    whole, y = _guarded(6 * 8 * 8, torch.float32, float('nan'))
    t = torch.zeros(6 * 8 * 8, device='cuda')
    for n in (0, 5):
        terms = (ctypes.c_void_p * 5)(*[_lib.ptr(t)] * 5)
        shifts = (ctypes.c_int * 5)(0, 0, 0, 0, 0)
        assert L.egn_fuse_sum_relu_f32(_lib.ptr(y), 1, 6, 8, 8, 8, n, terms, shifts, 1, st) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and _guards_intact(whole)
    m = P._req('ramps', 'refusals', N=1, H=5, W=7, cs=8, c0=6)
    assert _refused(m, {}, call=dict(m, c0=7)) and _refused(m, {}, call=dict(m, c0=-1))
    n = P._req('to_nhwc', 'refusals', N=1, C=6, H=5, W=7, cs=8)
    xn = P.inputs(n, 'rounding')
    assert _refused(n, xn, call=dict(n, cs=6)) and _refused(n, xn, call=dict(n, cs=4))
    c = P._req('to_nchw', 'refusals', N=1, C=6, H=5, W=7, cs=8)
    assert _refused(c, P.inputs(c, 'rounding'), call=dict(c, cs=5))
    p = P._req('pixshuf', 'refusals', N=1, C=3, H=5, W=7, cs=12, up=2)
    xp = P.inputs(p, 'rounding')
    assert _refused(p, xp, call=dict(p, cs=11)) and _refused(p, xp, call=dict(p, up=0))
