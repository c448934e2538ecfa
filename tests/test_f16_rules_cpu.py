"""The f16-operand lowering rules (precision = 'f16' / 'f16s2' / 'f16x'; engine.F16_RULES, csrc/conv_h.hip's predicate,
csrc/program.hip's add_convh) against what the code recorded BEFORE the rules were stated once -- without a GPU:

  * the op list of HRNet-W48 (256 x 256) and of HRNet-W32 (the Pedestrian model, 256 x 192) at 2 crops under every
    precision, and of W48 at 64 crops with EGONET_AMD_PAIR=1: kind, tag, lane, region, cin, cout, stride, act per op;
  * for every lowered op the class string, flops and bytes ``Program._emit`` reports (bench.py parses the class);
  * the answers of the three ``*_applies`` predicates over a grid that crosses every clause, out-of-range arguments
    included, and the return codes of the three ``egn_program_add_*`` entries on a hand-built program.

tests/golden/program_ops_precisions.json and tests/golden/f16_predicates.npz hold those answers.  They were written by

    PYTHONPATH=. python tests/test_f16_rules_cpu.py --record

on the commit before the rule table existed; ``_parent_cost`` below is that commit's ``_emit`` arithmetic, kept for the
recording alone.  The file is to be recorded again only when a rule is meant to change.
"""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

from egonet_amd import _lib, configs, engine
from egonet_amd.model.heatmapModel import hrnet

HERE = os.path.dirname(os.path.abspath(__file__))
OPS_GOLDEN = os.path.join(HERE, 'golden', 'program_ops_precisions.json')
PRED_GOLDEN = os.path.join(HERE, 'golden', 'f16_predicates.npz')
LOWERED = ('convh', 'convh2', 'convhx')
# name -> (config, crops, height, width, EGONET_AMD_PAIR, precisions)
RECORDINGS = {'w48': (lambda: configs.w48_config('heatmap'), 2, 256, 256, '0', engine.ALL_PRECISIONS),
              'w32': (lambda: configs.ped_config('heatmap'), 2, 256, 192, '0', engine.ALL_PRECISIONS),
              'w48_pair64': (lambda: configs.w48_config('heatmap'), 64, 256, 256, '1', ('f32', 'f16', 'f16x'))}
CASES = [(name, prec) for name, v in RECORDINGS.items() for prec in v[5]]
_cache = {}


def _record(name, prec):
    if (name, prec) not in _cache:
        cfg, n, h, w, pair, _ = RECORDINGS[name]
        saved = {k: os.environ.get(k) for k in ('EGONET_AMD_PAIR', 'EGONET_AMD_AUTOTUNE')}
        os.environ.update(EGONET_AMD_PAIR=pair, EGONET_AMD_AUTOTUNE='0')
        try:
            net = hrnet.get_pose_net(cfg(), is_train=False).eval()
            net.precision = prec
            with torch.no_grad():
                _cache[(name, prec)] = engine.HRNetEngine(net)._record(n, 3, h, w, 1)[0]
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return _cache[(name, prec)]


def _rows(rec):
    return [[kind, op.get('tag', ''), op['lane'], op['region'], op.get('cin'), op.get('cout'), op.get('stride'),
             op.get('act')] for kind, op in rec.ops]


def _keys(rec):
    """kind -> sorted keys of its op dict (``signal`` is set on some ops only: the dependency recording's mark)."""
    out = {}
    for kind, op in rec.ops:
        if kind in LOWERED:
            out.setdefault(kind, set()).add(tuple(sorted(k for k in op if k != 'signal')))
    assert all(len(v) == 1 for v in out.values()), out
    return {kind: list(v.pop()) for kind, v in out.items()}


def _parent_cost(kind, op):
    """[klass, flops, bytes] of a lowered op as ``Program._emit`` computed them before the rule table (the recording)."""
    x, y = op['x'], op['y']
    if kind == 'convh':
        m = x.n * x.h * x.w
        flops = 2.0 * m * op['cout'] * op['cin'] * 9
        nbytes = 4.0 * m * (op['cin'] + op['cout'] * (2 if op['res'] is not None else 1)) + 2.0 * op['cout'] * op['cin'] * 9
        klass = 'conv3x3h %d->%d@%dx%d' % (op['cin'], op['cout'], x.h, x.w)
    elif kind == 'convh2':
        flops = 2.0 * y.n * y.h * y.w * op['cout'] * op['cin'] * 9
        nbytes = 4.0 * (x.n * x.h * x.w * op['cin'] + y.n * y.h * y.w * op['cout']) + 2.0 * op['cout'] * op['cin'] * 9
        klass = 'conv3x3s2h %d->%d@%dx%d' % (op['cin'], op['cout'], y.h, y.w)
    else:
        assert kind == 'convhx'
        flops = 2.0 * y.n * y.h * y.w * op['cout'] * op['cin'] * 9
        nbytes = 4.0 * (x.n * x.h * x.w * op['cin'] + y.n * y.h * y.w * op['cout'] * (2 if op['res'] is not None else 1)) + \
            2.0 * op['cout'] * op['cin'] * 9
        klass = 'conv3x3hx%s %d->%d@%dx%d' % ('s2' if op['stride'] == 2 else '', op['cin'], op['cout'], y.h, y.w)
    return [klass, flops, nbytes]


# ---------------------------------------------------------------------------
# the predicates' grid
# ---------------------------------------------------------------------------
WIDTHS = (3, 32, 48, 64, 96, 128, 192, 256, 384, 512)
ACTS = (engine.ACT_NONE, engine.ACT_RELU, engine.ACT_SIGMOID, engine.ACT_LEAKY, engine.ACT_RELU | engine.ACT_RES_AFTER)
MAPS = ((1, 8), (2, 2), (8, 8), (64, 64))
PADS = ((0, 0), (4, 0), (0, 4), (4, 4))


def _crops(h, w, cin, cout, stride):
    """0, 1, 64, and around the smallest N whose input / output reaches 2 GiB (N - 1 still fits; ceil(2^29 / elements))."""
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    n_in, n_out = -(-2 ** 29 // (h * w * cin)), -(-2 ** 29 // (ho * wo * cout))
    return (0, 1, 64, n_in - 1, n_in, n_out - 1, n_out)


def _predicate_answers():
    """name -> uint8 array of the answers in grid order.  'h' is asked at stride 1 with every has_res, 's2' at stride 2
    (it takes no residual), 'hx' with every stride and has_res."""
    L = _lib.lib()
    out = {'h': [], 's2': [], 'hx': []}
    for cin, cout, (h, w), (pi, po), act in itertools.product(WIDTHS, WIDTHS, MAPS, PADS, ACTS):
        for n in _crops(h, w, cin, cout, 1):
            for has_res in (0, 1, 2):
                out['h'].append(L.egn_conv3x3_h_applies(n, h, w, cin, cin + pi, cout, cout + po, has_res, act))
        for n in _crops(h, w, cin, cout, 2):
            out['s2'].append(L.egn_conv3x3s2_h_applies(n, h, w, cin, cin + pi, cout, cout + po, act))
        for stride in (1, 2, 3):
            for n in _crops(h, w, cin, cout, stride):
                for has_res in (0, 1, 2):
                    out['hx'].append(L.egn_conv3x3_hx_applies(n, h, w, cin, cin + pi, cout, cout + po, has_res, act, stride))
    return {k: np.asarray(v, dtype=np.uint8) for k, v in out.items()}


def _add_answers():
    """The return codes of the three add entries on a program of six slots, 0 .. 3 bound: every ref position valid,
    NULL, unbound (slot 4) and out of range (slot 9), a NULL program, refused shapes and epilogues, a residual where the
    entry takes none -- and (kind, flops, bytes) of every op that was pushed."""
    L = _lib.lib()
    store = torch.zeros(4, 64)
    prog = C.c_void_p(L.egn_program_create(6))
    R = _lib.Ref
    good = [R(0, 0), R(1, 0), R(1, 256), R(1, 512), R(2, 0), R(3, 0)]           # x w scale shift res y

    def entries(p, refs, n, h, w, cin, cout, act, stride):
        x, wp, sc, sh, res, y = refs
        return [('h', lambda: L.egn_program_add_conv3x3_h(p, x, wp, sc, sh, res, y, n, h, w, cin, cout, act)),
                ('s2', lambda: L.egn_program_add_conv3x3s2_h(p, x, wp, sc, sh, y, n, h, w, cin, cout, act)),
                ('hx', lambda: L.egn_program_add_conv3x3_hx(p, x, wp, sc, sh, res, y, n, h, w, cin, cout, act, stride))]
    codes = []
    try:
        for slot in range(4):
            _lib.check(L.egn_program_bind(prog, slot, _lib.ptr(store[slot])))
        shapes = [(2, 8, 8, 48, 96), (2, 8, 8, 64, 64), (2, 8, 8, 40, 48), (0, 8, 8, 48, 48), (2, 1, 8, 64, 64)]
        for (n, h, w, cin, cout), stride, act in itertools.product(shapes, (1, 2, 3), (ACTS[0], ACTS[1], ACTS[2], ACTS[4])):
            for pos in range(6):
                for bad in (good[pos], _lib.NULL_REF, R(4, 0), R(9, 0), R(-2, 64)):
                    refs = list(good)
                    refs[pos] = bad
                    for name, call in entries(prog, refs, n, h, w, cin, cout, act, stride):
                        codes.append(call())
        for name, call in entries(None, good, 2, 8, 8, 48, 48, ACTS[1], 1) + entries(None, good, 2, 8, 8, 64, 64, ACTS[1], 2):
            codes.append(call())
        ops = []
        kind, flops, nbytes = C.c_int(), C.c_double(), C.c_double()
        for i in range(L.egn_program_num_ops(prog)):
            _lib.check(L.egn_program_op_info(prog, i, C.byref(kind), C.byref(flops), C.byref(nbytes), None, 0))
            ops.append([kind.value, flops.value, nbytes.value])
    finally:
        L.egn_program_destroy(prog)
    return {'codes': codes, 'ops': ops}


def _golden():
    if 'golden' not in _cache:
        with open(OPS_GOLDEN) as f:
            _cache['golden'] = json.load(f)
    return _cache['golden']


# ---------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name,prec', CASES)
def test_every_precision_records_the_ops_it_recorded(name, prec):
    want = _golden()['recordings'][name][prec]
    rec = _record(name, prec)
    assert _rows(rec) == want['ops']
    assert _keys(rec) == want['keys']
    counts = {k: sum(1 for kind, _ in rec.ops if kind == k) for k in LOWERED}
    if name == 'w48':
        assert len(rec.ops) == 337
        assert counts == {'f32': dict(convh=0, convh2=0, convhx=0), 'f16': dict(convh=208, convh2=0, convhx=0),
                          'f16s2': dict(convh=208, convh2=29, convhx=0), 'f16x': dict(convh=208, convh2=29, convhx=7)}[prec]
    if name == 'w32':
        assert counts['convh'] == counts['convh2'] == 0 and (counts['convhx'] > 200) == (prec == 'f16x')
    if name == 'w48_pair64':          # a branch any active rule lowers is never half of a pair: 'f32' alone pairs
        pairs = sum(1 for kind, _ in rec.ops if kind == 'convpair')
        assert pairs == want['pairs'] and (pairs > 0) == (prec == 'f32')


@pytest.mark.parametrize('name,prec', CASES)
def test_lowered_ops_agree_with_their_rule_and_cost_what_they_cost(name, prec):
    want = _golden()['recordings'][name][prec]['cost']
    rec = _record(name, prec)
    L = _lib.lib()
    by_kind = {rule.kind: rule for rule in engine.F16_RULES}
    assert tuple(by_kind) == LOWERED
    numel, off = {}, 0
    for t in rec.blobs:
        numel[off] = t.numel()
        off += engine._round_up(t.numel() * 4, 256)
    got = []
    for kind, op in rec.ops:
        if kind not in LOWERED:
            continue
        rule = by_kind[kind]
        assert rule in engine.active_rules(prec)
        assert ('res' in op) == rule.res_arg and ('stride' in op) == rule.stride_arg
        stride = op['stride'] if rule.stride_arg else rule.strides[0]
        assert stride in rule.strides and (op.get('res') is None or stride in rule.res_strides)
        assert (op['y'].h, op['y'].w) == ((op['x'].h - 1) // stride + 1, (op['x'].w - 1) // stride + 1)
        wbytes = {engine.pack_conv_weight_f16: L.egn_conv3x3_h_wpack_bytes,
                  engine.pack_conv_weight_f16x: L.egn_conv3x3_hx_wpack_bytes}[rule.pack](op['cin'], op['cout'])
        assert wbytes > 0 and numel[op['w'].off] * 4 == wbytes
        klass, flops, nbytes = engine.lowered_cost(kind, op)
        assert klass.split(' ')[0] == rule.klass[rule.strides.index(stride)]
        got.append([klass, flops, nbytes])
    assert got == want


def test_the_tables_order_is_the_precisions_order():
    assert [r.mode for r in engine.F16_RULES] == list(engine.ALL_PRECISIONS[1:])
    assert engine.PRECISIONS == ('f32', 'f16', 'f16s2') and engine.ALL_PRECISIONS == ('f32', 'f16', 'f16s2', 'f16x')
    assert engine.active_rules('f32') == ()
    for k, prec in enumerate(engine.ALL_PRECISIONS[1:]):
        assert engine.active_rules(prec) == tuple(engine.F16_RULES[:k + 1])
    with pytest.raises(ValueError, match="'f32', 'f16', 'f16s2' or 'f16x'"):
        engine.active_rules('bf16')
    # the kinds reach ``_push`` through the table: the owner check of tests/test_program_ops_sweep_cpu.py reads engine.py's
    # text, so every kind of the table must be spelled there (a new row's kind then needs its owner)
    import program_ops_sweep
    assert {r.kind for r in engine.F16_RULES} <= program_ops_sweep.pushed_kinds()
    assert tuple(r.kind for r in engine.F16_RULES) == LOWERED
    r = engine._Recorder()
    assert (r.f16, r.f16s2, r.f16x) == (False, False, False)
    r.rules = engine.active_rules('f16s2')
    assert (r.f16, r.f16s2, r.f16x) == (True, True, False)


def test_predicates_answer_as_they_did():
    want = np.load(PRED_GOLDEN)
    got = _predicate_answers()
    for k in ('h', 's2', 'hx'):
        w = np.unpackbits(want[k])[:got[k].size]
        assert got[k].size == int(want[k + '_count']) and 0 < int(got[k].sum()) < got[k].size
        assert set(np.unique(got[k])) <= {0, 1}
        bad = np.nonzero(got[k] != w)[0]
        assert bad.size == 0, (k, bad[:8])


def test_add_entries_return_what_they_returned():
    want = _golden()['add']
    got = _add_answers()
    assert got['codes'] == want['codes'] and set(got['codes']) == {0, -1}
    assert got['ops'] == want['ops'] and {k for k, _, _ in got['ops']} == {12, 13, 14}


if __name__ == '__main__':
    assert sys.argv[1:] == ['--record'], 'usage: python tests/test_f16_rules_cpu.py --record'
    torch.manual_seed(0)
    doc = {'recordings': {}, 'add': _add_answers()}
    for name, prec in CASES:
        rec = _record(name, prec)
        doc['recordings'].setdefault(name, {})[prec] = {
            'ops': _rows(rec), 'keys': _keys(rec), 'pairs': sum(1 for kind, _ in rec.ops if kind == 'convpair'),
            'cost': [_parent_cost(kind, op) for kind, op in rec.ops if kind in LOWERED]}
    with open(OPS_GOLDEN, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    ans = _predicate_answers()
    np.savez_compressed(PRED_GOLDEN, **dict({k: np.packbits(v) for k, v in ans.items()},
                                            **{k + '_count': np.int64(v.size) for k, v in ans.items()}))
    print({k: (int(v.size), int(v.sum())) for k, v in ans.items()}, len(doc['add']['codes']), len(doc['add']['ops']))
