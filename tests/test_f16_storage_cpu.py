"""activations = 'f16' on the host (no GPU): which tensors ``engine.f16_storage`` stores as f16, against an INDEPENDENT
statement of the rule read off the module tree; that the default records what it recorded before; the flags and sizes of
the ops; the host-only predicate egn_conv3x3_h16_applies; bad values and the ABI.

The independent statement: the f16 tensors are exactly
  * the ``conv1`` outputs of the BasicBlocks whose two convolutions are lowered (conv2 is the only reader of
    relu(bn1(conv1(x))); its own output is read by fuse layers, the next block's conv1 AND that block's residual), and
  * the tensors between two neighbouring lowered convolutions of a downsample chain (a transition's or a fuse layer's
    Sequential of (conv, bn[, relu]) units),
where "lowered" is ``engine.eligible`` under one of the precision's active rules -- never ``f16_storage`` itself.
Recordings are host-only, as in tests/program_ops_sweep.py."""
import os
import re

import pytest
import torch
import torch.nn as nn

import f16_mode_case as case48
import f16x_mode_case as case32
from egonet_amd import _lib, configs, engine, plan, synth
from egonet_amd.model.egonet import EgoNet
from egonet_amd.model.heatmapModel import hrnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELU, NONE = engine.ACT_RELU, engine.ACT_NONE
# name -> (config, crops)
MODELS = {
    'tiny-w48': (lambda: case48.config('coordinates'), 3),
    'tiny-w32': (lambda: case32.config('coordinates'), 2),
    'w48': (lambda: configs.w48_config('coordinates'), 2),
    'w32': (lambda: configs.ped_config('coordinates'), 2),
}
# the counts of the rule itself: F16S2_FP32_CLASSES = ((48, 48),), F16X_FP32_CLASSES and F16_STORAGE_FP32_CLASSES empty
COUNTS = {('w48', 'f16'): 104, ('w48', 'f16s2'): 106, ('w48', 'f16x'): 106, ('w32', 'f16x'): 116, ('tiny-w32', 'f16x'): 10}
_NETS, _RECS = {}, {}


def net_of(name):
    """(net, {conv module name: its input shape at the model's crop count}), one torch forward per model."""
    if name not in _NETS:
        mk, n = MODELS[name]
        cfg = mk()
        net = hrnet.get_pose_net(cfg, is_train=False).eval()
        iw, ih = cfg['heatmapModel']['input_size']
        seen = case32.seen_conv_inputs(net, torch.zeros(n, 3, ih, iw))
        _NETS[name] = (net, seen, (n, ih, iw))
    return _NETS[name]


SHIPPED = engine.F16_STORAGE_FP32_CLASSES          # what the measurement left on fp32 storage
EXCEPTIONS = {'all-classes': (), 'shipped': SHIPPED}


def recorded(name, precision, activations, fp32_classes=SHIPPED):
    """(recorder, Program(native=False), its call log) -- shared, never modified by a test."""
    key = (name, precision, activations, fp32_classes)
    if key not in _RECS:
        net, _, (n, ih, iw) = net_of(name)
        net.precision, net.activations = precision, activations
        before, engine.F16_STORAGE_FP32_CLASSES = engine.F16_STORAGE_FP32_CLASSES, fp32_classes
        try:
            eng = engine.HRNetEngine(net)
            assert eng.precision == precision and eng.activations == activations
            with torch.no_grad():
                rec, nslots, _ = eng._record(n, 3, ih, iw, 1)
                log = []
                prog = engine.Program(rec, None, nslots, log=log, native=False)
        finally:
            engine.F16_STORAGE_FP32_CLASSES = before
            del net.precision, net.activations          # (back to the class attributes)
        _RECS[key] = (rec, prog, log)
    return _RECS[key]


def expected_f16_tags(name, precision, fp32_classes):
    """The independent statement: tags of the convolutions whose output is stored as f16; a producer whose
    (cin, cout, stride) is in ``fp32_classes`` keeps fp32 storage."""
    net, seen, _ = net_of(name)
    rules = engine.active_rules(precision)
    mods = dict(net.named_modules())

    def lowered(conv_name):
        conv = mods[conv_name]
        n, _, h, w = seen[conv_name]
        return any(engine.eligible(rule, conv, n, h, w) for rule in rules)

    def stays_fp32(conv_name):
        conv = mods[conv_name]
        return (conv.in_channels, conv.out_channels, conv.stride[0]) in fp32_classes

    want = set()
    for mname, mod in mods.items():
        # BasicBlock: conv1 -> conv2 (+ residual); a Bottleneck has a conv3
        if hasattr(mod, 'conv1') and hasattr(mod, 'conv2') and not hasattr(mod, 'conv3') and mname:
            if lowered(mname + '.conv1') and lowered(mname + '.conv2') and not stays_fp32(mname + '.conv1'):
                want.add(mname + '.conv1')
        # a downsample chain: a Sequential of Sequential(conv, bn[, relu]) units
        if isinstance(mod, nn.Sequential) and len(mod) > 0 and \
                all(isinstance(u, nn.Sequential) and isinstance(u[0], nn.Conv2d) for u in mod):
            for s in range(len(mod) - 1):
                if lowered('%s.%d.0' % (mname, s)) and lowered('%s.%d.0' % (mname, s + 1)) and \
                        not stays_fp32('%s.%d.0' % (mname, s)):
                    want.add('%s.%d' % (mname, s))
    return want


def cases():
    for name in MODELS:
        for precision in engine.ALL_PRECISIONS:
            yield name, precision


@pytest.mark.parametrize('which', sorted(EXCEPTIONS))
@pytest.mark.parametrize('name,precision', list(cases()))
def test_rule_against_the_independent_statement(name, precision, which, monkeypatch):
    fp32_classes = EXCEPTIONS[which]
    monkeypatch.setattr(engine, 'F16_STORAGE_FP32_CLASSES', fp32_classes)
    rec, prog, log = recorded(name, precision, 'f16', fp32_classes)
    got = sorted(b.name for b in rec.bufs if b.f16)
    want = sorted(expected_f16_tags(name, precision, fp32_classes))
    assert got == want, (set(got) ^ set(want))
    assert len(set(got)) == len(got)
    if (name, precision) in COUNTS and not fp32_classes:
        assert len(got) == COUNTS[(name, precision)]
    if fp32_classes:
        assert set(got) <= {b.name for b in recorded(name, precision, 'f16', ())[0].bufs if b.f16}
    if precision == 'f32':
        assert got == []
    if name == 'tiny-w48' and precision != 'f32':
        assert len(got) > 0
    # f16_storage on a fresh recording returns exactly those buffers
    net, _, (n, ih, iw) = net_of(name)
    net.precision = precision
    try:
        with torch.no_grad():
            fresh, _, _ = engine.HRNetEngine(net)._record(n, 3, ih, iw, 1)
    finally:
        del net.precision
    assert not any(b.f16 for b in fresh.bufs)
    assert sorted(b.name for b in engine.f16_storage(fresh)) == got


def strip(log):
    """A call log without what is not comparable: ctypes structures by value."""
    def plain(a):
        if isinstance(a, _lib.Ref):
            return ('ref', a.slot, a.off)
        if isinstance(a, list):
            return [plain(v) for v in a]
        return a
    return [(name, tuple(plain(a) for a in args)) for name, args in log]


@pytest.mark.parametrize('name,precision', list(cases()))
def test_default_and_f32_record_what_they_recorded(name, precision):
    """activations = 'f32': no op carries a flag, no buffer is f16, no _h16 call -- the recording does not pass through
    ``f16_storage`` at all, so it is the parent's, op for op.  precision = 'f32' with activations = 'f16': the same log."""
    rec, prog, log = recorded(name, precision, 'f32')
    assert not any(b.f16 for b in rec.bufs)
    assert not any('x16' in op or 'y16' in op for _, op in rec.ops)
    assert not any('_h16' in call for call, _ in log)
    assert all(b.nbytes == b.n * b.h * b.w * b.cs * 4 for b in rec.bufs if b.slot == engine.SLOT_ARENA)
    rec16, prog16, log16 = recorded(name, precision, 'f16', ())
    assert [k for k, _ in rec16.ops] == [k for k, _ in rec.ops]
    assert [op.get('tag') for _, op in rec16.ops] == [op.get('tag') for _, op in rec.ops]
    if precision == 'f32':
        assert strip(log16) == strip(log) and prog16.arena_bytes == prog.arena_bytes
    else:
        # the calls differ exactly at the ops with a flag
        flagged = [op['tag'] for _, op in rec16.ops if op.get('x16') or op.get('y16')]
        assert sum(1 for call, _ in log16 if call == 'egn_program_add_conv3x3_h16') == len(flagged)
        assert len(log16) == len(log)
        adds = {rule.add for rule in engine.F16_RULES}
        for (c, _), (c16, _) in zip(log, log16):
            assert c in adds if c16 == 'egn_program_add_conv3x3_h16' else c == c16


def test_default_switch_is_f32_and_separate_from_precision():
    assert hrnet.PoseHighResolutionNet.activations == 'f32'
    assert engine.ACTIVATIONS == ('f32', 'f16')
    assert isinstance(SHIPPED, tuple) and all(isinstance(c, tuple) and len(c) == 3 for c in SHIPPED)
    assert len(set(SHIPPED)) == len(SHIPPED)
    assert 'f16' in engine.ALL_PRECISIONS and len(engine.ALL_PRECISIONS) == 4
    net, _, _ = net_of('tiny-w32')
    assert engine.HRNetEngine(net).activations == 'f32'


@pytest.mark.parametrize('which', sorted(EXCEPTIONS))
@pytest.mark.parametrize('name,precision', [(n, p) for n, p in cases() if p != 'f32'])
def test_op_flags_and_sizes(name, precision, which):
    rec, prog, log = recorded(name, precision, 'f16', EXCEPTIONS[which])
    rec32, prog32, _ = recorded(name, precision, 'f32')
    f16 = [b for b in rec.bufs if b.f16]
    lowered = set(engine._RULE_OF_KIND)
    for b in f16:
        assert b.slot == engine.SLOT_ARENA and b.cs == b.c
        assert b.nbytes == b.n * b.h * b.w * b.c * 2
        writers = [(k, op) for k, op in rec.ops if op.get('y') is b]
        assert len(writers) == 1 and writers[0][0] in lowered
        assert writers[0][1].get('y16') is True and writers[0][1].get('res') is None
        users = [(k, op) for i, (k, op) in enumerate(rec.ops) if i in b.uses and op.get('y') is not b]
        assert users
        for k, op in users:
            assert k in lowered and op['x'] is b and op.get('x16') is True and op.get('res') is not b
    # no flag without its buffer
    for k, op in rec.ops:
        if k in lowered:
            assert bool(op.get('x16')) == op['x'].f16 and bool(op.get('y16')) == op['y'].f16
        else:
            assert 'x16' not in op and 'y16' not in op
    # the calls: the storage flags arrive as recorded, chunk size and stride as the kind has them
    calls = [args for call, args in log if call == 'egn_program_add_conv3x3_h16']
    ops = [(k, op) for k, op in rec.ops if k in lowered and (op.get('x16') or op.get('y16'))]
    assert len(calls) == len(ops)
    for args, (k, op) in zip(calls, ops):
        rule = engine._RULE_OF_KIND[k]
        stride = op['stride'] if rule.stride_arg else rule.strides[0]
        assert args[6:] == (op['x'].n, op['x'].h, op['x'].w, op['cin'], op['cout'], op['act'], stride,
                            32 if k == 'convhx' else 48, int(bool(op.get('x16'))), int(bool(op.get('y16'))))
        assert _lib.lib().egn_conv3x3_h16_applies(op['x'].n, op['x'].h, op['x'].w, op['cin'], op['cin'], op['cout'], op['cout'],
                                                  int(op.get('res') is not None), op['act'], *args[12:]) == 1
    # bytes: lowered_cost counts an f16 tensor as 2 bytes an element, the class names stay
    for (k, op), (k32, op32) in zip(rec.ops, rec32.ops):
        if k in lowered:
            klass, flops, nbytes = engine.lowered_cost(k, op)
            klass32, flops32, nbytes32 = engine.lowered_cost(k32, op32)
            x, y = op['x'], op['y']
            saved = 2.0 * (x.n * x.h * x.w * op['cin'] * bool(op.get('x16')) + y.n * y.h * y.w * op['cout'] * bool(op.get('y16')))
            assert (klass, flops) == (klass32, flops32) and nbytes == nbytes32 - saved
            assert re.match(r'conv3x3(h|s2h|hx|hxs2) \d+->\d+@\d+x\d+$', klass)
    assert prog.arena_bytes <= prog32.arena_bytes
    assert [m['klass'] for m in prog.meta] == [m['klass'] for m in prog32.meta]


def test_exception_tuple_is_read_at_call_time(monkeypatch):
    """A producer class in F16_STORAGE_FP32_CLASSES keeps fp32 storage; the tuple is looked up at every call."""
    net, _, (n, ih, iw) = net_of('tiny-w32')
    net.precision = 'f16x'
    try:
        with torch.no_grad():
            a, _, _ = engine.HRNetEngine(net)._record(n, 3, ih, iw, 1)
            b, _, _ = engine.HRNetEngine(net)._record(n, 3, ih, iw, 1)
    finally:
        del net.precision
    monkeypatch.setattr(engine, 'F16_STORAGE_FP32_CLASSES', ())
    full = engine.f16_storage(a)
    classes = {(op['cin'], op['cout'], op.get('stride', 1)) for k, op in a.ops if op.get('y16')}
    assert (32, 32, 1) in classes
    monkeypatch.setattr(engine, 'F16_STORAGE_FP32_CLASSES', ((32, 32, 1),))
    fewer = engine.f16_storage(b)
    assert 0 < len(fewer) < len(full)
    assert not any((op['cin'], op['cout'], op.get('stride', 1)) == (32, 32, 1) for k, op in b.ops if op.get('y16'))


# ---------------------------------------------------------------------------
# the predicate, host only
# ---------------------------------------------------------------------------
def test_predicate_refuses():
    P = _lib.lib().egn_conv3x3_h16_applies
    ok48 = (2, 8, 8, 48, 48, 48, 48)
    ok32 = (2, 8, 8, 64, 64, 64, 64)
    assert P(*ok48, 0, RELU, 1, 48, 1, 1) == 1 and P(*ok32, 0, RELU, 1, 32, 1, 1) == 1
    assert P(*ok48, 1, RELU, 1, 48, 1, 0) == 1 and P(*ok32, 1, RELU, 1, 32, 1, 0) == 1
    assert P(*ok48, 0, NONE, 2, 48, 0, 1) == 1 and P(*ok32, 0, NONE, 2, 32, 1, 1) == 1
    for ok, ck in ((ok48, 48), (ok32, 32)):
        assert P(*ok, 1, RELU, 1, ck, 0, 1) == 0 and P(*ok, 1, RELU, 1, ck, 1, 1) == 0       # y_f16 with a residual
        for bad_ck in (0, 16, 24, 40, 64, 96, -48):
            assert P(*ok, 0, RELU, 1, bad_ck, 1, 1) == 0
        for xf, yf in ((2, 0), (0, 2), (-1, 0), (0, -1), (3, 1), (1, 256)):
            assert P(*ok, 0, RELU, 1, ck, xf, yf) == 0
        for stride in (0, 3, 4, -1):
            assert P(*ok, 0, RELU, stride, ck, 1, 1) == 0
        assert P(*ok, 1, RELU, 2, ck, 1, 0) == 0                                             # a residual at stride 2
        assert P(*ok, 0, engine.ACT_SIGMOID, 1, ck, 1, 1) == 0
        assert P(ok[0], 1, 8, *ok[3:], 0, RELU, 1, ck, 1, 1) == 0                            # H < 2
        assert P(*ok[:4], ok[4] + 4, *ok[5:], 0, RELU, 1, ck, 1, 1) == 0                     # a padded channel stride
    # widths: each chunk size takes its own only
    assert P(*ok48, 0, RELU, 1, 32, 1, 1) == 0 and P(*ok32, 0, RELU, 1, 48, 1, 1) == 0
    assert P(2, 8, 8, 40, 40, 48, 48, 0, RELU, 1, 48, 1, 1) == 0
    assert P(2, 8, 8, 64, 64, 192, 192, 0, RELU, 1, 32, 1, 1) == 0
    # the 2 GiB condition stays at fp32 sizes: 1024 x 64 x 128 x 64 x 4 bytes = 2 GiB is refused although the f16 tensor is 1 GiB
    assert P(1024, 64, 128, 64, 64, 64, 64, 0, RELU, 1, 32, 1, 1) == 0
    assert P(1023, 64, 128, 64, 64, 64, 64, 0, RELU, 1, 32, 1, 1) == 1


def test_predicate_with_both_flags_0_is_the_three_existing_ones():
    L = _lib.lib()
    P = L.egn_conv3x3_h16_applies
    widths = (3, 32, 40, 48, 64, 96, 128, 192, 256, 384, 512)
    checked = 0
    for n, h, w in ((1, 2, 2), (2, 8, 6), (3, 1, 8), (64, 64, 64), (400, 128, 128)):
        for cin in widths:
            for cout in widths:
                for has_res in (0, 1, 2):
                    for act in (NONE, RELU, engine.ACT_SIGMOID):
                        for xf, yf in ((0, 0), (1, 0)):
                            a = (n, h, w, cin, cin, cout, cout)
                            assert P(*a, has_res, act, 1, 48, xf, yf) == L.egn_conv3x3_h_applies(*a, has_res, act)
                            assert P(*a, has_res, act, 1, 32, xf, yf) == L.egn_conv3x3_hx_applies(*a, has_res, act, 1)
                            assert P(*a, has_res, act, 2, 32, xf, yf) == L.egn_conv3x3_hx_applies(*a, has_res, act, 2)
                            if has_res == 0:
                                assert P(*a, 0, act, 2, 48, xf, yf) == L.egn_conv3x3s2_h_applies(*a, act)
                            else:
                                assert P(*a, has_res, act, 2, 48, xf, yf) == 0
                            checked += 1
        # a padded channel stride on either side
        assert P(n, h, w, 48, 52, 48, 48, 0, RELU, 1, 48, 0, 0) == L.egn_conv3x3_h_applies(n, h, w, 48, 52, 48, 48, 0, RELU) == 0
        assert P(n, h, w, 64, 64, 64, 68, 0, RELU, 1, 32, 0, 0) == L.egn_conv3x3_hx_applies(n, h, w, 64, 64, 64, 68, 0, RELU, 1) == 0
    assert checked > 10000


# ---------------------------------------------------------------------------
# bad values and the ABI
# ---------------------------------------------------------------------------
def test_bad_values_raise():
    cfg = case32.config('coordinates')
    cfg['heatmapModel']['activations'] = 'bf16'
    with pytest.raises(ValueError, match='activations'):
        hrnet.get_pose_net(cfg, is_train=False)
    with pytest.raises(ValueError, match='activations'):
        EgoNet(cfg, pre_trained=False)
    with pytest.raises(ValueError, match='activations'):
        EgoNet(case32.config('coordinates'), pre_trained=False, activations='bf16')
    cfg['heatmapModel']['activations'] = 'f16'
    assert hrnet.get_pose_net(cfg, is_train=False).activations == 'f16'
    assert EgoNet(cfg, pre_trained=False).HC.activations == 'f16'
    assert EgoNet(cfg, pre_trained=False, activations='f32').HC.activations == 'f32'
    assert EgoNet(case32.config('coordinates'), pre_trained=False).HC.activations == 'f32'
    net = hrnet.get_pose_net(case32.config('coordinates'), is_train=False).eval()
    net.activations = 'bf16'
    eng = engine.HRNetEngine(net)
    with pytest.raises(ValueError, match='activations'):
        eng.activations
    with pytest.raises(ValueError, match='activations'):
        eng._record(1, 3, case32.HEIGHT, case32.WIDTH, None)
    with pytest.raises(ValueError, match='activations'):
        eng.program(torch.zeros(1, 3, case32.HEIGHT, case32.WIDTH))
    # 'f16' is not a precision of its own and the precision values are no activations
    for v in ('f16s2', 'f16x', 'F16', None, 16):
        with pytest.raises(ValueError):
            engine.check_activations(v)


def test_export_plan_refuses_the_switch(tmp_path):
    cfg = configs.tiny_config('coordinates', num_joints=5)
    ego = EgoNet(cfg, pre_trained=False, activations='f16')
    ego.LS = synth.synth_lifter_stats(10, 12, seed=1)
    ego.eval()
    path = str(tmp_path / 'no.egnplan')
    with pytest.raises(ValueError, match='activations'):
        plan.export_plan(ego, path, batch_sizes=(1,), device=None)
    assert not os.path.exists(path)
    ego.HC.activations = 'f32'
    plan.export_plan(ego, path, batch_sizes=(1,), device=None)
    assert os.path.getsize(path) > 0


def test_tool_has_its_own_argument():
    text = open(os.path.join(ROOT, 'tools', 'inference_kitti.py')).read()
    assert "ap.add_argument('--activations', default='f32', choices=['f32', 'f16']," in text
    assert "activations=a.activations" in text


def test_symbols_in_the_header_and_bound():
    header = open(os.path.join(ROOT, 'include', 'egonet_hip.h')).read()
    L = _lib.lib()
    for name, nargs in (('egn_conv3x3_h16_applies', 13), ('egn_conv3x3_h16_f32', 17), ('egn_program_add_conv3x3_h16', 17)):
        m = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert m, name
        assert len(m.group(1).split(',')) == nargs, (name, m.group(1))
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    # the existing entries keep their signatures
    assert len(L.egn_conv3x3_h_f32.argtypes) == 13 and len(L.egn_conv3x3s2_h_f32.argtypes) == 12
    assert len(L.egn_conv3x3_hx_f32.argtypes) == 14
    assert len(L.egn_program_add_conv3x3_h.argtypes) == 13 and len(L.egn_program_add_conv3x3s2_h.argtypes) == 12
    assert len(L.egn_program_add_conv3x3_hx.argtypes) == 14
