"""precision = 'f16s2' without a GPU: 'f16' plus the 3x3 / stride 2 / pad 1 layers on the f16-operand kernel
(csrc/conv_h.hip with S = 2).  The host-only predicate, ``engine.f16s2_eligible``, what the recorder lowers, the switch --
and that 'f16' and its emulation are what they were.  The layers in the reference: libs/model/heatmapModel/hrnet.py, the
stride-2 units of the transition and fuse layers (fp32 torch calls)."""
import json

import pytest
import torch
import torch.nn as nn

import f16s2_mode_case as case
from egonet_amd import _lib, configs, engine, tuner
from egonet_amd.model.heatmapModel import hrnet

RELU, NONE = engine.ACT_RELU, engine.ACT_NONE
WIDTHS = (48, 96, 192, 384)


def _is_s2(m):
    return isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (2, 2)


def test_predicate_answers():
    L = _lib.lib()
    for cin in WIDTHS:                  # the class grid, at the sizes of the kernel test and of W48
        for cout in WIDTHS:
            for n, h, w in ((1, 8, 8), (64, 64, 64), (16, 32, 32), (5, 4, 4), (4, 2, 2), (2, 7, 9)):
                for act in (RELU, NONE):
                    assert L.egn_conv3x3s2_h_applies(n, h, w, cin, cin, cout, cout, act) == 1, (n, h, w, cin, cout, act)
    no = [(64, 64, 64, 40, 40, 48, 48, RELU),                   # Cin = 40
          (64, 64, 64, 256, 256, 96, 96, RELU),                 # transition1: 256 -> 96
          (64, 128, 128, 64, 64, 64, 64, RELU),                 # the stem's 64 -> 64
          (64, 64, 64, 48, 52, 48, 48, RELU),                   # padded channel strides
          (64, 64, 64, 48, 48, 48, 52, RELU),
          (64, 64, 64, 48, 48, 48, 48, engine.ACT_SIGMOID),
          (64, 64, 64, 48, 48, 48, 48, engine.ACT_LEAKY),
          (0, 8, 8, 48, 48, 48, 48, RELU),                      # N = 0
          (1, 1, 8, 48, 48, 48, 48, RELU), (1, 8, 1, 48, 48, 48, 48, RELU),       # H = 1, W = 1
          (4096, 64, 64, 48, 48, 48, 48, RELU),                 # a 3 GiB input: 32-bit offsets
          (2048, 64, 64, 48, 48, 384, 384, RELU)]               # (1.5 GiB in, 3 GiB out)
    for a in no:
        assert L.egn_conv3x3s2_h_applies(*a) == 0, a


def test_f16s2_eligible_never_offers_other_layers(monkeypatch):
    assert engine.F16S2_FP32_CLASSES == () or all(len(c) == 2 for c in engine.F16S2_FP32_CLASSES)
    conv = nn.Conv2d(48, 96, 3, 2, 1, bias=False)
    if (48, 96) not in engine.F16S2_FP32_CLASSES:
        assert engine.f16s2_eligible(conv, 3, 16, 16)
    assert not engine.f16_eligible(conv, 3, 16, 16)
    assert not engine.f16s2_eligible(nn.Conv2d(48, 48, 3, 1, 1, bias=False), 3, 16, 16)      # stride 1: 'f16' has it
    assert not engine.f16s2_eligible(nn.Conv2d(48, 48, 1, 1, 0, bias=False), 3, 16, 16)
    assert not engine.f16s2_eligible(nn.Conv2d(48, 48, 1, 2, 0, bias=False), 3, 16, 16)
    assert not engine.f16s2_eligible(nn.Conv2d(48, 96, 3, 2, 1, bias=True), 3, 16, 16)
    assert not engine.f16s2_eligible(nn.Conv2d(48, 96, 3, 2, 1, bias=False, groups=2), 3, 16, 16)
    assert not engine.f16s2_eligible(nn.Conv2d(48, 96, 3, 2, 2, bias=False, dilation=2), 3, 16, 16)
    assert not engine.f16s2_eligible(nn.Conv2d(48, 96, 3, 2, 1, bias=False, padding_mode='reflect'), 3, 16, 16)
    assert not engine.f16s2_eligible(nn.Conv2d(40, 96, 3, 2, 1, bias=False), 3, 16, 16)
    assert not engine.f16s2_eligible(nn.Conv2d(256, 96, 3, 2, 1, bias=False), 3, 16, 16)
    assert not engine.f16s2_eligible(nn.BatchNorm2d(48), 3, 16, 16)
    # a class measured not to win is left on fp32, by the rule and by the recorder alike
    monkeypatch.setattr(engine, 'F16S2_FP32_CLASSES', ((48, 96),))
    assert not engine.f16s2_eligible(conv, 3, 16, 16)
    assert engine.f16s2_eligible(nn.Conv2d(96, 96, 3, 2, 1, bias=False), 3, 16, 16)
    x = engine.Buf(3, 16, 16, 48)
    assert not engine._Recorder.takes_f16s2(x, conv.weight, None, RELU, None, 2, 1)
    monkeypatch.setattr(engine, 'F16S2_FP32_CLASSES', ())
    assert engine._Recorder.takes_f16s2(x, conv.weight, None, RELU, None, 2, 1)
    # what the recorder's question refuses beside the rule's
    assert not engine._Recorder.takes_f16s2(x, conv.weight, torch.zeros(96), RELU, None, 2, 1)          # a bias
    assert not engine._Recorder.takes_f16s2(x, conv.weight, None, RELU, None, 2, 1, out_nchw=True)
    assert not engine._Recorder.takes_f16s2(x, conv.weight, None, RELU, None, 2, 1, cout_cs=100)
    assert not engine._Recorder.takes_f16s2(x, conv.weight, None, RELU, None, 2, 1, dst_given=True)
    assert not engine._Recorder.takes_f16s2(x, conv.weight, None, engine.ACT_SIGMOID, None, 2, 1)
    assert not engine._Recorder.takes_f16s2(x, conv.weight, None, RELU, None, 1, 1)


def _measured_fp32(m):
    return (m.in_channels, m.out_channels) in engine.F16S2_FP32_CLASSES


def _summary(rec, monkeypatch):
    """(kind, tag, tile configuration the shipped table answers, region, lane) per op."""
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    out = []
    for kind, op in rec.ops:
        cfg = tuner.choose(None, engine.Program._conv_key(op), engine.Program._conv_kinds(op)) if kind == 'conv' else None
        out.append((kind, op.get('tag', ''), cfg, op.get('region'), op.get('lane')))
    return out


def _tag(name):
    """Module name of a convolution -> the tag the recorder gives its layer: the transition and fuse units are recorded
    under the name of their Sequential(conv, bn[, relu])."""
    return name[:-2] if name.startswith(('transition', 'stage')) and '.branches.' not in name and name.endswith('.0') \
        else name


def test_f16s2_recording_lowers_exactly_the_eligible_layers(monkeypatch):
    """On the GPU test's model (W48 widths, 64 x 64 input): the lowered tags are the modules ``f16_eligible`` or
    ``f16s2_eligible`` name with the input shapes the torch forward shows them; everything else is recorded exactly as
    in 'f32', and 'f16' records what it recorded before the wider mode existed."""
    net = case.model('coordinates')
    seen = case.seen_conv_inputs(net, case.crops('forward'))
    mods = dict(net.named_modules())
    el1 = {_tag(name) for name, (n, c, h, w) in seen.items() if engine.f16_eligible(mods[name], n, h, w)}
    el2 = {_tag(name) for name, (n, c, h, w) in seen.items() if engine.f16s2_eligible(mods[name], n, h, w)}
    # the stride-2 count, from the module list
    s2 = {_tag(name) for name, m in mods.items() if _is_s2(m)}
    left = sorted(s2 - el2)
    assert len(el1) == 18 and len(el2) > 0 and not (el1 & el2) and el2 <= s2
    # left on fp32: the stem (3 -> 64, 64 -> 64), transition1's 256 -> 96, the coordinate head's J-wide blocks -- and the
    # layers of the classes that were measured not to win
    heads = sorted(t for t in s2 if t.startswith('head2.'))
    measured = sorted(_tag(name) for name, m in mods.items() if _is_s2(m) and _measured_fp32(m))
    assert left == sorted(['conv1', 'conv2', 'transition1.1.0'] + heads + measured), \
        'stride-2 3x3 layers left on fp32: %s' % (left,)
    eng = engine.HRNetEngine(net)
    with torch.no_grad():
        rec32, _, _ = eng._record(3, 3, 64, 64, None)
        net.precision = 'f16'
        rec16, _, _ = eng._record(3, 3, 64, 64, None)
        assert set(eng.last_f16_ops) == el1 and len(eng.last_f16_ops) == 18
        net.precision = 'f16s2'
        rec, _, _ = eng._record(3, 3, 64, 64, None)
    assert set(eng.last_f16_ops) == el1 | el2 and len(eng.last_f16_ops) == len(el1) + len(el2)
    assert all(kind != 'convh2' for kind, _ in rec32.ops + rec16.ops)
    a, b = _summary(rec32, monkeypatch), _summary(rec, monkeypatch)
    assert len(a) == len(b)
    for (ka, ta, ca, ra, la), (kb, tb, cb, rb, lb) in zip(a, b):
        assert (ta, ra, la) == (tb, rb, lb)
        if ta in el1:
            assert (ka, kb, cb) == ('conv', 'convh', None)
        elif ta in el2:
            assert (ka, kb, cb) == ('conv', 'convh2', None)     # not a tuner request any more
        else:
            assert (ka, ca) == (kb, cb)
    # 'f16s2' and 'f16' differ in the stride-2 layers only
    for (ka, ta, ca, ra, la), (kb, tb, cb, rb, lb) in zip(_summary(rec16, monkeypatch), b):
        assert (ta, ra, la, ca if ta not in el2 else None) == (tb, rb, lb, cb) and (ka == kb or ta in el2)
    # the emulation rounds exactly these layers, and the committed bounds are this model's
    _, hit, hit_s2 = case.cpu_emulated(net, case.crops('forward'))
    assert (hit, hit_s2) == (len(el1) + len(el2), len(el2))
    with open(case.BOUNDS_PATH) as f:
        bounds = json.load(f)
    assert bounds['coordinates']['forward']['f16_convs'] == hit
    assert bounds['coordinates']['forward']['f16s2_convs'] == len(el2) == len(s2) - 3 - len(heads) - len(measured) > 0


def test_f16_emulation_without_the_keyword_is_what_it_was():
    import f16_mode_case
    net = case.model('coordinates')
    _, hit = f16_mode_case.cpu_emulated(net, case.crops('forward'))
    assert hit == 18
    with torch.no_grad(), engine.f16_emulation(net) as em:
        net(case.crops('forward'))
    assert len(em.hit) == 18 and all(m.stride == (1, 1) for m in em.hit)
    with torch.no_grad(), engine.f16_emulation(net, precision='f16') as em16:
        net(case.crops('forward'))
    assert em16.hit == em.hit
    with pytest.raises(ValueError):
        engine.f16_emulation(net, precision='f32')


def test_w48_every_3x3_s2_layer_behind_transition1_is_lowered(monkeypatch):
    assert set(engine.F16S2_FP32_CLASSES) <= {(48, 48)}       # (the measured exceptions, class by class: DESIGN 3.16b)
    net = hrnet.get_pose_net(configs.w48_config(), is_train=False).eval()
    eng = engine.HRNetEngine(net)
    with torch.no_grad():
        net.precision = 'f16'
        rec16, _, _ = eng._record(2, 3, 256, 256, None)
        n16 = len(eng.last_f16_ops)
        net.precision = 'f16s2'
        rec, _, _ = eng._record(2, 3, 256, 256, None)
    assert n16 == 208
    behind = {name: m for name, m in net.named_modules() if _is_s2(m)
              and name.startswith(('transition2', 'transition3', 'stage2', 'stage3', 'stage4'))}
    want = {_tag(name) for name, m in behind.items() if not _measured_fp32(m)}
    measured = {_tag(name) for name, m in behind.items() if _measured_fp32(m)}
    lowered = [op['tag'] for kind, op in rec.ops if kind == 'convh2']
    assert len(want) > 0 and set(lowered) == want and len(lowered) == len(want)
    assert len(eng.last_f16_ops) == 208 + len(want)
    left = [op['tag'] for kind, op in rec.ops if kind == 'conv' and (op['kh'], op['stride']) == (3, 2)]
    # fp32: the stem, 256 -> 96, the layers of a class measured not to win, and (not backbone layers) the coordinate head's
    # J-wide blocks behind the heat-maps
    assert sorted(t for t in left if not t.startswith('head2.')) == sorted(['conv1', 'conv2', 'transition1.1.0'] + list(measured)), left
    # the 'f16' recording has them all as fp32 layers, as before
    left16 = [op['tag'] for kind, op in rec16.ops if kind == 'conv' and (op['kh'], op['stride']) == (3, 2)]
    assert set(left16) == want | set(left) and len(left16) == len(want) + len(left) and all(kind != 'convh2' for kind, _ in rec16.ops)


def test_the_switch_and_its_validation():
    assert engine.PRECISIONS == ('f32', 'f16', 'f16s2')
    cfg = case.config('heatmap')
    cfg['heatmapModel']['precision'] = 'f16s2'
    assert hrnet.get_pose_net(cfg, is_train=False).precision == 'f16s2'
    for bad in ('bf16', 'fp16', 'half'):
        cfg['heatmapModel']['precision'] = bad
        with pytest.raises(ValueError):
            hrnet.get_pose_net(cfg, is_train=False)
        net = case.model('heatmap')
        net.precision = bad
        with pytest.raises(ValueError, match='f16s2'), torch.no_grad():
            engine.HRNetEngine(net)._record(1, 3, 64, 64, None)
    from egonet_amd.model.egonet import EgoNet
    assert EgoNet(case.config('coordinates'), precision='f16s2').HC.precision == 'f16s2'
    assert EgoNet(case.config('coordinates'), precision='f16').HC.precision == 'f16'
    for bad in ('bf16', 'fp16', 'half'):
        with pytest.raises(ValueError):
            EgoNet(case.config('coordinates'), precision=bad)
    # the program key carries the value
    net = case.model('heatmap')
    eng = engine.HRNetEngine(net)
    net.precision = 'f16s2'
    assert eng.precision == 'f16s2'


def test_inference_tool_takes_the_value():
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'inference_kitti.py')
    with open(path) as f:
        src = f.read()
    assert "choices=['f32', 'f16', 'f16s2']" in src


def test_a_cpu_input_ignores_the_switch():
    """precision = 'f16s2' is read by the eval-mode HIP program only: a CPU input runs the fp32 torch graph."""
    net = case.model('heatmap')
    x = case.crops('forward')
    with torch.no_grad():
        want = net(x)
        net.precision = 'f16s2'
        got = net(x)
    assert torch.equal(got, want)
