"""precision = 'f16x' without a GPU: what 'f16s2' lowers plus the 3x3 / pad 1 layers of the 32-MULTIPLE widths on the
f16-operand kernel (csrc/conv_h.hip with CK = 32).  The filter pack, the host-only predicate, ``engine.f16x_eligible``,
what the recorder lowers on HRNet-W32 (the Pedestrian model) and on HRNet-W48, the switch -- and that 'f32', 'f16' and
'f16s2' record what they recorded.  The layers in the reference: libs/model/heatmapModel/hrnet.py (fp32 torch calls);
the Pedestrian model is its configs/KITTI_train_IGRs_Ped.yml."""
import json
import os
import sys

import pytest
import torch
import torch.nn as nn

import f16x_mode_case as case
from egonet_amd import _lib, configs, engine, tuner
from egonet_amd.model.heatmapModel import hrnet

RELU, NONE = engine.ACT_RELU, engine.ACT_NONE
CINS = (32, 64, 128, 256)
W48_EXTRA = {'layer1.0.conv2', 'layer1.1.conv2', 'layer1.2.conv2', 'layer1.3.conv2', 'conv2', 'transition1.0',
             'transition1.1.0'}


@pytest.mark.parametrize('cout,cin', [(32, 32), (64, 32), (256, 256), (48, 256)])
def test_filter_pack_round_trip(cout, cin):
    g = torch.Generator().manual_seed(cout + cin)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    w[0, 0, 0, 0], w[1, 2, 1, 1] = 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11       # ties: to even (1.0 / 1 + 2^-9)
    p = engine.pack_conv_weight_f16x(w)
    assert p.dtype == torch.float32 and p.numel() * 4 == _lib.lib().egn_conv3x3_hx_wpack_bytes(cin, cout) == cout * cin * 18
    back = engine.unpack_conv_weight_f16x(p, cout, cin)
    assert back.dtype == torch.float16 and torch.equal(back, w.half())
    assert float(back[0, 0, 0, 0]) == 1.0 and float(back[1, 2, 1, 1]) == 1.0 + 2.0 ** -9
    # the layout: [Cout/16][Cin/32][tap][lane = 16 g + li][j] holds W[16 ct + li][32 chunk + 8 g + j][tap]
    lanes = p.view(torch.float16).reshape(cout // 16, cin // 32, 9, 4, 16, 8)          # ct chunk tap g li j
    for ct, ch, tap, gg, li, j in ((0, 0, 0, 0, 0, 0), (1, 0, 5, 2, 3, 4), (cout // 16 - 1, cin // 32 - 1, 8, 3, 15, 7)):
        assert lanes[ct, ch, tap, gg, li, j] == w.half()[16 * ct + li, 32 * ch + 8 * gg + j, tap // 3, tap % 3]


def test_wpack_bytes():
    L = _lib.lib()
    assert L.egn_conv3x3_hx_wpack_bytes(32, 32) == 18432
    assert L.egn_conv3x3_hx_wpack_bytes(256, 48) == 256 * 48 * 18 and L.egn_conv3x3_hx_wpack_bytes(256, 96) == 256 * 96 * 18
    for cin, cout in ((48, 48), (40, 32), (32, 192), (96, 96), (32, 40), (0, 32)):
        assert L.egn_conv3x3_hx_wpack_bytes(cin, cout) == 0, (cin, cout)
    assert L.egn_conv_num_configs() == 93          # the family is beside the table, not in it


def test_predicate_answers():
    L = _lib.lib()
    # the W32 classes at the Pedestrian map sizes (H x W), both strides, with and without a residual at stride 1
    for c, (h, w) in zip(CINS, ((64, 48), (32, 24), (16, 12), (8, 6))):
        for n in (1, 16, 64):
            for act in (RELU, NONE):
                assert L.egn_conv3x3_hx_applies(n, h, w, c, c, c, c, 1, act, 1) == 1, (n, h, w, c)
                assert L.egn_conv3x3_hx_applies(n, h, w, c, c, c, c, 0, act, 1) == 1, (n, h, w, c)
                for cout in CINS:          # the fuse and transition units
                    assert L.egn_conv3x3_hx_applies(n, h, w, c, c, cout, cout, 0, act, 2) == 1, (n, h, w, c, cout)
                    assert L.egn_conv3x3_hx_applies(n, h, w, c, c, cout, cout, 0, act, 1) == 1, (n, h, w, c, cout)
    yes = [(64, 64, 64, 64, 64, 64, 64, 0, RELU, 1), (64, 128, 128, 64, 64, 64, 64, 0, RELU, 2),      # layer1, the stem's conv2
           (16, 64, 48, 64, 64, 64, 64, 0, RELU, 1), (16, 128, 96, 64, 64, 64, 64, 0, RELU, 2),
           (64, 64, 64, 256, 256, 48, 48, 0, RELU, 1), (64, 64, 64, 256, 256, 96, 96, 0, RELU, 2),    # transition1 of W48
           (5, 2, 2, 128, 128, 128, 128, 1, RELU, 1), (3, 9, 7, 32, 32, 32, 32, 0, NONE, 2)]
    for a in yes:
        assert L.egn_conv3x3_hx_applies(*a) == 1, a
    no = [(16, 64, 48, 40, 40, 32, 32, 0, RELU, 1),                  # Cin = 40
          (16, 64, 48, 48, 48, 48, 48, 0, RELU, 1),                  # Cin = 48: the old family's
          (16, 64, 48, 48, 48, 96, 96, 0, RELU, 2),
          (16, 64, 48, 96, 96, 32, 32, 0, RELU, 1),
          (16, 64, 48, 32, 32, 192, 192, 0, RELU, 1),                # Cout = 192
          (16, 64, 48, 32, 32, 40, 40, 0, RELU, 1),
          (16, 64, 48, 32, 36, 32, 32, 0, RELU, 1),                  # padded channel strides
          (16, 64, 48, 32, 32, 32, 36, 0, RELU, 2),
          (16, 64, 48, 32, 32, 32, 32, 0, engine.ACT_SIGMOID, 1),
          (16, 64, 48, 32, 32, 32, 32, 0, engine.ACT_LEAKY, 2),
          (16, 64, 48, 32, 32, 32, 32, 1, RELU | engine.ACT_RES_AFTER, 1),
          (16, 64, 48, 32, 32, 32, 32, 1, RELU, 2),                  # a residual at stride 2
          (16, 64, 48, 32, 32, 32, 32, 2, RELU, 1),
          (16, 64, 48, 32, 32, 32, 32, 0, RELU, 3), (16, 64, 48, 32, 32, 32, 32, 0, RELU, 0),
          (0, 8, 8, 32, 32, 32, 32, 0, RELU, 1),
          (1, 1, 8, 32, 32, 32, 32, 0, RELU, 1), (1, 8, 1, 32, 32, 32, 32, 0, RELU, 2),           # H = 1, W = 1
          (6144, 64, 64, 32, 32, 32, 32, 0, RELU, 1),                # 3 GiB of activations: 32-bit offsets
          (6144, 64, 64, 32, 32, 32, 32, 0, RELU, 2),                # (3 GiB in)
          (3072, 64, 64, 32, 32, 256, 256, 0, RELU, 1)]              # (1.5 GiB in, 12 GiB out)
    for a in no:
        assert L.egn_conv3x3_hx_applies(*a) == 0, a
    # the two older predicates answer as they did
    assert L.egn_conv3x3_h_applies(16, 64, 48, 32, 32, 32, 32, 0, RELU) == 0
    assert L.egn_conv3x3_h_applies(64, 64, 64, 256, 256, 48, 48, 0, RELU) == 0
    assert L.egn_conv3x3s2_h_applies(64, 128, 128, 64, 64, 64, 64, RELU) == 0
    assert L.egn_conv3x3s2_h_applies(64, 64, 64, 256, 256, 96, 96, RELU) == 0
    assert L.egn_conv3x3_h_applies(64, 64, 64, 48, 48, 48, 48, 1, RELU) == 1
    assert L.egn_conv3x3s2_h_applies(64, 64, 64, 48, 48, 96, 96, RELU) == 1


def test_f16x_eligible_never_offers_other_layers(monkeypatch):
    assert all(len(c) == 3 for c in engine.F16X_FP32_CLASSES)
    monkeypatch.setattr(engine, 'F16X_FP32_CLASSES', ())
    conv = nn.Conv2d(32, 64, 3, 2, 1, bias=False)
    assert engine.f16x_eligible(conv, 3, 16, 12)
    assert engine.f16x_eligible(nn.Conv2d(64, 64, 3, 1, 1, bias=False), 3, 16, 12)
    assert engine.f16x_eligible(nn.Conv2d(256, 48, 3, 1, 1, bias=False), 3, 16, 12)
    assert not engine.f16_eligible(conv, 3, 16, 12) and not engine.f16s2_eligible(conv, 3, 16, 12)
    assert not engine.f16x_eligible(nn.Conv2d(48, 48, 3, 1, 1, bias=False), 3, 16, 12)      # 'f16' has it
    assert not engine.f16x_eligible(nn.Conv2d(48, 96, 3, 2, 1, bias=False), 3, 16, 12)      # 'f16s2' has it
    assert not engine.f16x_eligible(nn.Conv2d(32, 32, 1, 1, 0, bias=False), 3, 16, 12)
    assert not engine.f16x_eligible(nn.Conv2d(32, 32, 3, 1, 0, bias=False), 3, 16, 12)
    assert not engine.f16x_eligible(nn.Conv2d(32, 32, 3, 3, 1, bias=False), 3, 16, 12)
    assert not engine.f16x_eligible(nn.Conv2d(32, 32, 3, (1, 2), 1, bias=False), 3, 16, 12)
    assert not engine.f16x_eligible(nn.Conv2d(32, 64, 3, 2, 1, bias=True), 3, 16, 12)
    assert not engine.f16x_eligible(nn.Conv2d(32, 64, 3, 2, 1, bias=False, groups=2), 3, 16, 12)
    assert not engine.f16x_eligible(nn.Conv2d(32, 64, 3, 1, 2, bias=False, dilation=2), 3, 16, 12)
    assert not engine.f16x_eligible(nn.Conv2d(32, 64, 3, 1, 1, bias=False, padding_mode='reflect'), 3, 16, 12)
    assert not engine.f16x_eligible(nn.Conv2d(3, 64, 3, 2, 1, bias=False), 3, 16, 12)
    assert not engine.f16x_eligible(nn.Conv2d(32, 192, 3, 1, 1, bias=False), 3, 16, 12)
    assert not engine.f16x_eligible(nn.BatchNorm2d(32), 3, 16, 12)
    # a class measured not to win is left on fp32, by the rule and by the recorder alike; the class carries the stride
    x = engine.Buf(3, 16, 12, 32)
    monkeypatch.setattr(engine, 'F16X_FP32_CLASSES', ((32, 64, 2),))
    assert not engine.f16x_eligible(conv, 3, 16, 12)
    assert engine.f16x_eligible(nn.Conv2d(32, 64, 3, 1, 1, bias=False), 3, 16, 12)
    assert not engine._Recorder.takes_f16x(x, conv.weight, None, RELU, None, 2, 1)
    assert engine._Recorder.takes_f16x(x, conv.weight, None, RELU, None, 1, 1)
    monkeypatch.setattr(engine, 'F16X_FP32_CLASSES', ())
    assert engine._Recorder.takes_f16x(x, conv.weight, None, RELU, None, 2, 1)
    # what the recorder's question refuses beside the rule's
    res = engine.Buf(3, 16, 12, 64)
    assert engine._Recorder.takes_f16x(x, conv.weight, None, RELU, res, 1, 1)
    assert not engine._Recorder.takes_f16x(x, conv.weight, None, RELU, res, 2, 1)                     # a residual at stride 2
    assert not engine._Recorder.takes_f16x(x, conv.weight, torch.zeros(64), RELU, None, 2, 1)          # a bias
    assert not engine._Recorder.takes_f16x(x, conv.weight, None, RELU, None, 2, 1, out_nchw=True)
    assert not engine._Recorder.takes_f16x(x, conv.weight, None, RELU, None, 2, 1, cout_cs=100)
    assert not engine._Recorder.takes_f16x(x, conv.weight, None, RELU, None, 2, 1, dst_given=True)
    assert not engine._Recorder.takes_f16x(x, conv.weight, None, engine.ACT_SIGMOID, None, 2, 1)
    assert not engine._Recorder.takes_f16x(x, conv.weight, None, RELU, None, 2, 0)


def _summary(rec, monkeypatch):
    """(kind, tag, tile configuration the shipped table answers, region, lane) per op."""
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    out = []
    for kind, op in rec.ops:
        cfg = tuner.choose(None, engine.Program._conv_key(op), engine.Program._conv_kinds(op)) if kind == 'conv' else None
        out.append((kind, op.get('tag', ''), cfg, op.get('region'), op.get('lane')))
    return out


def _storage(rec, nslots, shapes):
    """Slots, buffers (the arena's tenants) and the weights blob of a recording."""
    return (nslots, repr(sorted(shapes.items())), rec.blob_off, [t.numel() for t in rec.blobs],
            [(b.n, b.h, b.w, b.c, b.cs, b.nbytes, b.first, b.last) for b in rec.bufs])


def _tag(name):
    """Module name of a convolution -> the tag the recorder gives its layer: the transition and fuse units are recorded
    under the name of their Sequential(conv, bn[, relu])."""
    return name[:-2] if name.startswith(('transition', 'stage')) and '.branches.' not in name and name.endswith('.0') \
        else name


def _is33(m):
    return isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3)


def _measured_fp32(m):
    return (m.in_channels, m.out_channels, m.stride[0]) in engine.F16X_FP32_CLASSES


def test_pedestrian_model_old_modes_are_untouched_and_f16x_lowers_the_eligible_layers(monkeypatch):
    """configs.ped_config() (HRNet-W32, 192 x 256): 'f32', 'f16' and 'f16s2' record the same program, 'f16x' lowers exactly
    the modules ``f16x_eligible`` names at the shapes a torch forward shows, and records the rest as 'f32' does."""
    net = hrnet.get_pose_net(configs.ped_config(), is_train=False).eval()
    x = torch.zeros(2, 3, 256, 192)
    seen = case.seen_conv_inputs(net, x)
    mods = dict(net.named_modules())
    el = {_tag(name) for name, (n, c, h, w) in seen.items() if engine.f16x_eligible(mods[name], n, h, w)}
    assert not any(engine.f16_eligible(mods[name], n, h, w) or engine.f16s2_eligible(mods[name], n, h, w)
                   for name, (n, c, h, w) in seen.items())
    eng = engine.HRNetEngine(net)
    recs = {}
    with torch.no_grad():
        for prec in ('f32', 'f16', 'f16s2', 'f16x'):
            net.precision = prec
            rec, nslots, shapes = eng._record(2, 3, 256, 192, None)
            recs[prec] = (_summary(rec, monkeypatch), _storage(rec, nslots, shapes), list(eng.last_f16_ops), rec)
    for prec in ('f16', 'f16s2'):
        assert recs[prec][0] == recs['f32'][0] and recs[prec][1] == recs['f32'][1] and recs[prec][2] == []
    assert recs['f32'][2] == []
    a, b, tags, rec = recs['f32'][0], recs['f16x'][0], recs['f16x'][2], recs['f16x'][3]
    assert set(tags) == el and len(tags) == len(el) > 200
    assert len(a) == len(b)
    for (ka, ta, ca, ra, la), (kb, tb, cb, rb, lb) in zip(a, b):
        assert (ta, ra, la) == (tb, rb, lb)
        if ta in el:
            assert (ka, kb, cb) == ('conv', 'convhx', None)          # not a tuner request any more
        else:
            assert (ka, ca) == (kb, cb)
    assert all(kind not in ('convh', 'convh2', 'convpair') for kind, _ in rec.ops)
    # the stage, transition, layer1 and conv2 3x3 layers are lowered: what is left is conv1, the head's, a measured class
    left = [op for kind, op in rec.ops if kind == 'conv' and op['kh'] == 3]
    for op in left:
        assert op['tag'] == 'conv1' or op['tag'].startswith('head2.') or \
            (op['cin'], op['cout'], op['stride']) in engine.F16X_FP32_CLASSES, op['tag']
    for t in ('conv2', 'layer1.0.conv2', 'layer1.3.conv2', 'transition1.0', 'transition1.1.0', 'transition3.3.0',
              'stage2.0.branches.0.0.conv1', 'stage4.2.branches.3.3.conv2'):
        m = mods[t + '.0' if t.startswith('transition') else t]
        assert (t in tags) == (not _measured_fp32(m)), t
    # the lowered ops carry the layer's stride and residual
    for kind, op in rec.ops:
        if kind == 'convhx':
            assert op['stride'] in (1, 2) and (op['res'] is None or op['stride'] == 1)
    assert any(op['res'] is not None for kind, op in rec.ops if kind == 'convhx')


def test_w48_f16x_is_f16s2_plus_the_seven_layers(monkeypatch):
    net = hrnet.get_pose_net(configs.w48_config(), is_train=False).eval()
    mods = dict(net.named_modules())
    eng = engine.HRNetEngine(net)
    with torch.no_grad():
        net.precision = 'f16'
        rec16, ns16, sh16 = eng._record(2, 3, 256, 256, None)
        tags16 = list(eng.last_f16_ops)
        net.precision = 'f16s2'
        rec2, ns2, sh2 = eng._record(2, 3, 256, 256, None)
        tags2 = list(eng.last_f16_ops)
        net.precision = 'f16x'
        recx, _, _ = eng._record(2, 3, 256, 256, None)
        tagsx = list(eng.last_f16_ops)
        # the two old modes after 'f16x' was visited, op for op what they were before
        net.precision = 'f16'
        rec16b, ns16b, sh16b = eng._record(2, 3, 256, 256, None)
        net.precision = 'f16s2'
        rec2b, ns2b, sh2b = eng._record(2, 3, 256, 256, None)
    extra = {t for t in W48_EXTRA
             if not _measured_fp32(mods[t + '.0' if t.startswith('transition') else t])}
    assert set(tagsx) == set(tags2) | extra and len(tagsx) == len(tags2) + len(extra) and not (set(tags2) & W48_EXTRA)
    assert len(tags16) == 208
    assert [op['tag'] for kind, op in recx.ops if kind == 'convhx'] == [t for t in tagsx if t in extra]
    assert all(kind != 'convhx' for kind, _ in rec16.ops + rec2.ops + rec16b.ops + rec2b.ops)
    assert _summary(rec16, monkeypatch) == _summary(rec16b, monkeypatch) and _storage(rec16, ns16, sh16) == _storage(rec16b, ns16b, sh16b)
    assert _summary(rec2, monkeypatch) == _summary(rec2b, monkeypatch) and _storage(rec2, ns2, sh2) == _storage(rec2b, ns2b, sh2b)
    # 'f16x' and 'f16s2' differ in the seven layers only
    a, b = _summary(rec2, monkeypatch), _summary(recx, monkeypatch)
    assert len(a) == len(b)
    for (ka, ta, ca, ra, la), (kb, tb, cb, rb, lb) in zip(a, b):
        assert (ta, ra, la) == (tb, rb, lb)
        if ta in extra:
            assert (ka, kb, cb) == ('conv', 'convhx', None)
        else:
            assert (ka, ca) == (kb, cb)


def test_case_model_recording_emulation_and_bounds(monkeypatch):
    """On the GPU test's model: the lowered tags are the eligible modules, the emulation rounds exactly those layers, and
    the committed bounds file is what its generator writes."""
    net = case.model('coordinates')
    x = case.crops('forward')
    seen = case.seen_conv_inputs(net, x)
    mods = dict(net.named_modules())
    el = {_tag(name) for name, (n, c, h, w) in seen.items() if engine.f16x_eligible(mods[name], n, h, w)}
    eng = engine.HRNetEngine(net)
    with torch.no_grad():
        net.precision = 'f16x'
        rec, _, _ = eng._record(x.shape[0], 3, case.HEIGHT, case.WIDTH, None)
    assert set(eng.last_f16_ops) == el and len(eng.last_f16_ops) == len(el)
    left = [op['tag'] for kind, op in rec.ops if kind == 'conv' and op['kh'] == 3]
    assert all(t == 'conv1' or t.startswith('head2.') or _measured_fp32(mods[t]) for t in left), left
    with torch.no_grad(), engine.f16_emulation(net, precision='f16x') as em:
        net(x)
    names = {m: name for name, m in mods.items()}
    assert {_tag(names[m]) for m in em.hit} == el and len(em.hit) == len(el)
    # the other two emulations hit nothing on this model, and 'f32' is no emulation
    for prec in ('f16', 'f16s2'):
        with torch.no_grad(), engine.f16_emulation(net, precision=prec) as em0:
            net(x)
        assert em0.hit == []
    with pytest.raises(ValueError, match='f16x'):
        engine.f16_emulation(net, precision='f32')
    with open(case.BOUNDS_PATH) as f:
        bounds = json.load(f)
    assert bounds['coordinates']['forward']['f16_convs'] == len(el)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    try:
        import make_f16x_bounds
    finally:
        sys.path.pop(0)
    fresh = make_f16x_bounds.compute()
    if fresh['_torch'] == bounds['_torch']:
        assert fresh == bounds
    else:           # another torch build may sum in another order: the counts and the file's shape must still agree
        assert {h: {w: (v['f16_convs'], v['f16x_convs'], sorted(v)) for w, v in fresh[h].items()} for h in case.HEADS} == \
            {h: {w: (v['f16_convs'], v['f16x_convs'], sorted(v)) for w, v in bounds[h].items()} for h in case.HEADS}


def test_the_switch_and_its_validation():
    assert engine.ALL_PRECISIONS == ('f32', 'f16', 'f16s2', 'f16x') and engine.PRECISIONS[-1] == 'f16s2'
    cfg = case.config('heatmap')
    cfg['heatmapModel']['precision'] = 'f16x'
    assert hrnet.get_pose_net(cfg, is_train=False).precision == 'f16x'
    for bad in ('bf16', 'f16s1', 'f16X'):
        cfg['heatmapModel']['precision'] = bad
        with pytest.raises(ValueError, match="'f32', 'f16', 'f16s2' or 'f16x'"):
            hrnet.get_pose_net(cfg, is_train=False)
        net = case.model('heatmap')
        net.precision = bad
        with pytest.raises(ValueError, match="'f32', 'f16', 'f16s2' or 'f16x'"), torch.no_grad():
            engine.HRNetEngine(net)._record(1, 3, case.HEIGHT, case.WIDTH, None)
    from egonet_amd.model.egonet import EgoNet
    assert EgoNet(case.config('coordinates'), precision='f16x').HC.precision == 'f16x'
    for bad in ('bf16', 'f16s1', 'f16X'):
        with pytest.raises(ValueError, match="'f32', 'f16', 'f16s2' or 'f16x'"):
            EgoNet(case.config('coordinates'), precision=bad)
    # the program key carries the value
    net = case.model('heatmap')
    eng = engine.HRNetEngine(net)
    net.precision = 'f16x'
    assert eng.precision == 'f16x'


def test_inference_tool_takes_the_value():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'inference_kitti.py')
    with open(path) as f:
        src = f.read()
    assert "choices=['f32', 'f16', 'f16s2'] + ['f16x']" in src and '--precision f32|f16|f16s2|f16x' in src


def test_a_cpu_input_ignores_the_switch():
    """precision = 'f16x' is read by the eval-mode HIP program only: a CPU input runs the fp32 torch graph."""
    net = case.model('heatmap')
    x = case.crops('forward')
    with torch.no_grad():
        want = net(x)
        net.precision = 'f16x'
        got = net(x)
    assert torch.equal(got, want)
