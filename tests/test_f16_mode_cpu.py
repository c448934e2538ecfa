"""The opt-in f16-operand inference mode (PoseHighResolutionNet.precision = 'f16', csrc/conv_h.hip) without a GPU: the
filter packing, the host-only predicate, what the recorder lowers -- and that the default recording is untouched.  The
layers in the reference: libs/model/heatmapModel/hrnet.py:63-92 (3x3 convolutions of the BasicBlocks, fp32 torch calls)."""
import json

import pytest
import torch
import torch.nn as nn

import f16_mode_case as case
from egonet_amd import _lib, configs, engine, tuner
from egonet_amd.model.heatmapModel import hrnet
from egonet_amd.model.heatmapModel.hrnet import PoseHighResolutionNet

RELU, NONE = engine.ACT_RELU, engine.ACT_NONE


@pytest.mark.parametrize('cout,cin', [(48, 48), (96, 48), (384, 384)])
def test_filter_pack_round_trip(cout, cin):
    g = torch.Generator().manual_seed(cout + cin)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    w[0, 0, 0, 0], w[1, 2, 1, 1] = 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11       # ties: to even (1.0 / 1 + 2^-9)
    p = engine.pack_conv_weight_f16(w)
    assert p.dtype == torch.float32 and p.numel() * 4 == _lib.lib().egn_conv3x3_h_wpack_bytes(cin, cout)
    back = engine.unpack_conv_weight_f16(p, cout, cin)
    assert back.dtype == torch.float16 and torch.equal(back, w.half())
    assert float(back[0, 0, 0, 0]) == 1.0 and float(back[1, 2, 1, 1]) == 1.0 + 2.0 ** -9
    # the padding past k = 432 of every chunk is zero
    lanes = p.view(torch.float16).reshape(cout // 16, cin // 48, 14, 4, 16, 8)         # ct chunk step g li j
    assert (lanes[:, :, 13, 2:] == 0).all()


def test_predicate_answers():
    L = _lib.lib()
    ok = [(64, 64, 64, 48, 48, 48, 48, 1, RELU), (16, 32, 32, 96, 96, 96, 96, 0, RELU), (64, 16, 16, 192, 192, 192, 192, 1, RELU),
          (1, 8, 8, 384, 384, 384, 384, 0, NONE), (5, 2, 2, 384, 384, 384, 384, 1, RELU), (2, 6, 5, 48, 48, 96, 96, 0, NONE),
          (3, 12, 20, 96, 96, 96, 96, 1, RELU)]
    no = [(64, 64, 64, 40, 40, 48, 48, 0, RELU),                    # Cin = 40
          (64, 64, 64, 48, 48, 48, 48, 0, engine.ACT_SIGMOID),      # a sigmoid epilogue
          (64, 64, 64, 48, 48, 48, 48, 0, engine.ACT_LEAKY),
          (64, 64, 64, 48, 48, 48, 48, 1, RELU | engine.ACT_RES_AFTER),
          (64, 64, 64, 48, 52, 48, 48, 0, RELU),                    # padded channel strides
          (64, 64, 64, 48, 48, 48, 52, 0, RELU),
          (64, 64, 64, 256, 256, 48, 48, 0, RELU),                  # transition1: 256 -> 48
          (64, 64, 64, 64, 64, 64, 64, 0, RELU),                    # layer1 / the Pedestrian widths
          (64, 64, 48, 32, 32, 32, 32, 0, RELU), (64, 32, 24, 128, 128, 128, 128, 0, RELU),
          (0, 8, 8, 48, 48, 48, 48, 0, RELU), (1, 1, 8, 48, 48, 48, 48, 0, RELU), (1, 8, 1, 48, 48, 48, 48, 0, RELU),
          (4096, 64, 64, 48, 48, 48, 48, 0, RELU)]                  # 3 GiB of activations: 32-bit offsets
    for a in ok:
        assert L.egn_conv3x3_h_applies(*a) == 1, a
    for a in no:
        assert L.egn_conv3x3_h_applies(*a) == 0, a
    assert L.egn_conv3x3_h_wpack_bytes(40, 48) == 0 and L.egn_conv3x3_h_wpack_bytes(48, 48) == 3 * 14 * 1024


def test_f16_eligible_never_offers_other_layers():
    conv = nn.Conv2d(48, 48, 3, 1, 1, bias=False)
    assert engine.f16_eligible(conv, 3, 16, 16)
    assert not engine.f16_eligible(nn.Conv2d(48, 96, 3, 2, 1, bias=False), 3, 16, 16)        # stride 2: never offered
    assert not engine.f16_eligible(nn.Conv2d(48, 48, 3, 1, 1, bias=True), 3, 16, 16)
    assert not engine.f16_eligible(nn.Conv2d(48, 48, 1, 1, 0, bias=False), 3, 16, 16)
    assert not engine.f16_eligible(nn.Conv2d(48, 48, 3, 1, 1, bias=False, groups=2), 3, 16, 16)
    assert not engine.f16_eligible(nn.Conv2d(48, 48, 3, 1, 2, bias=False, dilation=2), 3, 16, 16)
    assert not engine.f16_eligible(nn.Conv2d(40, 48, 3, 1, 1, bias=False), 3, 16, 16)
    assert not engine.f16_eligible(nn.BatchNorm2d(48), 3, 16, 16)


def _summary(rec, monkeypatch):
    """(kind, tag, tile configuration the shipped table answers) per op."""
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    out = []
    for kind, op in rec.ops:
        cfg = tuner.choose(None, engine.Program._conv_key(op), engine.Program._conv_kinds(op)) if kind == 'conv' else None
        out.append((kind, op.get('tag', ''), cfg, op.get('region'), op.get('lane')))
    return out


@pytest.mark.parametrize('n', [1, 3])
def test_default_recording_is_unchanged_op_for_op(n, monkeypatch):
    assert _lib.lib().egn_conv_num_configs() == 93          # the family is beside the table, not in it
    assert PoseHighResolutionNet.precision == 'f32'
    net = hrnet.get_pose_net(configs.w48_config(), is_train=False).eval()
    assert 'precision' not in net.__dict__
    eng = engine.HRNetEngine(net)
    with torch.no_grad():
        rec_default, slots_d, shapes_d = eng._record(n, 3, 256, 256, None)
        assert eng.last_f16_ops == []
        net.precision = 'f32'
        rec_f32, slots_e, shapes_e = eng._record(n, 3, 256, 256, None)
    a, b = _summary(rec_default, monkeypatch), _summary(rec_f32, monkeypatch)
    assert a == b and (slots_d, shapes_d) == (slots_e, shapes_e)
    assert all(kind != 'convh' for kind, _ in rec_default.ops) and eng.last_f16_ops == []
    assert rec_default.blob_off == rec_f32.blob_off and rec_default.plan_arena() == rec_f32.plan_arena()
    # no tile configuration a caller can be handed is the new family's: every id has a table kind
    for kind, tag, cfg, _, _ in a:
        assert cfg is None or 0 <= cfg <= 93


def test_f16_recording_lowers_exactly_the_eligible_layers(monkeypatch):
    """On the GPU test's model (W48 widths, 64 x 64 input): the lowered tags are the modules ``f16_eligible`` names with
    the input shapes the torch forward shows them; everything else is recorded exactly as in 'f32'."""
    net = case.model('coordinates')
    seen = {}
    hooks = [m.register_forward_pre_hook(lambda mod, args, name=name: seen.__setitem__(name, tuple(args[0].shape)))
             for name, m in net.named_modules() if isinstance(m, nn.Conv2d)]
    with torch.no_grad():
        net(case.crops('forward'))
    for h in hooks:
        h.remove()
    mods = dict(net.named_modules())
    eligible = {name for name, (n, c, h, w) in seen.items() if engine.f16_eligible(mods[name], n, h, w)}
    assert len(eligible) == 18
    eng = engine.HRNetEngine(net)
    with torch.no_grad():
        rec32, _, _ = eng._record(3, 3, 64, 64, None)
        net.precision = 'f16'
        rec16, _, _ = eng._record(3, 3, 64, 64, None)
    assert set(eng.last_f16_ops) == eligible and len(eng.last_f16_ops) == len(eligible)
    a, b = _summary(rec32, monkeypatch), _summary(rec16, monkeypatch)
    assert len(a) == len(b)
    for (ka, ta, ca, ra, la), (kb, tb, cb, rb, lb) in zip(a, b):
        assert (ta, ra, la) == (tb, rb, lb)
        if ta in eligible:
            assert (ka, kb, cb) == ('conv', 'convh', None)      # not a tuner request any more
        else:
            assert (ka, ca) == (kb, cb)
    # the emulation rounds exactly these layers
    _, hit = case.cpu_emulated(net, case.crops('forward'))
    assert hit == len(eligible)
    # the committed bounds are what the generator writes for this model (same torch build: to the bit)
    with open(case.BOUNDS_PATH) as f:
        bounds = json.load(f)
    assert bounds['coordinates']['forward']['f16_convs'] == len(eligible)


def test_w48_every_3x3_s1_layer_of_stages_2_to_4_is_lowered(monkeypatch):
    monkeypatch.setenv('EGONET_AMD_PAIR', 'force')         # even where pairs are forced: a lowered layer is never half of one
    net = hrnet.get_pose_net(configs.w48_config(), is_train=False).eval()
    net.precision = 'f16'
    eng = engine.HRNetEngine(net)
    with torch.no_grad():
        rec, _, _ = eng._record(2, 3, 256, 256, None)
    want = {name for name, m in net.named_modules() if isinstance(m, nn.Conv2d) and name.startswith(('stage2', 'stage3', 'stage4'))
            and m.kernel_size == (3, 3) and m.stride == (1, 1)}
    assert len(want) == 208 and want <= set(eng.last_f16_ops)
    assert all(kind != 'convpair' for kind, _ in rec.ops)
    left = [op['tag'] for kind, op in rec.ops if kind == 'conv' and (op['kh'], op['stride']) == (3, 1)]
    assert all(t.startswith(('layer1', 'transition1', 'head2')) for t in left), left       # 64 / 256 / J-wide layers: fp32


def test_the_switch_and_its_validation():
    cfg = case.config('heatmap')
    cfg['heatmapModel']['precision'] = 'f16'
    assert hrnet.get_pose_net(cfg, is_train=False).precision == 'f16'
    cfg['heatmapModel']['precision'] = 'f32'
    assert hrnet.get_pose_net(cfg, is_train=False).precision == 'f32'
    cfg['heatmapModel']['precision'] = 'bf16'
    with pytest.raises(ValueError):
        hrnet.get_pose_net(cfg, is_train=False)
    net = case.model('heatmap')
    net.precision = 'fp16'
    with pytest.raises(ValueError), torch.no_grad():
        engine.HRNetEngine(net)._record(1, 3, 64, 64, None)
    from egonet_amd.model.egonet import EgoNet
    assert EgoNet(case.config('coordinates')).HC.precision == 'f32'
    assert EgoNet(case.config('coordinates'), precision='f16').HC.precision == 'f16'
    with pytest.raises(ValueError):
        EgoNet(case.config('coordinates'), precision='half')


def test_a_cpu_input_ignores_the_switch():
    """precision = 'f16' is read by the eval-mode HIP program only: a CPU input runs the fp32 torch graph."""
    net = case.model('heatmap')
    x = case.crops('forward')
    with torch.no_grad():
        want = net(x)
        net.precision = 'f16'
        got = net(x)
    assert torch.equal(got, want)
