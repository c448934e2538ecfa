"""The pixel-shuffle and angle-regression heads on the native training path, CPU side:

* the train-mode routing -- ``PoseHighResolutionNet._native_autograd_ok`` is True for both heads with default
  settings (their train-mode forward under autograd is the native tape's node, not the module graph) and False
  under each opt-out;
* the eval-mode programs are unchanged by the training branch of the walker: the op list the inference recorder
  gets for the two heads is stated here, op for op (the angle head's AvgPool2d + first Linear stay ONE 4x4 valid
  convolution with the derived filter).
"""
import pytest
import torch

from egonet_amd import configs, engine, synth
from egonet_amd.model.heatmapModel import hrnet


def _net(head):
    if head == 'pixshuf':
        cfg = configs.tiny_config('heatmap')
        cfg['heatmapModel']['pixel_shuffle'] = True
        cfg['heatmapModel']['heatmap_size'] = [32, 32]            # upsampling factor 2
    else:
        cfg = configs.tiny_config('angleregression', input_size=(256, 256))
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=3))
    return net


@pytest.mark.parametrize('head', ['pixshuf', 'angle'])
def test_native_autograd_routing_covers_both_heads(head, monkeypatch):
    net = _net(head).train()
    monkeypatch.delenv('EGONET_AMD_AUTOGRAD', raising=False)
    assert net._native_autograd_ok()
    # opt-outs, one at a time
    monkeypatch.setenv('EGONET_AMD_AUTOGRAD', '0')
    assert not net._native_autograd_ok()
    monkeypatch.delenv('EGONET_AMD_AUTOGRAD')
    h = net.conv1.register_forward_hook(lambda *a: None)
    net.__dict__.pop('_hook_dicts', None)
    assert not net._native_autograd_ok()
    h.remove()
    net.__dict__.pop('_hook_dicts', None)
    assert net._native_autograd_ok()
    net._is_replica = True
    assert not net._native_autograd_ok()
    del net._is_replica
    for p in net.parameters():
        p.requires_grad_(False)
    assert not net._native_autograd_ok()


# (kind, tag, weight shape, has bias, has BatchNorm, act, stride, pad) from the first head op on
_PIXSHUF_HEAD = [
    ('conv', 'final_layer', (5, 8, 1, 1), True, False, engine.ACT_NONE, 1, 0),
    ('conv', 'upsample_layer.0', (20, 5, 1, 1), True, True, engine.ACT_RELU, 1, 0),
    ('pixshuf', 'upsample_layer.3', 5, 2),
]
_ANGLE_HEAD = [('conv', 'head.0', (256, 8, 1, 1), True, False, engine.ACT_NONE, 1, 0)]
for _k in range(1, 5):
    _cin = 256
    _ANGLE_HEAD += [
        ('conv', 'head.%d.conv1' % _k, (256, _cin, 3, 3), False, True, engine.ACT_RELU, 2, 1),
        ('conv', 'head.%d.downsample' % _k, (256, _cin, 1, 1), False, True, engine.ACT_NONE, 2, 0),
        ('conv', 'head.%d.conv2' % _k, (256, 256, 3, 3), False, True, engine.ACT_RELU, 1, 1),
    ]
_ANGLE_HEAD += [
    ('conv', 'final_fc.0', (256, 256, 4, 4), True, True, engine.ACT_RELU, 1, 0),
    ('conv', 'final_fc.3', (2, 256, 1, 1), True, False, engine.ACT_NONE, 1, 0),
]


def _head_ops(net, first_tag, size):
    class Spy(engine._Recorder):
        def __init__(self):
            super().__init__()
            self.calls = []

        def conv(self, x, weight, bias=None, bn=None, act=engine.ACT_NONE, res=None, stride=1, pad=0, dst=None,
                 out_nchw=False, cout_cs=None, tag=''):
            self.calls.append(('conv', tag, tuple(weight.shape), bias is not None, bn is not None, act, stride, pad,
                               weight))
            return super().conv(x, weight, bias, bn, act, res, stride, pad, dst, out_nchw, cout_cs, tag)

        def pixel_shuffle(self, x, c, up, dst_ext, tag=''):
            self.calls.append(('pixshuf', tag, c, up))
            return super().pixel_shuffle(x, c, up, dst_ext, tag)

    r = Spy()
    net.eval()
    engine.HRNetEngine(net)._record(2, 3, size, size, None, r=r)
    tags = [c[1] for c in r.calls]
    return r, r.calls[tags.index(first_tag):]


def test_eval_programs_of_the_two_heads_are_unchanged():
    net = _net('pixshuf')
    r, ops = _head_ops(net, 'final_layer', 64)
    assert [o[:8] if o[0] == 'conv' else o for o in ops] == _PIXSHUF_HEAD
    kinds = [k for k, _ in r.ops if k not in ('fork', 'join')]
    assert len(kinds) == 56 and kinds[-3:] == ['conv', 'conv', 'pixshuf'], kinds
    assert not hasattr(r, 'avgpool')

    net = _net('angle')
    r, ops = _head_ops(net, 'head.0', 256)
    assert [o[:8] for o in ops] == _ANGLE_HEAD
    # the fused AvgPool2d(4) + Linear filter: W[o][c] / 16 on each of the 16 taps
    fc1 = net.final_fc[0]
    w1 = ops[-2][8]
    assert torch.equal(w1, (fc1.weight.detach() / 16.0).view(256, 256, 1, 1).expand(-1, -1, 4, 4).contiguous())
    assert ops[-1][8].shape == (2, 256, 1, 1) and ops[-1][8].data_ptr() == net.final_fc[3].weight.data_ptr()
    kinds = [k for k, _ in r.ops if k not in ('fork', 'join')]
    assert len(kinds) == 68 and set(kinds) == {'to_nhwc', 'conv', 'pwpair', 'fuse'}, kinds      # no pool op

