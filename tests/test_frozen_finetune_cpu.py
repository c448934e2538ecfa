"""Frozen-layer fine-tuning, the parts that need no GPU: ``extra.freeze_bn`` keeps the BatchNorm layers of the frozen
prefixes in eval mode through ``model.train()``, and the launches the pruned backward is expected to make
(``frozen_bn.planned_backward_launches``, the tape's rule without a device) against this suite's own walk over the
torch modules (tests/frozen_walk.py)."""
import pytest
import torch.nn as nn

import frozen_walk as W
from egonet_amd import configs, frozen_bn
from egonet_amd.model.heatmapModel import hrnet as hip_hrnet


def _bn_modes(model):
    return {name: m.training for name, m in model.named_modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)}


def _model(freeze=(), freeze_bn=None, head='coordinates'):
    cfg = configs.clone(configs.tiny_config(head))
    cfg['heatmapModel']['init_weights'] = False
    if freeze:
        cfg['heatmapModel']['extra']['freeze_layers'] = list(freeze)
    if freeze_bn is not None:
        cfg['heatmapModel']['extra']['freeze_bn'] = freeze_bn
    return hip_hrnet.get_pose_net(cfg, is_train=True)


def test_freeze_bn_keeps_the_frozen_batchnorms_in_eval_mode(capsys):
    net = _model(W.STEM_FREEZE, freeze_bn=True)
    capsys.readouterr()

    def check():
        modes = _bn_modes(net)
        assert len(modes) > 20
        for name, training in modes.items():
            assert training == (not name.startswith(W.STEM_FREEZE)), name
        assert net.training
    net.train()
    check()
    net.eval()
    assert not any(_bn_modes(net).values()) and not net.training
    net.train()
    check()
    assert not net.bn1.training and not net.layer1[0].bn2.training and net.bn2.training


@pytest.mark.parametrize('flag', [None, False])
def test_without_freeze_bn_nothing_changes(flag, capsys):
    net = _model(W.STEM_FREEZE, freeze_bn=flag)
    capsys.readouterr()
    assert not net.conv1.weight.requires_grad and not net.bn1.weight.requires_grad
    net.train()
    assert all(_bn_modes(net).values())
    net.eval()
    net.train()
    assert all(_bn_modes(net).values())
    assert net.frozen_bn_prefixes == ()


def _walk_self_check():
    """The walk on the unfrozen tiny model: every conv has a weight gradient, every conv but the first a data gradient,
    every BatchNorm the two backward entry points."""
    net = _model()
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d)]
    bns = [m for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
    want = {'dgrad': len(convs) - 1, 'wgrad': len(convs), 'bn_bwd': 2 * len(bns)}
    assert W.expected_launches(net) == want
    return want


@pytest.mark.parametrize('prefixes', [(), W.STEM_FREEZE, W.PED_FREEZE], ids=['none', 'stem', 'pedestrian'])
@pytest.mark.parametrize('bn', ['train', 'eval', 'eval_affine'])
def test_planned_backward_launches_match_the_module_walk(prefixes, bn, capsys):
    full = _walk_self_check()
    net = W.freeze(_model(), prefixes, bn_eval=bn != 'train', affine_trains=bn == 'eval_affine')
    want = W.expected_launches(net)
    got = frozen_bn.planned_backward_launches(net, 64, 64, prune=True)
    assert got == want, (got, want)
    if not prefixes:
        assert want == full
    else:
        assert want['wgrad'] < full['wgrad']
        if bn != 'eval_affine':         # (a trainable gamma on bn1 makes every later input need a gradient)
            assert want['dgrad'] < full['dgrad'] and want['bn_bwd'] < full['bn_bwd']
    # without pruning every layer runs its backward; only the weight gradients of frozen filters are skipped
    unpruned = frozen_bn.planned_backward_launches(net, 64, 64, prune=False)
    assert unpruned['dgrad'] == full['dgrad'] and unpruned['wgrad'] == want['wgrad']
    if bn == 'train':
        assert unpruned['bn_bwd'] == full['bn_bwd']


def test_stem_freeze_counts_by_hand():
    """conv1 is dead; conv2 trains but its input needs nothing; layer1 is frozen yet back-propagated through (conv2 in
    front of it trains): only its weight gradients go."""
    net = W.freeze(_model(), W.STEM_FREEZE)
    full = _walk_self_check()
    layer1_convs = sum(isinstance(m, nn.Conv2d) for m in net.layer1.modules())
    got = frozen_bn.planned_backward_launches(net, 64, 64, prune=True)
    assert got == {'dgrad': full['dgrad'] - 1, 'wgrad': full['wgrad'] - 1 - layer1_convs, 'bn_bwd': full['bn_bwd'] - 2}


def test_train_igrs_freeze_flags_reach_the_config(capsys):
    import argparse
    from tools import train_IGRs
    base = dict(tiny=True, lr=1e-3, epochs=1, batch_frames=2, workers=0, report_every=1, eval_every=0)
    plain = train_IGRs.igr_cfgs(argparse.Namespace(**base))['heatmapModel']['extra']
    assert 'freeze_layers' not in plain and 'freeze_bn' not in plain
    cfg = train_IGRs.igr_cfgs(argparse.Namespace(freeze=['conv1', 'bn1', 'layer1'], freeze_bn=True, **base))
    extra = cfg['heatmapModel']['extra']
    assert extra['freeze_layers'] == ['conv1', 'bn1', 'layer1'] and extra['freeze_bn'] is True
    only = train_IGRs.igr_cfgs(argparse.Namespace(freeze=['conv1'], freeze_bn=False, **base))['heatmapModel']['extra']
    assert only['freeze_layers'] == ['conv1'] and 'freeze_bn' not in only
    with pytest.raises(SystemExit):
        train_IGRs.igr_cfgs(argparse.Namespace(freeze=None, freeze_bn=True, **base))
    cfg['heatmapModel']['init_weights'] = False
    net = hip_hrnet.get_pose_net(cfg, is_train=True)
    capsys.readouterr()
    net.train()
    assert not net.bn1.training and not net.layer1[1].bn3.training and net.bn2.training


def test_eval_mode_batchnorm_without_running_statistics_is_refused():
    bn = nn.BatchNorm2d(8, track_running_stats=False).eval()
    with pytest.raises(NotImplementedError):
        frozen_bn.bn_form(bn)
    assert frozen_bn.bn_form(nn.BatchNorm2d(8)) == frozen_bn.BATCH
    frozen = nn.BatchNorm2d(8).eval()
    assert frozen_bn.bn_form(frozen) == frozen_bn.AFFINE
    frozen.weight.requires_grad = frozen.bias.requires_grad = False
    assert frozen_bn.bn_form(frozen) == frozen_bn.FUSED
