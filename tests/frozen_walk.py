"""What the backward of a native HRNet step launches for a given set of frozen layers, worked out from the torch
modules alone (helper of tests/test_frozen_finetune_cpu.py and tests/test_gpu_frozen_finetune.py; imported, not a
conftest).

The walk follows the modules' own ``forward`` (hrnet.py: ``_Residual.forward``, ``HighResolutionModule.forward``,
``PoseHighResolutionNet._trunk`` / ``_torch_forward``), not the engine's recorder, and carries one bit per tensor: does
it need a gradient.  Per conv (+ BatchNorm) layer whose output needs one:
  bn_bwd  += 2 (the two BatchNorm backward entry points), or 1 where the BatchNorm is in eval mode with gamma and beta
             frozen (the fused form's single pass);
  wgrad   += 1 where the conv weight trains;
  dgrad   += 1 where the layer's input needs a gradient.
Every output of the model is taken to receive a gradient (the bridge with a loss on all outputs; the native step with
its default weights).
"""
import torch.nn as nn

PED_FREEZE = ('conv1', 'bn1', 'conv2', 'bn2', 'layer1', 'transition1', 'stage2')     # KITTI_train_IGRs_Ped.yml:110-117
STEM_FREEZE = ('conv1', 'bn1', 'layer1')


def freeze(model, prefixes, bn_eval=False, affine_trains=False):
    """requires_grad = False under ``prefixes`` (get_pose_net's rule); ``bn_eval``: their BatchNorm modules in eval
    mode; ``affine_trains``: ... with gamma / beta left trainable."""
    for name, p in model.named_parameters():
        if name.startswith(tuple(prefixes)):
            p.requires_grad = False
    for name, m in model.named_modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm) and name.startswith(tuple(prefixes)):
            if bn_eval:
                m.eval()
            if affine_trains:
                m.weight.requires_grad = True
                m.bias.requires_grad = True
    return model


class _Count(object):
    def __init__(self):
        self.c = {'dgrad': 0, 'wgrad': 0, 'bn_bwd': 0}

    def layer(self, conv, bn, x, res=False):
        ps = [conv.weight, conv.bias] + ([bn.weight, bn.bias] if bn is not None else [])
        need = x or res or any(p is not None and p.requires_grad for p in ps)
        if not need:
            return False
        if bn is not None:
            fused = (not bn.training) and not (bn.weight.requires_grad or bn.bias.requires_grad)
            self.c['bn_bwd'] += 1 if fused else 2
        self.c['wgrad'] += int(conv.weight.requires_grad)
        self.c['dgrad'] += int(x)
        return True

    def block(self, blk, x):
        y = x
        for i in range(1, blk.depth + 1):
            conv, bn = getattr(blk, 'conv%d' % i), getattr(blk, 'bn%d' % i)
            if i < blk.depth:
                y = self.layer(conv, bn, y)
            else:
                res = x if blk.downsample is None else self.layer(blk.downsample[0], blk.downsample[1], x)
                y = self.layer(conv, bn, y, res)
        return y

    def chain(self, seq, x):
        """A Sequential of residual blocks, conv + BN (+ ReLU / Upsample) runs and plain convs."""
        mods = list(seq)
        k = 0
        while k < len(mods):
            m = mods[k]
            if hasattr(m, 'depth'):
                x = self.block(m, x)
            elif isinstance(m, nn.Sequential):
                x = self.chain(m, x)
            elif isinstance(m, (nn.Conv2d, nn.Linear)):
                bn = mods[k + 1] if k + 1 < len(mods) and isinstance(mods[k + 1], nn.modules.batchnorm._BatchNorm) else None
                x = self.layer(m, bn, x)
            k += 1
        return x

    def module(self, mod, xs):
        xs = [self.chain(br, x) for br, x in zip(mod.branches, xs)]
        if mod.fuse_layers is None:
            return xs
        outs = []
        for row in mod.fuse_layers:
            terms = [xs[j] if row[j] is None else self.chain(row[j], xs[j]) for j in range(mod.num_branches)]
            outs.append(any(terms))
        return outs


def expected_launches(model):
    k = _Count()
    x = k.layer(model.conv1, model.bn1, False)
    x = k.layer(model.conv2, model.bn2, x)
    ys = [k.chain(model.layer1, x)]
    for idx in (1, 2, 3):
        trans = getattr(model, 'transition%d' % idx)
        xs = [ys[i] if t is None else k.chain(t, ys[-1]) for i, t in enumerate(trans)]
        for mod in getattr(model, 'stage%d' % (idx + 1)):
            xs = k.module(mod, xs)
        ys = xs
    y = ys[0]
    if model.head_type == 'heatmap':
        y = k.chain([model.final_layer], y)
        if model.pixel_shuffle:
            k.chain(model.upsample_layer, y)
    elif model.head_type == 'coordinates':
        maps = k.chain(model.head1, y)
        k.chain(model.head2, maps)
    else:
        k.chain(model.final_fc, k.chain(model.head, y))
    return k.c
