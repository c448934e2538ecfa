#!/usr/bin/env python
"""Step time of the native HRNet training step with a frozen prefix: the parent commit against this commit with the
pruned backward, and with the frozen prefix's BatchNorm layers in eval mode as well (fused and unfused form).

    python tools/frozen_finetune_bench.py --parent-tree DIR [--out profiles/frozen_finetune_bench.json]

``DIR`` is a checkout of the parent commit with its library built (``git worktree add DIR HEAD~1 && (cd DIR && python -m
egonet_amd.build)``).  Every measurement is a process of its own (``--child``), the variants alternate round by round on
the same GPU in the same session; a window is ``--steps`` steps between two device synchronisations after ``--warmup``
steps, the figure of a variant is the median of all its windows and the spread their min .. max.  A difference counts
only where it exceeds the windows' spread.

Models: HRNet-W48 at 256 x 256 and W32 at 192 x 256 (the Pedestrian config), 32 crops, coordinate head, both with the
Pedestrian config's freeze list (conv1 .. stage2).  Variants:
  parent     the parent commit's step (frozen parameters: requires_grad = False, every BatchNorm in train mode)
  noprune    this commit, EGONET_AMD_PRUNE_BACKWARD=0 (control: should equal parent)
  prune      this commit, the backward stops at the frozen frontier
  prune_bn   ... and the frozen prefix's BatchNorm layers in eval mode, gamma / beta frozen (fused form)
  prune_bn_affine   ... in eval mode with gamma / beta trainable (unfused form)
Recorded per variant: ms per step, convolution launches per step (egn_direct_conv_count: forward, data gradient, weight
gradient), the backward's launch counters (last_backward_launches), torch.cuda.max_memory_allocated.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PED_FREEZE = ('conv1', 'bn1', 'conv2', 'bn2', 'layer1', 'transition1', 'stage2')
VARIANTS = ('parent', 'noprune', 'prune', 'prune_bn', 'prune_bn_affine')
MODELS = {'w48_256': (48, (256, 256)), 'w32_192x256': (32, (192, 256))}


def child(a):
    tree = a.parent_tree if a.variant == 'parent' else ROOT
    sys.path.insert(0, tree)
    if a.variant == 'noprune':
        os.environ['EGONET_AMD_PRUNE_BACKWARD'] = '0'
    import torch
    from egonet_amd import _lib, configs, synth
    from egonet_amd.model.heatmapModel import hrnet
    from egonet_amd.train_hrnet import HRNetTrainStep
    assert os.path.realpath(os.path.dirname(os.path.dirname(hrnet.__file__)))\
        .startswith(os.path.realpath(tree)), hrnet.__file__
    width, (iw, ih) = MODELS[a.model]
    cfg = configs.hrnet_config(width, (iw, ih), 33, 'coordinates')
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=5))
    net = net.cuda().train()
    for name, p in net.named_parameters():
        if name.startswith(PED_FREEZE):
            p.requires_grad = False
    if a.variant.startswith('prune_bn'):
        for name, m in net.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d) and name.startswith(PED_FREEZE):
                m.eval()
                if a.variant == 'prune_bn_affine':
                    m.weight.requires_grad = m.bias.requires_grad = True
    n = a.crops
    gen = torch.Generator().manual_seed(1)
    x = synth.synth_crops(n, 3, ih, iw, seed=2).cuda()
    tg = torch.rand(n, 33, ih // 4, iw // 4, generator=gen).cuda()
    jt = (torch.rand(n, 33, 2, generator=gen) * torch.tensor([iw, ih], dtype=torch.float32)).cuda()
    tr = HRNetTrainStep(net, lr=1e-4)
    L = _lib.lib()
    for _ in range(a.warmup):
        tr.step(x, tg, jt)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    c0 = L.egn_direct_conv_count()
    tr.step(x, tg, jt)
    launches = L.egn_direct_conv_count() - c0     # forward, data-gradient and weight-gradient convolutions
    torch.cuda.synchronize()
    windows = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss = tr.step(x, tg, jt)
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) * 1e3 / a.steps)
    print('RESULT ' + json.dumps({'model': a.model, 'variant': a.variant, 'ms': windows, 'conv_launches': int(launches),
                                  'max_memory_allocated': int(torch.cuda.max_memory_allocated()),
                                  'loss': float(loss.item()),
                                  'backward_launches': getattr(tr, 'last_backward_launches', None)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--parent-tree', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frozen_finetune_bench.json'))
    ap.add_argument('--crops', type=int, default=32)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--windows', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--models', nargs='+', default=sorted(MODELS), choices=sorted(MODELS))
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--variant', choices=VARIANTS)
    ap.add_argument('--model', choices=sorted(MODELS))
    ap.add_argument('--child-timeout', type=float, default=240.0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    variants = [v for v in VARIANTS if v != 'parent' or a.parent_tree]
    # every variant chooses its tile configurations the same way: the shipped table, else the cost model (no in-process
    # tuning, whose outcome would differ from child to child)
    os.environ.setdefault('EGONET_AMD_AUTOTUNE', '0')
    rows = {}
    for model in a.models:
        for rnd in range(a.rounds):
            for v in variants:              # alternating: one window set of each variant per round
                cmd = [sys.executable, os.path.abspath(__file__), '--child', '--variant', v, '--model', model,
                       '--crops', str(a.crops), '--warmup', str(a.warmup), '--steps', str(a.steps),
                       '--windows', str(a.windows)] + (['--parent-tree', a.parent_tree] if a.parent_tree else [])
                out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                                     timeout=a.child_timeout)
                line = [ln for ln in out.stdout.splitlines() if ln.startswith('RESULT ')]
                if out.returncode != 0 or not line:
                    # a child that failed on the GPU ends the whole measurement: nothing more is started on that card
                    sys.stdout.write(out.stdout[-3000:])
                    raise SystemExit('child %s / %s failed with status %d' % (model, v, out.returncode))
                r = json.loads(line[0][7:])
                e = rows.setdefault((model, v), dict(r, ms=[]))
                e['ms'] += r['ms']
                print('%s %-16s round %d: %s ms/step, %d conv launches' % (model, v, rnd,
                                                                           ['%.2f' % t for t in r['ms']],
                                                                           r['conv_launches']), flush=True)
    result = {'autotune': os.environ['EGONET_AMD_AUTOTUNE'], 'crops': a.crops, 'steps_per_window': a.steps,
              'warmup': a.warmup, 'freeze': list(PED_FREEZE), 'rows': []}
    for (model, v), e in rows.items():
        ms = e.pop('ms')
        result['rows'].append(dict(e, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), windows=len(ms)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
