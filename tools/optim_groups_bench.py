"""What the grouped optimizer launch (csrc/optim.hip) costs against the old one-launch update.

    python tools/optim_groups_bench.py [--passes 7] [--reps 20] [--steps 3] [--no-step] [--out profiles/optim_groups_bench.json]

On the flat parameter buffers of HRNet-W48 and of the lifter (the layout ``train_common.FlatParams`` gives them), us per
launch of
  old               egn_adam_l2_step_dev_f32 (tick + update), the code this measurement's pull request does not touch
  one_group         the grouped launch, Adam with weight decay, one group
  no_decay_split    AdamW, two groups: conv / linear weights against BatchNorm gamma / beta and biases
  amsgrad           the split with AMSGrad in both groups (36 against 28 bytes per element)
  norm              the two launches of egn_grad_norm_clip_f32 alone
  split_clipped     norm + the split with the coefficient multiplied in
and on 1 M floats ``alt3_4float``: three groups in alternating segments of 4 floats, the table-bound worst case (one
lane of a wave busy per item), against ``old`` on the same buffer.  Then the W48 training step at 32 crops
(tools/train_hc_bench.py's data and warm-up) plain against no-decay split + clipping.

Method of tools/precision_bench.py: windows of ``--reps`` launches between two events, the variants alternating,
medians of ``--passes`` windows, spread = max - min."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egonet_amd import _lib, configs, optim, synth                      # noqa: E402
from egonet_amd.model import FCmodel                                    # noqa: E402
from egonet_amd.model.heatmapModel import hrnet                         # noqa: E402


def _layout(net):
    """(numel, group) per trainable parameter in FlatParams order; group 1 = no weight decay."""
    g1 = {id(p) for p in optim.no_decay_groups(net, 1e-2)[1]['params']}
    return [(p.numel(), int(id(p) in g1)) for p in net.parameters() if p.requires_grad]


def _segments(layout):
    segs, at = [], 0
    for n, k in layout:
        end = at + (n + 3) // 4 * 4
        if segs and segs[-1][2] == k:
            segs[-1] = (segs[-1][0], end, k)
        else:
            segs.append((at, end, k))
        at = end
    return segs, at


def _groups(family, n, amsgrad=False):
    rows = [dict(params=[], lr=1e-4, weight_decay=1e-2, amsgrad=amsgrad), dict(params=[], lr=1e-4, weight_decay=0.0,
                                                                               amsgrad=amsgrad),
            dict(params=[], lr=5e-5, weight_decay=1e-3, amsgrad=amsgrad)]
    return optim.group_table(optim.spec(family, rows[:n]))


class Buffers(object):
    def __init__(self, total):
        g = torch.Generator(device='cuda').manual_seed(0)
        self.n = total
        self.p = 0.1 * torch.randn(total, device='cuda', generator=g)
        self.g = 1e-3 * torch.randn(total, device='cuda', generator=g)
        self.m, self.v, self.vmax = (torch.zeros(total, device='cuda') for _ in range(3))
        self.lr = torch.full((1,), 1e-4, device='cuda')
        self.step = torch.zeros(1, dtype=torch.int32, device='cuda')
        self.clip = torch.zeros(2, device='cuda')
        self.ws = optim.norm_workspace('cuda')

    def old(self):
        _lib.check(_lib.lib().egn_adam_l2_step_dev_f32(_lib.ptr(self.p), _lib.ptr(self.g), _lib.ptr(self.m),
                                                       _lib.ptr(self.v), self.n, _lib.ptr(self.lr), 0.9, 0.999, 1e-8,
                                                       1e-2, _lib.ptr(self.step), None))

    def grouped(self, family, segs, ngroups, amsgrad=False, clip=False, norm=True):
        groups = _groups(family, ngroups, amsgrad)
        items = optim.work_items(segs, _lib.lib().egn_optim_item_floats())
        gd, idv = optim._to_device(groups, 'cuda'), optim._to_device(items, 'cuda')

        def run():
            if clip and norm:
                _lib.check(optim.grad_norm_clip(self.g, self.n, 1.0, self.ws, self.clip, None))
            _lib.check(optim.grouped_step(family, self.p, self.g, self.m, self.v, self.vmax if amsgrad else None, self.n,
                                          groups, gd, items, idv, self.clip if clip else None, self.step, None))
        run.items = len(items)
        return run

    def norm(self):
        _lib.check(optim.grad_norm_clip(self.g, self.n, 1.0, self.ws, self.clip, None))


def measure(variants, passes, reps):
    """name -> callable; -> name -> {median_us, spread_us, us}: windows of ``reps`` calls, the variants alternating."""
    t = {k: [] for k in variants}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(passes):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {k: {'median_us': round(statistics.median(v), 2), 'spread_us': round(max(v) - min(v), 2),
                'us': [round(x, 2) for x in v]} for k, v in t.items()}


def flat_rows(name, layout, passes, reps):
    segs, total = _segments(layout)
    b = Buffers(total)
    one = [(0, total, 0)]
    variants = {
        'old': b.old,
        'one_group': b.grouped('adam', one, 1),
        'no_decay_split': b.grouped('adamw', segs, 2),
        'amsgrad': b.grouped('adamw', segs, 2, amsgrad=True),
        'norm': b.norm,
        'split_clipped': b.grouped('adamw', segs, 2, clip=True),
    }
    rows = measure(variants, passes, reps)
    old = rows['old']['median_us']
    for k, r in rows.items():
        r['vs_old'] = round(r['median_us'] / old, 3)
    return {'buffer': name, 'floats': total, 'segments_of_the_split': len(segs),
            'work_items_of_the_split': variants['no_decay_split'].items, 'launches': rows}


def alt3_row(passes, reps):
    total = 1 << 20
    segs = [(4 * i, 4 * i + 4, i % 3) for i in range(total // 4)]
    b = Buffers(total)
    variants = {'old': b.old, 'alt3_4float': b.grouped('adam', segs, 3), 'one_group': b.grouped('adam', [(0, total, 0)], 1)}
    rows = measure(variants, passes, reps)
    for r in rows.values():
        r['vs_old'] = round(r['median_us'] / rows['old']['median_us'], 3)
    return {'buffer': '1 M floats, three groups in segments of 4 floats', 'floats': total,
            'work_items': variants['alt3_4float'].items, 'launches': rows}


def step_row(batch, passes, steps):
    from egonet_amd.train_hrnet import HRNetTrainStep
    import gc
    cfg = configs.w48_config('coordinates')
    g = torch.Generator().manual_seed(100)
    x = synth.synth_crops(batch, 3, 256, 256, seed=50).cuda()
    tgt = torch.rand(batch, 33, 64, 64, generator=g).cuda()
    jt = (torch.rand(batch, 33, 2, generator=g) * 256).cuda()
    trs = {}
    for mode in ('plain', 'split_clipped'):
        net = hrnet.get_pose_net(cfg, is_train=False)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=1))
        net = net.cuda().train()
        if mode == 'plain':
            trs[mode] = HRNetTrainStep(net, lr=1e-4, weight_decay=1e-2)
        else:
            trs[mode] = HRNetTrainStep(net, optim_spec=optim.spec('adamw', optim.no_decay_groups(net, 1e-2), lr=1e-4),
                                       max_grad_norm=1.0)
        for _ in range(2):
            trs[mode].step(x, tgt, jt)
    gc.collect()
    gc.freeze()
    t = {k: [] for k in trs}
    for _ in range(passes):
        for k, tr in trs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                tr.step(x, tgt, jt)
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) / steps)
    row = {'crops': batch, 'steps_per_window': steps}
    for k, v in t.items():
        row[k] = {'median_ms_per_step': round(statistics.median(v), 3), 'spread_ms': round(max(v) - min(v), 3),
                  'ms': [round(q, 3) for q in v]}
    row['split_clipped_minus_plain_ms'] = round(row['split_clipped']['median_ms_per_step'] -
                                                row['plain']['median_ms_per_step'], 3)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--no-step', action='store_true', help='the launches alone, no W48 training step')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_groups_bench.json'))
    a = ap.parse_args(argv)
    w48 = hrnet.get_pose_net(configs.w48_config('coordinates'), is_train=False)
    lifter = FCmodel.get_fc_model(1, configs.w48_config(), 66, 96)
    out = {'what': 'us per optimizer launch pair (tick + update; norm: its two launches) on the flat parameter buffers, '
                   'windows of %d launches between two events, variants alternating, medians of %d windows, spread = '
                   'max - min; the W48 step at %d crops in ms, windows of %d steps' % (a.reps, a.passes, a.batch, a.steps),
           'device': torch.cuda.get_device_name(0), 'item_floats': _lib.lib().egn_optim_item_floats(),
           'lookup': 'work items (begin, length <= item_floats, group), one per wave; the LDS segment search was not built',
           'flat': [flat_rows('HRNet-W48', _layout(w48), a.passes, a.reps),
                    flat_rows('lifter', _layout(lifter), a.passes, a.reps)],
           'worst_case': alt3_row(a.passes, a.reps)}
    del w48, lifter
    if not a.no_step:
        out['w48_step'] = step_row(a.batch, a.passes, a.steps)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    brief = {r['buffer']: {k: (v['median_us'], v['spread_us']) for k, v in r['launches'].items()} for r in out['flat']}
    print(json.dumps({'out': a.out, 'us (median, spread)': brief,
                      'worst_case': {k: v['median_us'] for k, v in out['worst_case']['launches'].items()},
                      'w48_step': out.get('w48_step', {}).get('split_clipped_minus_plain_ms')}))


if __name__ == '__main__':
    main()
