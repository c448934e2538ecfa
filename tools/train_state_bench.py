"""What saving and resuming a native training step costs (egonet_amd/train_state.py, the checkpoints of
egonet_amd/trainer.py) -- what ``training_settings.checkpoint_every`` buys and pays.

    python tools/train_state_bench.py [--passes 5] [--steps 5] [--batch 8] [--rows 2048] [--out profiles/train_state_bench.json]

For HRNet-W48 with the coordinates head (AdamW, the no-decay split, AMSGrad, clipping: every buffer a step can own) and,
separately, for the lifter (66 -> 96, the same optimizer), on synthetic data:
  state_dict_ms         ``step.state_dict()``: the read-back of the step count, the copies of m, v, vmax to the host
  load_state_dict_ms    ``step.load_state_dict(sd)``: validation and the copies back, in place
  checkpoint_write_ms   ``trainer.save_checkpoint``: model + step state + the torch-form dict + generators, two files
  checkpoint_resume_ms  ``trainer.load_checkpoint`` into the same objects
  step_ms_before / step_ms_after    the training step before the first ``state_dict()`` and after a save and a load
Host wall-clock times around a device synchronisation, medians of ``--passes``, spread = max - min; the step in windows
of ``--steps`` steps between two events.  No target is set for any of them.  The file says which device measured."""
import argparse
import gc
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egonet_amd import configs, optim, synth, trainer                  # noqa: E402
from egonet_amd.model import FCmodel                                    # noqa: E402
from egonet_amd.model.heatmapModel import hrnet                         # noqa: E402
from egonet_amd.train_hrnet import HRNetTrainStep                       # noqa: E402
from egonet_amd.train_lifter import LifterTrainStep                     # noqa: E402


def _row(v, digits=3):
    return {'median': round(statistics.median(v), digits), 'spread': round(max(v) - min(v), digits),
            'all': [round(x, digits) for x in v]}


def _host_ms(fn, passes):
    out = []
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def _step_ms(step, batch, passes, steps):
    out = []
    for _ in range(passes):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step.step(*batch)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return out


def measure(name, net, step, batch, cfgs, passes, steps):
    for _ in range(5):
        step.step(*batch)
    gc.collect()
    gc.freeze()                 # as trainer.train does: the per-step Python objects then collect in < 1 ms
    before = _step_ms(step, batch, passes, steps)
    kept = []
    t_sd = _host_ms(lambda: kept.append(step.state_dict()) or kept.pop(), passes)
    sd = step.state_dict()
    t_load = _host_ms(lambda: step.load_state_dict(sd), passes)
    opt = torch.optim.AdamW(optim.no_decay_groups(net, 1e-2, lr=1e-4), amsgrad=True)
    sche = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[10], gamma=0.5)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'train.ckpt')
        t_write = _host_ms(lambda: trainer.save_checkpoint(path, net, step, opt, sche, cfgs, 1, [0], [0.0]), passes)
        size = os.path.getsize(path) + os.path.getsize(trainer.rank_file(path, 0))
        t_resume = _host_ms(lambda: trainer.load_checkpoint(path, net, step, opt, sche, cfgs), passes)
    after = _step_ms(step, batch, passes, steps)
    gc.unfreeze()
    return {'model': name, 'flat_floats': int(step.flat.numel), 'checkpoint_bytes': int(size),
            'state_dict_ms': _row(t_sd), 'load_state_dict_ms': _row(t_load), 'checkpoint_write_ms': _row(t_write),
            'checkpoint_resume_ms': _row(t_resume), 'step_ms_before': _row(before), 'step_ms_after': _row(after)}


def _optim_kw(net):
    return dict(optim_spec=optim.spec('adamw', optim.no_decay_groups(net, 1e-2), lr=1e-4, amsgrad=True), max_grad_norm=1.0)


def w48_row(batch, passes, steps):
    cfg = configs.clone(configs.w48_config('coordinates'))
    cfg.update(exp_type='instanceto2d', optimizer={'optim_type': 'adamw', 'weight_decay': 1e-2, 'amsgrad': True,
                                                  'no_decay_norm_bias': True, 'max_grad_norm': 1.0})
    g = torch.Generator().manual_seed(100)
    x = synth.synth_crops(batch, 3, 256, 256, seed=50).cuda()
    tgt = torch.rand(batch, 33, 64, 64, generator=g).cuda()
    jt = (torch.rand(batch, 33, 2, generator=g) * 256).cuda()
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=1))
    net = net.cuda().train()
    row = measure('HRNet-W48, coordinates head', net, HRNetTrainStep(net, **_optim_kw(net)), (x, tgt, jt), cfg, passes,
                  steps)
    row['crops'] = batch
    return row


def lifter_row(rows, passes, steps):
    cfg = configs.clone(configs.w48_config())
    cfg.update(exp_type='2dto3d', optimizer={'optim_type': 'adamw', 'weight_decay': 1e-2, 'amsgrad': True,
                                            'no_decay_norm_bias': True, 'max_grad_norm': 1.0})
    torch.manual_seed(0)
    net = FCmodel.get_fc_model(1, cfg, 66, 96).cuda().train()
    g = torch.Generator().manual_seed(5)
    batch = (torch.randn(rows, 66, generator=g).cuda(), torch.randn(rows, 96, generator=g).cuda())
    row = measure('lifter 66 -> 96', net, LifterTrainStep(net, **_optim_kw(net)), batch, cfg, passes, steps)
    row['rows'] = rows
    return row


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8, help='crops of the W48 step')
    ap.add_argument('--rows', type=int, default=2048, help='rows of the lifter step')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_state_bench.json'))
    a = ap.parse_args(argv)
    out = {'what': 'host wall-clock ms around a device synchronisation, medians of %d passes, spread = max - min; the '
                   'training step in ms, windows of %d steps between two events, before the first state_dict() and after '
                   'a save and a load; checkpoints written to a temporary directory of the host' % (a.passes, a.steps),
           'device': torch.cuda.get_device_name(0), 'measured_on_device': True,
           'optimizer': 'AdamW, no-decay split (two groups), AMSGrad, max_grad_norm 1.0',
           'models': [w48_row(a.batch, a.passes, a.steps), lifter_row(a.rows, a.passes, a.steps)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps({'out': a.out, 'ms (median)': {
        r['model']: {k: r[k]['median'] for k in r if isinstance(r[k], dict)} for r in out['models']}}))


if __name__ == '__main__':
    main()
