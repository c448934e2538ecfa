"""Training cost of the pixel-shuffle heat-map head (hrnet.py:373-383, 598-600) on HRNet-W48, 256 x 256 crops,
heatmap_size = input_size (upsampling factor 4), synthetic crops / targets / weights:

  native    HRNetTrainStep.step (forward, fused pixel-shuffle loss, backward, Adam: HIP launches only)
  base      the same step on the plain heat-map head (final_layer only): native minus base = the head's cost
  bridge    the reference's loop  optim.zero_grad(); loss = JointsMSELoss(model(x)); loss.backward(); optim.step()
            on the autograd bridge (one node on the native tape; torch owns loss and Adam)
  torch     that loop with EGONET_AMD_AUTOGRAD=0: the module graph in torch (MIOpen / rocBLAS)

    python tools/train_heads_bench.py [--batch 32] [--steps 5] [--warmup 2] [--modes native,base,bridge,torch]

Prints one JSON line per mode (ms per step: mean / min over the timed steps, each step synchronised).

    python tools/train_heads_bench.py --integral [--batch 32] [--steps 5] [--rounds 5] [--out FILE.json]

The plain heat-map head with its integral terms (L_2d and L_cr on the soft-arg-max of the maps, csrc/softargmax.hip):
the W48 step with the terms off, with w_coor, and with w_coor + w_cr, timed in ALTERNATING windows of ``--steps``
steps (off, coor, coor+cr, off, ...; ``--rounds`` windows each, one synchronise per window) -- medians and the windows'
spread; and the two new launches alone on the step's maps (device events).  One JSON object, also written to ``--out``.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egonet_amd import configs, synth                                   # noqa: E402
from egonet_amd.model.heatmapModel import hrnet                         # noqa: E402
from egonet_amd.train_hrnet import HRNetTrainStep                       # noqa: E402
from oracle.hrnet_train_oracle import joints_mse_loss                   # noqa: E402


def _model(pixel_shuffle):
    cfg = configs.w48_config('heatmap')
    if pixel_shuffle:
        cfg['heatmapModel']['pixel_shuffle'] = True
        cfg['heatmapModel']['heatmap_size'] = [256, 256]
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=1))
    return net.cuda().train(), cfg


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sum(ts) / len(ts), min(ts)


def _integral(a):
    """The three variants of the heat-map-head step in alternating windows, and the two soft-arg-max launches alone."""
    import statistics
    from egonet_amd import softargmax
    n, J, hm = a.batch, 33, 64
    g = torch.Generator().manual_seed(100)
    x = synth.synth_crops(n, 3, 256, 256, seed=50).cuda()
    tgt = torch.rand(n, J, hm, hm, generator=g).cuda()
    jt = (torch.rand(n, J, 2, generator=g) * 256).cuda()
    variants = {'off': dict(w_coor=0.0), 'coor': dict(w_coor=0.1), 'coor_cr': dict(w_coor=0.1, w_cr=0.05)}
    steps = {}
    for name, kw in variants.items():
        tr = HRNetTrainStep(_model(False)[0], lr=1e-3, **kw)
        tr.apply_cr_loss = True
        steps[name] = tr
        for _ in range(a.warmup):
            tr.step(x, tgt, jt if kw['w_coor'] else None)
    torch.cuda.synchronize()
    windows = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, tr in steps.items():
            joints = jt if variants[name]['w_coor'] else None
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.step(x, tgt, joints)
            torch.cuda.synchronize()
            windows[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    out = {'model': 'W48 heatmap head, 256 x 256 crops, %d x %d maps' % (hm, hm), 'batch': n, 'steps_per_window': a.steps,
           'rounds': a.rounds, 'warmup': a.warmup, 'ms_per_step': {}}
    for name, w in windows.items():
        out['ms_per_step'][name] = {'median': round(statistics.median(w), 3), 'min': round(min(w), 3),
                                    'max': round(max(w), 3), 'windows': [round(v, 3) for v in w]}
    med = {k: v['median'] for k, v in out['ms_per_step'].items()}
    out['added_ms'] = {'coor': round(med['coor'] - med['off'], 3), 'coor_cr': round(med['coor_cr'] - med['off'], 3)}
    # the two launches alone, on maps of the step's shape (cs = 36)
    cs = (J + 3) // 4 * 4
    z = (torch.randn(n, hm, hm, cs, generator=torch.Generator().manual_seed(1)) * 3).cuda()
    dc = torch.randn(n, J, 2, generator=torch.Generator().manual_seed(2)).cuda()
    dz = torch.zeros_like(z)
    coords, save = softargmax.forward(z, n, hm, hm, J, cs, float(hm), float(hm))
    softargmax.backward(z, save, dc, n, n, hm, hm, J, cs, float(hm), float(hm), dz, True)
    torch.cuda.synchronize()

    def events(fn, reps=50):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return {'median_us': round(statistics.median(ts), 2), 'min_us': round(min(ts), 2), 'max_us': round(max(ts), 2)}
    map_bytes = n * hm * hm * cs * 4
    out['launches_alone'] = {
        'forward': events(lambda: softargmax.forward(z, n, hm, hm, J, cs, float(hm), float(hm))),
        'backward': events(lambda: softargmax.backward(z, save, dc, n, n, hm, hm, J, cs, float(hm), float(hm), dz, True)),
        'map_bytes': map_bytes,
        # forward reads the maps twice (max, sums), backward reads them once and read-modify-writes the gradient
        'bytes_floor': {'forward': 2 * map_bytes, 'backward': 3 * map_bytes}}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(out, indent=1) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--integral', action='store_true', help="the heat-map head's integral terms (see the module text)")
    ap.add_argument('--rounds', type=int, default=5, help='--integral: windows per variant')
    ap.add_argument('--out', default=None, help='--integral: also write the JSON object here')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--modes', default='native,base,bridge,torch')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.integral:
        return _integral(a)
    n = a.batch
    g = torch.Generator().manual_seed(100)
    x = synth.synth_crops(n, 3, 256, 256, seed=50).cuda()
    for mode in a.modes.split(','):
        if mode == 'base':
            net, cfg = _model(False)
            tgt = torch.rand(n, 33, 64, 64, generator=g).cuda()
        else:
            net, cfg = _model(True)
            tgt = torch.rand(n, 33, 256, 256, generator=g).cuda()
        if mode in ('native', 'base'):
            tr = HRNetTrainStep(net, lr=1e-3, w_coor=0.0)

            def fn():
                tr.step(x, tgt, None)
        elif mode in ('bridge', 'torch'):
            os.environ['EGONET_AMD_AUTOGRAD'] = '1' if mode == 'bridge' else '0'
            optim = torch.optim.Adam(net.parameters(), lr=1e-3)

            def fn():
                optim.zero_grad()
                joints_mse_loss(net(x), tgt).backward()
                optim.step()
        else:
            raise SystemExit('unknown mode %r' % mode)
        mean, best = _time(fn, a.steps, a.warmup)
        print(json.dumps({'mode': mode, 'model': 'W48 heatmap' + (' + pixel shuffle f=4' if mode != 'base' else ''),
                          'batch': n, 'ms_per_step': round(mean, 2), 'ms_min': round(best, 2),
                          'crops_per_s': round(n * 1e3 / mean, 1), 'steps': a.steps, 'warmup': a.warmup}), flush=True)
        del net, fn
        torch.cuda.empty_cache()
    os.environ.pop('EGONET_AMD_AUTOGRAD', None)


if __name__ == '__main__':
    main()
