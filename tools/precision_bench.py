#!/usr/bin/env python
"""What the opt-in f16-operand mode (precision = 'f16', csrc/conv_h.hip) buys and what it costs in accuracy.

    python tools/precision_bench.py [--passes 7] [--steps 20] [--out profiles/f16_mode_bench.json]

1. Per class -- the four 3x3 / stride 1 classes of HRNet-W48 (48 -> 48 @ 64^2, 96 -> 96 @ 32^2, 192 -> 192 @ 16^2,
   384 -> 384 @ 8^2) at 64 and at 16 crops, residual + ReLU epilogue -- microseconds of the f16-operand op against the
   fp32 op the shipped tile table picks for the shape, both as ops of ONE program timed by ``egn_program_run_timed``
   (hipEvents around each op, serial on one stream) in the same process.  Two programs hold the pair in either order and
   alternate, so neither op always finds the input warmed by the other; ``--passes`` timed passes after two warm-ups,
   median and spread (max - min) per op.  ``faster`` = the medians differ by more than the larger of the two spreads.
2. The 64-crop and 16-crop ``EgoNet.infer_crops`` step of bench.py (HRNet-W48, coordinate head, seeded weights) in both
   modes in the same process: windows of ``--steps`` steps, the modes alternating, medians of ``--passes`` windows; a host
   clock around work that ends in a device synchronise.
3. Accuracy on the device: the test model of tests/f16_mode_case.py against its fp32 CPU forward beside the CPU
   emulation's E (tests/golden/f16_mode_bounds.json), and HRNet-W48 at 256 x 256 on 8 crops, 'f16' against 'f32' on the
   device: heat-maps, coordinates in pixels, soft-arg-max in pixels, arg-max agreement.  Seeded weights, not trained.

``--s2`` measures what precision = 'f16s2' adds to 'f16' by the same method (default --out profiles/f16s2_mode_bench.json):
every 3x3 / stride 2 class of HRNet-W48 (the fuse layers' 48 -> 48 / 96 / 192 / 384, 96 -> 96 / 192 / 384, 192 -> 384 and the
transitions' 96 -> 192, 192 -> 384, at the map sizes the network has them, with the fuse layers' epilogues) against the
fp32 op of the shipped table; the step in 'f16' against 'f16s2'; the device-side deviation of 'f16s2' from 'f32'.  A class
stays lowered only if it is faster by more than the spread at 64 crops and not slower beyond the spread at 16 crops at
every map size (``keep``); the others are what engine.F16S2_FP32_CLASSES has to name."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from egonet_amd import _lib, configs, engine, synth, tuner                       # noqa: E402
from egonet_amd.common.img_proc import modify_bbox                               # noqa: E402
from egonet_amd.model.egonet import EgoNet                                       # noqa: E402

CLASSES = ((48, 64), (96, 32), (192, 16), (384, 8))       # (channels, map side)
# stride 2: (cin, cout, INPUT map side, epilogue) -- a fuse chain from branch j to i is i - j - 1 units cj -> cj with ReLU
# and one cj -> ci without; transition2 / transition3 are 96 -> 192 @ 32 and 192 -> 384 @ 16 with ReLU (same shapes)
RELU, NONE = engine.ACT_RELU, engine.ACT_NONE
S2_CLASSES = ((48, 48, 64, RELU), (48, 48, 32, RELU), (48, 96, 64, NONE), (48, 192, 32, NONE), (48, 384, 16, NONE),
              (96, 96, 32, RELU), (96, 192, 32, NONE), (96, 384, 16, NONE), (192, 384, 16, NONE))


def class_row(n, c, hw, passes, cout=None, stride=1, act=RELU):
    """Stride 1: c -> c with residual (the default).  Stride 2: c -> cout on an hw x hw INPUT, no residual."""
    L = _lib.lib()
    dev = torch.device('cuda')
    cin, c = c, (c if cout is None else cout)
    ho = (hw - 1) // stride + 1
    g = torch.Generator().manual_seed(c + n)
    x = torch.relu(torch.randn(n, hw, hw, cin, generator=g)).cuda()
    wt = torch.randn(c, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)
    key = (n, hw, hw, cin, cin, c, c, 3, 3, stride, 1, stride == 1, False)
    cfg = tuner.choose(dev, key, tuner.ALL_KINDS)
    w32 = engine.pack_for_kind(wt, tuner.kind_of(cfg)).cuda()
    w16 = engine.pack_conv_weight_f16(wt).cuda()
    sc, sh = (torch.rand(c, generator=g) + 0.5).cuda(), torch.randn(c, generator=g).cuda()
    res = torch.randn(n, ho, ho, c, generator=g).cuda()          # (stride 2: bound to its slot, read by neither op)
    y32, y16 = torch.empty_like(res), torch.empty_like(res)
    tensors = (x, w32, w16, sc, sh, res, y32, y16)
    progs = []
    for order in ((0, 1), (1, 0)):
        p = C.c_void_p(L.egn_program_create(8))
        for slot, t in enumerate(tensors):
            _lib.check(L.egn_program_bind(p, slot, _lib.ptr(t)))
        R = [_lib.Ref(s, 0) for s in range(8)]
        for which in order:
            if which == 0:
                _lib.check(L.egn_program_add_conv2d(p, R[0], R[1], R[3], R[4], R[5] if stride == 1 else _lib.NULL_REF, R[6],
                                                    n, hw, hw, cin, cin, c, c, 3, 3, stride, 1, act, 0, cfg), 'fp32 op')
            elif stride == 2:
                _lib.check(L.egn_program_add_conv3x3s2_h(p, R[0], R[2], R[3], R[4], R[7], n, hw, hw, cin, c, act), 'f16 op')
            else:
                _lib.check(L.egn_program_add_conv3x3_h(p, R[0], R[2], R[3], R[4], R[5], R[7], n, hw, hw, c, c,
                                                       engine.ACT_RELU), 'f16 op')
        progs.append((p, order))
    st = _lib.current_stream()
    us = {0: [], 1: []}
    ms = (C.c_float * 2)()
    try:
        for it in range(2 + passes):
            got = {0: [], 1: []}
            for p, order in progs:
                _lib.check(L.egn_program_run_timed(p, st, ms, 2))
                for k, which in enumerate(order):
                    got[which].append(ms[k] * 1e3)
            if it >= 2:
                for which in (0, 1):
                    us[which].append(sum(got[which]) / len(got[which]))
        torch.cuda.synchronize()
        diff = float((y16 - y32).abs().max())
    finally:
        for p, _ in progs:
            L.egn_program_destroy(p)
    m32, m16 = statistics.median(us[0]), statistics.median(us[1])
    s32, s16 = max(us[0]) - min(us[0]), max(us[1]) - min(us[1])
    px = float(n * hw * hw)
    # x, res, y once at 8 TB/s (stride 2: x and y)
    floor = 4.0 * (px * c * 3 if stride == 1 else px * cin + float(n * ho * ho) * c) / 8.0e12 * 1e6
    row = {'crops': n, 'class': '%d->%d@%dx%d' % (cin, c, hw, hw), 'fp32_cfg': cfg, 'fp32_us': m32, 'fp32_spread_us': s32,
           'f16_us': m16, 'f16_spread_us': s16, 'fp32_all_us': us[0], 'f16_all_us': us[1],
           'speedup': m32 / m16, 'faster': bool(m32 - m16 > max(s32, s16)),
           'f16_activation_bytes_floor_us': floor, 'max_abs_diff_f16_vs_fp32': diff}
    if stride == 2:
        row.update(stride=2, act=act, not_slower=bool(m16 - m32 <= max(s32, s16)))
    return row


def _w48_ego():
    cfg = configs.w48_config('coordinates')
    ego = EgoNet(cfg, pre_trained=False)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=1))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=2))
    ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    return ego.eval().cuda()


def step_row(ego, batch, passes, steps, modes=('f32', 'f16')):
    crops = synth.synth_crops(batch, 3, 256, 256, seed=100).cuda()
    rets = [modify_bbox(b, 1.0) for b in synth.synth_boxes(batch, seed=5)]
    centers = torch.tensor(np.stack([r['c'] for r in rets]), dtype=torch.float64, device='cuda')
    scales = torch.tensor(np.stack([r['s'] for r in rets]), dtype=torch.float64, device='cuda')

    def window(prec):
        ego.HC.precision = prec
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            res = ego.infer_crops(crops, centers, scales, decode='coords', to_host=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, res
    ma, mb = modes
    nops = {}
    for prec in modes:
        window(prec)
        nops[prec] = len(ego.HC._hip_engine().last_f16_ops)      # (the warm-up window recorded the mode's program)
    t = {ma: [], mb: []}
    for _ in range(passes):
        for prec in modes:
            t[prec].append(window(prec)[0])
    ego.HC.precision = 'f32'
    m32, m16 = statistics.median(t[ma]), statistics.median(t[mb])
    row = {'crops': batch, 'steps_per_window': steps, ma + '_ms_per_step': m32, mb + '_ms_per_step': m16,
           ma + '_all_ms': t[ma], mb + '_all_ms': t[mb], ma + '_crops_per_s': batch / m32 * 1e3,
           mb + '_crops_per_s': batch / m16 * 1e3, 'speedup': m32 / m16}
    row.update({m + '_ops': nops[m] for m in modes if m != 'f32'})
    return row


def accuracy(ego, mode='f16'):
    if mode == 'f16':
        import f16_mode_case as case
    else:
        import f16s2_mode_case as case
    out = {}
    with open(case.BOUNDS_PATH) as f:
        bounds = json.load(f)
    for head in case.HEADS:
        net = case.model(head)
        x = case.crops('forward')
        ref = case.cpu_f32(net, x)
        net = net.cuda()
        row = {}
        with torch.no_grad():
            for prec in ('f32', mode):
                net.precision = prec
                row[prec] = case.deviations(case.quantities(net(x.cuda())), ref)
        row['E_cpu_emulation'] = {k: bounds[head]['forward'][k] for k in row[mode]}
        out['test_model_%s_vs_fp32_cpu' % head] = row
    # HRNet-W48 at 256 x 256: the mode against 'f32', both on the device
    x = synth.synth_crops(8, 3, 256, 256, seed=100).cuda()
    res = {}
    with torch.no_grad():
        for prec in ('f32', mode):
            ego.HC.precision = prec
            maps, coords = ego.HC(x)
            res[prec] = (maps.double().cpu(), coords.double().cpu())
    ego.HC.precision = 'f32'
    (m32, c32), (m16, c16) = res['f32'], res[mode]

    def soft(m):
        n, k, h, w = m.shape
        p = torch.softmax(m.reshape(n, k, h * w), dim=2).reshape(n, k, h, w)
        xs = (p.sum(2) * torch.arange(w, dtype=torch.float64)).sum(2)
        ys = (p.sum(3) * torch.arange(h, dtype=torch.float64)).sum(2)
        return torch.stack([xs, ys], dim=2) * (256.0 / w)
    out['w48_256x256_8_crops_%s_vs_f32_device' % mode] = {
        'heatmap_max_abs_diff': float((m16 - m32).abs().max()), 'heatmap_max_abs': float(m32.abs().max()),
        'coords_px_max_abs_diff': float((c16 - c32).abs().max() * 256.0),
        'softargmax_px_max_abs_diff': float((soft(m16) - soft(m32)).abs().max()),
        'argmax_agreement': float((m16.flatten(2).argmax(2) == m32.flatten(2).argmax(2)).double().mean())}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--no-step', action='store_true', help='the per-class table alone')
    ap.add_argument('--s2', action='store_true', help="what precision = 'f16s2' adds to 'f16' (the stride-2 classes)")
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    if a.passes < 3:
        ap.error('--passes must be at least 3')
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'f16s2_mode_bench.json' if a.s2 else 'f16_mode_bench.json')
    os.environ.setdefault('EGONET_AMD_AUTOTUNE', '0')
    if a.s2:
        return main_s2(a)
    out = {'what': 'us per op (egn_program_run_timed, medians of %d passes, spread = max - min) of the f16-operand 3x3 op '
                   'against the fp32 op of the shipped tile table; ms per infer_crops step in both modes (medians of '
                   'alternating windows); accuracy of the mode on the device' % a.passes,
           'device': torch.cuda.get_device_name(0),
           'classes': [class_row(n, c, hw, a.passes) for n in (64, 16) for c, hw in CLASSES]}
    if not a.no_step:
        ego = _w48_ego()
        out['infer_crops_step'] = [step_row(ego, b, a.passes, a.steps) for b in (64, 16)]
        out['accuracy'] = accuracy(ego)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({'out': a.out,
                      'classes': {'%s n%d' % (r['class'], r['crops']): [round(r['fp32_us'], 1), round(r['f16_us'], 1), r['faster']]
                                  for r in out['classes']},
                      'step_ms': [[r['crops'], round(r['f32_ms_per_step'], 3), round(r['f16_ms_per_step'], 3)]
                                  for r in out.get('infer_crops_step', [])]}))
    return out


def main_s2(a):
    rows = [class_row(n, cin, hw, a.passes, cout=cout, stride=2, act=act) for n in (64, 16) for cin, cout, hw, act in S2_CLASSES]
    keep = {}
    for r in rows:
        k = r['class'].split('@')[0]
        keep[k] = keep.get(k, True) and (r['faster'] if r['crops'] == 64 else r['not_slower'])
    out = {'what': 'us per op (egn_program_run_timed, medians of %d passes, spread = max - min) of the f16-operand 3x3 '
                   'stride-2 op against the fp32 op of the shipped tile table; ms per infer_crops step in f16 and f16s2 '
                   'modes (medians of alternating windows); deviation of f16s2 from f32 on the device' % a.passes,
           'device': torch.cuda.get_device_name(0), 'classes': rows, 'keep': keep,
           'F16S2_FP32_CLASSES_measured': sorted(k for k, v in keep.items() if not v),
           'F16S2_FP32_CLASSES_shipped': [list(c) for c in engine.F16S2_FP32_CLASSES]}
    if not a.no_step:
        ego = _w48_ego()
        out['infer_crops_step'] = [step_row(ego, b, a.passes, a.steps, modes=('f16', 'f16s2')) for b in (64, 16)]
        # the 16-crop step again in a model of its own that never ran 64 crops: the small step overlaps four launch lanes
        # and its time moves by +-0.2 ms with where the programs' arenas lie, more than the two modes differ
        del ego
        torch.cuda.empty_cache()
        ego = _w48_ego()
        out['infer_crops_step_16_crops_fresh_model'] = step_row(ego, 16, a.passes, a.steps, modes=('f16', 'f16s2'))
        out['accuracy'] = accuracy(ego, mode='f16s2')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({'out': a.out, 'keep': keep,
                      'classes': {'%s n%d' % (r['class'], r['crops']): [round(r['fp32_us'], 1), round(r['fp32_spread_us'], 1),
                                                                        round(r['f16_us'], 1), round(r['f16_spread_us'], 1)]
                                  for r in rows},
                      'step_ms': [[r['crops'], round(r['f16_ms_per_step'], 3), round(r['f16s2_ms_per_step'], 3), r['f16_ops'], r['f16s2_ops']]
                                  for r in out.get('infer_crops_step', [])]}))
    return out


if __name__ == '__main__':
    main()
