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
every map size (``keep``); the others are what engine.F16S2_FP32_CLASSES has to name.

``--x`` measures what precision = 'f16x' adds (default --out profiles/f16x_mode_bench.json): every (cin, cout, stride, map,
epilogue) class the mode lowers on HRNet-W32 at 192 x 256 (the Pedestrian model) and the seven layers it adds on HRNet-W48,
read off the recorded programs, each against the fp32 op of the shipped table at 64 and 16 crops; the Pedestrian
``infer_crops`` step in 'f32' against 'f16x' and the W48 step in 'f16s2' against 'f16x'; the deviation of 'f16x' from 'f32'
on the device for W32.  ``keep`` per (cin, cout, stride) by the rule above; the others are what engine.F16X_FP32_CLASSES
has to name.

``--a`` measures what activations = 'f16' (f16 STORAGE between two f16-operand convolutions) buys, default
--out profiles/f16_storage_bench.json.  Results cannot differ (tests/test_gpu_f16_storage_mode.py), so only time is measured:
every (producer, consumer) PAIR around a tensor ``engine.f16_storage`` names on HRNet-W48 and HRNet-W32 (192 x 256) under
'f16x', read off the recorded programs with the consumer's own epilogue, as a two-op program with the tensor in fp32 against
the same program with it in f16 -- both in one process, the order of the two alternating pass by pass, microseconds of
both ops together from ``egn_program_run_timed``, medians and spread as above, at 64 and 16 crops, beside the bytes floor at
8 TB/s.  Then the ``infer_crops`` step of both models under 'f16x' with the switch off against on (the switch-off program is
the one the parent commit records, tests/test_f16_storage_cpu.py), and the 16-crop step in a fresh model.  ``keep`` per
PRODUCER (cin, cout, stride): faster beyond the spread at 64 crops and not slower beyond it at 16 in every pair; the
others are what engine.F16_STORAGE_FP32_CLASSES has to name."""
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


def op_pair(n, cin, cout, h, w, stride, act, has_res, passes, seed, pack16, add16):
    """The fp32 op the shipped table picks for a 3x3 / pad 1 layer on an h x w INPUT map and an f16-operand op of the same
    layer (filter packed by ``pack16``, added to a program by ``add16(L, p, x, w16, scale, shift, res, y)``) as ops of ONE
    program, in either order, alternating: (cfg, fp32 us per pass, f16 us per pass, max |y16 - y32|)."""
    L = _lib.lib()
    dev = torch.device('cuda')
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(n, h, w, cin, generator=g)).cuda()
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5)
    key = (n, h, w, cin, cin, cout, cout, 3, 3, stride, 1, has_res, False)
    cfg = tuner.choose(dev, key, tuner.ALL_KINDS)
    w32 = engine.pack_for_kind(wt, tuner.kind_of(cfg)).cuda()
    w16 = pack16(wt).cuda()
    sc, sh = (torch.rand(cout, generator=g) + 0.5).cuda(), torch.randn(cout, generator=g).cuda()
    res = torch.randn(n, ho, wo, cout, generator=g).cuda()       # (bound to its slot; read only where has_res)
    y32, y16 = torch.empty_like(res), torch.empty_like(res)
    tensors = (x, w32, w16, sc, sh, res, y32, y16)
    progs = []
    for order in ((0, 1), (1, 0)):
        p = C.c_void_p(L.egn_program_create(8))
        for slot, t in enumerate(tensors):
            _lib.check(L.egn_program_bind(p, slot, _lib.ptr(t)))
        R = [_lib.Ref(s, 0) for s in range(8)]
        rref = R[5] if has_res else _lib.NULL_REF
        for which in order:
            if which == 0:
                _lib.check(L.egn_program_add_conv2d(p, R[0], R[1], R[3], R[4], rref, R[6],
                                                    n, h, w, cin, cin, cout, cout, 3, 3, stride, 1, act, 0, cfg), 'fp32 op')
            else:
                _lib.check(add16(L, p, R[0], R[2], R[3], R[4], rref, R[7]), 'f16 op')
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
    return cfg, us[0], us[1], diff


def _row(n, label, cfg, us32, us16, diff, floor):
    m32, m16 = statistics.median(us32), statistics.median(us16)
    s32, s16 = max(us32) - min(us32), max(us16) - min(us16)
    return {'crops': n, 'class': label, 'fp32_cfg': cfg, 'fp32_us': m32, 'fp32_spread_us': s32,
            'f16_us': m16, 'f16_spread_us': s16, 'fp32_all_us': us32, 'f16_all_us': us16,
            'speedup': m32 / m16, 'faster': bool(m32 - m16 > max(s32, s16)),
            'f16_activation_bytes_floor_us': floor, 'max_abs_diff_f16_vs_fp32': diff}


def class_row(n, c, hw, passes, cout=None, stride=1, act=RELU):
    """Stride 1: c -> c with residual (the default).  Stride 2: c -> cout on an hw x hw INPUT, no residual."""
    cin, c = c, (c if cout is None else cout)
    ho = (hw - 1) // stride + 1

    def add16(L, p, x, w16, sc, sh, res, y):
        if stride == 2:
            return L.egn_program_add_conv3x3s2_h(p, x, w16, sc, sh, y, n, hw, hw, cin, c, act)
        return L.egn_program_add_conv3x3_h(p, x, w16, sc, sh, res, y, n, hw, hw, c, c, engine.ACT_RELU)
    cfg, us32, us16, diff = op_pair(n, cin, c, hw, hw, stride, act, stride == 1, passes, c + n,
                                    engine.pack_conv_weight_f16, add16)
    px = float(n * hw * hw)
    # x, res, y once at 8 TB/s (stride 2: x and y)
    floor = 4.0 * (px * c * 3 if stride == 1 else px * cin + float(n * ho * ho) * c) / 8.0e12 * 1e6
    row = _row(n, '%d->%d@%dx%d' % (cin, c, hw, hw), cfg, us32, us16, diff, floor)
    if stride == 2:
        s = max(row['fp32_spread_us'], row['f16_spread_us'])
        row.update(stride=2, act=act, not_slower=bool(row['f16_us'] - row['fp32_us'] <= s))
    return row


def x_classes(cfg, n):
    """Every class precision = 'f16x' lowers to the CK = 32 instances on the model of ``cfg`` at ``n`` crops, whatever
    engine.F16X_FP32_CLASSES holds: sorted unique (cin, cout, stride, h, w, act, residual), h x w the INPUT map."""
    from egonet_amd.model.heatmapModel import hrnet
    net = hrnet.get_pose_net(cfg, is_train=False).eval()
    net.precision = 'f16x'
    iw, ih = cfg['heatmapModel']['input_size']
    shipped, engine.F16X_FP32_CLASSES = engine.F16X_FP32_CLASSES, ()
    try:
        with torch.no_grad():
            rec, _, _ = engine.HRNetEngine(net)._record(n, 3, ih, iw, None)
    finally:
        engine.F16X_FP32_CLASSES = shipped
    return sorted({(op['cin'], op['cout'], op['stride'], op['x'].h, op['x'].w, op['act'], op['res'] is not None)
                   for kind, op in rec.ops if kind == 'convhx'})


def class_row_x(n, cin, cout, stride, h, w, act, has_res, passes):
    """As ``class_row`` for the 'f16x' op on an h x w INPUT map, with the layer's own epilogue."""
    def add16(L, p, x, w16, sc, sh, res, y):
        return L.egn_program_add_conv3x3_hx(p, x, w16, sc, sh, res, y, n, h, w, cin, cout, act, stride)
    cfg, us32, us16, diff = op_pair(n, cin, cout, h, w, stride, act, has_res, passes, cin + cout + n,
                                    engine.pack_conv_weight_f16x, add16)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    # x, y (and res) once at 8 TB/s
    floor = 4.0 * (float(n * h * w) * cin + float(n * ho * wo) * cout * (2 if has_res else 1)) / 8.0e12 * 1e6
    row = _row(n, '%d->%d s%d@%dx%d' % (cin, cout, stride, h, w), cfg, us32, us16, diff, floor)
    s = max(row['fp32_spread_us'], row['f16_spread_us'])
    row.update(key=[cin, cout, stride], act=act, residual=has_res, not_slower=bool(row['f16_us'] - row['fp32_us'] <= s))
    return row


def _ped_ego():
    cfg = configs.ped_config('coordinates')
    ego = EgoNet(cfg, pre_trained=False)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=1))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=2))
    ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    return ego.eval().cuda()


def _w48_ego():
    cfg = configs.w48_config('coordinates')
    ego = EgoNet(cfg, pre_trained=False)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=1))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=2))
    ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    return ego.eval().cuda()


def step_row(ego, batch, passes, steps, modes=('f32', 'f16'), size=(256, 256), attr='precision'):
    """``size``: (height, width) of the crops.  ``attr``: the switch of ``ego.HC`` the two modes are values of."""
    crops = synth.synth_crops(batch, 3, size[0], size[1], seed=100).cuda()
    rets = [modify_bbox(b, 1.0) for b in synth.synth_boxes(batch, seed=5)]
    centers = torch.tensor(np.stack([r['c'] for r in rets]), dtype=torch.float64, device='cuda')
    scales = torch.tensor(np.stack([r['s'] for r in rets]), dtype=torch.float64, device='cuda')

    def window(prec):
        setattr(ego.HC, attr, prec)
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
    setattr(ego.HC, attr, 'f32')
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


def accuracy_x(ego):
    """precision = 'f16x' on the device: the test model of tests/f16x_mode_case.py against its fp32 CPU forward beside
    the CPU emulation's E, and HRNet-W32 at 192 x 256 on 8 crops, 'f16x' against 'f32' on the device."""
    import f16x_mode_case as case
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
            for prec in ('f32', 'f16x'):
                net.precision = prec
                row[prec] = case.deviations(case.quantities(net(x.cuda())), ref)
        row['E_cpu_emulation'] = {k: bounds[head]['forward'][k] for k in row['f16x']}
        out['test_model_%s_vs_fp32_cpu' % head] = row
    x = synth.synth_crops(8, 3, case.HEIGHT, case.WIDTH, seed=100).cuda()
    res = {}
    with torch.no_grad():
        for prec in ('f32', 'f16x'):
            ego.HC.precision = prec
            res[prec] = case.quantities(ego.HC(x))
    ego.HC.precision = 'f32'
    q32, q16 = res['f32'], res['f16x']
    m32, m16 = q32['heatmap'], q16['heatmap']
    out['w32_192x256_8_crops_f16x_vs_f32_device'] = {
        'heatmap_max_abs_diff': float((m16 - m32).abs().max()), 'heatmap_max_abs': float(m32.abs().max()),
        'coords_px_max_abs_diff': float((q16['coords_px'] - q32['coords_px']).abs().max()),
        'softargmax_px_max_abs_diff': float((q16['softargmax_px'] - q32['softargmax_px']).abs().max()),
        'argmax_agreement': float((m16.flatten(2).argmax(2) == m32.flatten(2).argmax(2)).double().mean())}
    return out


def a_pairs(cfg, n, precision='f16x'):
    """Every (producer, consumer) pair around a tensor activations = 'f16' stores as f16 on the model of ``cfg`` at ``n``
    crops, whatever engine.F16_STORAGE_FP32_CLASSES holds: sorted unique
    ((cin, cout, stride, h, w, act, ck), (cout2, stride2, act2, residual2, ck2)), h x w the producer's INPUT map."""
    from egonet_amd.model.heatmapModel import hrnet
    net = hrnet.get_pose_net(cfg, is_train=False).eval()
    net.precision = precision
    iw, ih = cfg['heatmapModel']['input_size']
    with torch.no_grad():
        rec, _, _ = engine.HRNetEngine(net)._record(n, 3, ih, iw, None)
    shipped, engine.F16_STORAGE_FP32_CLASSES = engine.F16_STORAGE_FP32_CLASSES, ()
    try:
        bufs = engine.f16_storage(rec)
    finally:
        engine.F16_STORAGE_FP32_CLASSES = shipped

    def stride_ck(kind, op):
        rule = engine._RULE_OF_KIND[kind]
        return (op['stride'] if rule.stride_arg else rule.strides[0]), rule.ck
    pairs = set()
    for kind, op in rec.ops:
        if op.get('x16'):
            (pk, prod), = [(k, o) for k, o in rec.ops if o.get('y') is op['x']]
            assert op['x'] in bufs and prod.get('y16')
            ps, pck = stride_ck(pk, prod)
            cs_, cck = stride_ck(kind, op)
            pairs.add(((prod['cin'], prod['cout'], ps, prod['x'].h, prod['x'].w, prod['act'], pck),
                       (op['cout'], cs_, op['act'], op.get('res') is not None, cck)))
    return sorted(pairs)


def pair_row(n, prod, cons, passes):
    """Producer + consumer as a two-op program, the tensor between them in fp32 against f16 (both through
    egn_program_add_conv3x3_h16, flags 0 / 1): us of both ops together per pass, the two programs in alternating order."""
    L = _lib.lib()
    cin, cmid, s1, h, w, act1, ck1 = prod
    cout, s2, act2, has_res, ck2 = cons
    h1, w1 = (h - 1) // s1 + 1, (w - 1) // s1 + 1
    h2, w2 = (h1 - 1) // s2 + 1, (w1 - 1) // s2 + 1
    g = torch.Generator().manual_seed(cin + cmid + cout + n)
    x = torch.relu(torch.randn(n, h, w, cin, generator=g)).cuda()

    def filt(co, ci, ck):
        wt = torch.randn(co, ci, 3, 3, generator=g) / (3.0 * ci ** 0.5)
        return (engine.pack_conv_weight_f16x if ck == 32 else engine.pack_conv_weight_f16)(wt).cuda()
    wa, wb = filt(cmid, cin, ck1), filt(cout, cmid, ck2)
    sa, ha = (torch.rand(cmid, generator=g) + 0.5).cuda(), torch.randn(cmid, generator=g).cuda()
    sb, hb = (torch.rand(cout, generator=g) + 0.5).cuda(), torch.randn(cout, generator=g).cuda()
    # the consumer's residual: the block's own input where the shapes agree (a BasicBlock), else a tensor of its own
    res = x if has_res and tuple(x.shape) == (n, h2, w2, cout) else torch.randn(n, h2, w2, cout, generator=g).cuda()
    mids = {0: torch.empty(n, h1, w1, cmid, device='cuda'), 1: torch.empty(n, h1, w1, cmid, device='cuda', dtype=torch.float16)}
    ys = {0: torch.empty(n, h2, w2, cout, device='cuda'), 1: torch.empty(n, h2, w2, cout, device='cuda')}
    progs = {}
    for f16 in (0, 1):
        p = C.c_void_p(L.egn_program_create(12))
        tensors = (x, wa, sa, ha, mids[f16], wb, sb, hb, res, ys[f16])
        for slot, t in enumerate(tensors):
            _lib.check(L.egn_program_bind(p, slot, _lib.ptr(t)))
        R = [_lib.Ref(k, 0) for k in range(len(tensors))]
        _lib.check(L.egn_program_add_conv3x3_h16(p, R[0], R[1], R[2], R[3], _lib.NULL_REF, R[4], n, h, w, cin, cmid, act1, s1,
                                                 ck1, 0, f16), 'producer')
        _lib.check(L.egn_program_add_conv3x3_h16(p, R[4], R[5], R[6], R[7], R[8] if has_res else _lib.NULL_REF, R[9], n, h1, w1,
                                                 cmid, cout, act2, s2, ck2, f16, 0), 'consumer')
        progs[f16] = p
    st = _lib.current_stream()
    us = {0: [], 1: []}
    ops = {0: [], 1: []}
    ms = (C.c_float * 2)()
    try:
        for it in range(2 + passes):
            for f16 in ((0, 1) if it % 2 == 0 else (1, 0)):
                _lib.check(L.egn_program_run_timed(progs[f16], st, ms, 2))
                if it >= 2:
                    us[f16].append((ms[0] + ms[1]) * 1e3)
                    ops[f16].append([ms[0] * 1e3, ms[1] * 1e3])
        torch.cuda.synchronize()
        same = bool(torch.equal(ys[0], ys[1]))
    finally:
        for p in progs.values():
            L.egn_program_destroy(p)
    m32, m16 = statistics.median(us[0]), statistics.median(us[1])
    s32, s16 = max(us[0]) - min(us[0]), max(us[1]) - min(us[1])
    spread = max(s32, s16)
    px0, px1, px2 = float(n * h * w), float(n * h1 * w1), float(n * h2 * w2)
    fixed = 4.0 * (px0 * cin + px2 * cout * (2 if has_res else 1))
    return {'crops': n, 'class': '%d->%d s%d@%dx%d -> %d s%d%s' % (cin, cmid, s1, h, w, cout, s2, ' +res' if has_res else ''),
            'producer_key': [cin, cmid, s1], 'consumer': [cmid, cout, s2, act2, has_res],
            'f32_storage_us': m32, 'f32_storage_spread_us': s32, 'f16_storage_us': m16, 'f16_storage_spread_us': s16,
            'f32_storage_all_us': us[0], 'f16_storage_all_us': us[1],
            'f32_storage_ops_us': [statistics.median(o[k] for o in ops[0]) for k in (0, 1)],
            'f16_storage_ops_us': [statistics.median(o[k] for o in ops[1]) for k in (0, 1)],
            'speedup': m32 / m16, 'faster': bool(m32 - m16 > spread), 'not_slower': bool(m16 - m32 <= spread),
            'bytes_floor_us': [(fixed + 8.0 * px1 * cmid) / 8.0e12 * 1e6, (fixed + 4.0 * px1 * cmid) / 8.0e12 * 1e6],
            'outputs_bit_identical': same}


def main_a(a):
    rows = []
    for n in (64, 16) if not a.no_pairs else ():
        ped = a_pairs(configs.ped_config('coordinates'), n)
        w48 = [c for c in a_pairs(configs.w48_config('coordinates'), n) if c not in ped]
        for model, pairs in (('w32_192x256', ped), ('w48_256x256', w48)):
            for prod, cons in pairs:
                rows.append(dict(pair_row(n, prod, cons, a.passes), model=model))
    keep = {}
    for r in rows:
        k = '%d->%d s%d' % tuple(r['producer_key'])
        keep[k] = keep.get(k, True) and (r['faster'] if r['crops'] == 64 else r['not_slower'])
    out = {'what': 'us of a producer + consumer pair of f16-operand 3x3 ops (egn_program_run_timed, both ops together, medians '
                   'of %d passes, spread = max - min) with the tensor between them stored as fp32 against f16; ms per '
                   'infer_crops step of HRNet-W48 and HRNet-W32 (192 x 256) under f16x with activations f32 against f16 '
                   '(medians of alternating windows)' % a.passes,
           'device': torch.cuda.get_device_name(0), 'pairs': rows, 'keep': keep,
           'all_outputs_bit_identical': all(r['outputs_bit_identical'] for r in rows),
           'F16_STORAGE_FP32_CLASSES_measured': sorted(k for k, v in keep.items() if not v),
           'F16_STORAGE_FP32_CLASSES_shipped': [list(c) for c in engine.F16_STORAGE_FP32_CLASSES]}
    if not a.no_step:
        for name, mk, size in (('w48', _w48_ego, (256, 256)), ('w32', _ped_ego, (256, 192))):
            ego = mk()
            ego.HC.precision = 'f16x'
            out[name + '_infer_crops_step'] = [step_row(ego, b, a.passes, a.steps, size=size, attr='activations')
                                               for b in (64, 16)]
            # the 16-crop step again in a model of its own that never ran 64 crops (as --s2 / --x: its time moves with
            # where the programs' arenas lie)
            del ego
            torch.cuda.empty_cache()
            ego = mk()
            ego.HC.precision = 'f16x'
            out[name + '_infer_crops_step_16_crops_fresh_model'] = step_row(ego, 16, a.passes, a.steps, size=size,
                                                                            attr='activations')
            del ego
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    steps = {k: v if isinstance(v, list) else [v] for k, v in out.items() if 'infer_crops_step' in k}
    print(json.dumps({'out': a.out, 'keep': keep, 'bit_identical': out['all_outputs_bit_identical'],
                      'pairs': {'%s n%d' % (r['class'], r['crops']): [round(r['f32_storage_us'], 1), round(r['f32_storage_spread_us'], 1),
                                                                      round(r['f16_storage_us'], 1), round(r['f16_storage_spread_us'], 1)]
                                for r in rows},
                      'step_ms': {k: [[r['crops'], round(r['f32_ms_per_step'], 3), round(r['f16_ms_per_step'], 3)] for r in v]
                                  for k, v in steps.items()}}))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--no-step', action='store_true', help='the per-class table alone')
    ap.add_argument('--s2', action='store_true', help="what precision = 'f16s2' adds to 'f16' (the stride-2 classes)")
    ap.add_argument('--x', action='store_true', help="what precision = 'f16x' adds (the 32-multiple widths)")
    ap.add_argument('--no-pairs', action='store_true', help='with --a: the steps alone (under the shipped exception tuple)')
    ap.add_argument('--a', action='store_true', help="what activations = 'f16' buys (f16 storage between f16-operand convs)")
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    if a.passes < 3:
        ap.error('--passes must be at least 3')
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'f16_storage_bench.json' if a.a else 'f16x_mode_bench.json' if a.x else
                             ('f16s2_mode_bench.json' if a.s2 else 'f16_mode_bench.json'))
    os.environ.setdefault('EGONET_AMD_AUTOTUNE', '0')
    if a.a:
        return main_a(a)
    if a.x:
        return main_x(a)
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


def main_x(a):
    rows = []
    for n in (64, 16):
        ped = x_classes(configs.ped_config('coordinates'), n)
        w48 = [c for c in x_classes(configs.w48_config('coordinates'), n) if c not in ped]
        for model, classes in (('w32_192x256', ped), ('w48_256x256', w48)):
            for cin, cout, stride, h, w, act, has_res in classes:
                rows.append(dict(class_row_x(n, cin, cout, stride, h, w, act, has_res, a.passes), model=model))
    keep = {}
    for r in rows:
        k = '%d->%d s%d' % tuple(r['key'])
        keep[k] = keep.get(k, True) and (r['faster'] if r['crops'] == 64 else r['not_slower'])
    out = {'what': 'us per op (egn_program_run_timed, medians of %d passes, spread = max - min) of the f16-operand 3x3 op '
                   'on chunks of 32 against the fp32 op of the shipped tile table; ms per infer_crops step of HRNet-W32 at '
                   '192 x 256 in f32 and f16x modes and of HRNet-W48 in f16s2 and f16x modes (medians of alternating '
                   'windows); deviation of f16x from f32 on the device' % a.passes,
           'device': torch.cuda.get_device_name(0), 'classes': rows, 'keep': keep,
           'F16X_FP32_CLASSES_measured': sorted(k for k, v in keep.items() if not v),
           'F16X_FP32_CLASSES_shipped': [list(c) for c in engine.F16X_FP32_CLASSES]}
    if not a.no_step:
        ego = _ped_ego()
        out['w32_infer_crops_step'] = [step_row(ego, b, a.passes, a.steps, modes=('f32', 'f16x'), size=(256, 192))
                                       for b in (64, 16)]
        out['accuracy'] = accuracy_x(ego)
        del ego
        torch.cuda.empty_cache()
        ego = _w48_ego()
        out['w48_infer_crops_step'] = [step_row(ego, b, a.passes, a.steps, modes=('f16s2', 'f16x')) for b in (64, 16)]
        # the 16-crop step again in a model of its own that never ran 64 crops (as --s2: its time moves with where the
        # programs' arenas lie)
        del ego
        torch.cuda.empty_cache()
        ego = _w48_ego()
        out['w48_infer_crops_step_16_crops_fresh_model'] = step_row(ego, 16, a.passes, a.steps, modes=('f16s2', 'f16x'))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({'out': a.out, 'keep': keep,
                      'classes': {'%s n%d' % (r['class'], r['crops']): [round(r['fp32_us'], 1), round(r['fp32_spread_us'], 1),
                                                                        round(r['f16_us'], 1), round(r['f16_spread_us'], 1)]
                                  for r in rows},
                      'w32_step_ms': [[r['crops'], round(r['f32_ms_per_step'], 3), round(r['f16x_ms_per_step'], 3), r['f16x_ops']]
                                      for r in out.get('w32_infer_crops_step', [])],
                      'w48_step_ms': [[r['crops'], round(r['f16s2_ms_per_step'], 3), round(r['f16x_ms_per_step'], 3),
                                       r['f16s2_ops'], r['f16x_ops']] for r in out.get('w48_infer_crops_step', []) +
                                      [out[k] for k in ('w48_infer_crops_step_16_crops_fresh_model',) if k in out]]}))
    return out


if __name__ == '__main__':
    main()
