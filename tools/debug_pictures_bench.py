#!/usr/bin/env python
"""What the training debug pictures cost, stage by stage (csrc/debug_pictures.hip, egonet_amd/visualization/debug.py).

    python tools/debug_pictures_bench.py [--passes 7] [--windows 7] [--out profiles/debug_pictures_bench.json] [--no-loop]

Workloads: one report batch at the HRNet-W48 sizes (256 x 256 crops, 64 x 64 maps) with 24 and with 32 crops, and at
the Pedestrian sizes (192 x 256 crops, 48 x 64 maps) with 24 crops; J = 33; all three pictures with their markers and
joint numbers.  Medians of ``--passes`` passes after a warm-up pass, with max - min as the spread:
  kernels             hipEvents around the range, the grid and the two mosaics (five launches, no markers)
  device_route        ``save_debug_images`` on CUDA tensors up to the hand-over to the writer (range, composition,
                      arg-max and its read-back, the marker lists built on the host, one overlay launch); host clock
                      around a synchronise, the writer's copy and encoder not included
  marker_lists        of that, the host time that builds the marker and digit primitives
  host_twin           the same call on numpy arrays (the host twins and the host overlay), writer not included
  d2h_floats          crops, targets, maps and coordinates device -> host as float32: what the plain route copies first
                      (plain route = d2h_floats + host_twin)
  d2h_pictures        the finished uint8 pictures device -> pinned host in one copy
  jpeg_encode         PIL JPEG (quality 95) per picture: grid, mosaic
  loop                the HRNet-W48 training loop, 24 crops, report_every = 30: windows of 30 steps that start with a
                      report (loss read-back), pictures on and off alternating in one process; ms per window, and
                      on - off = the cost of one reported step with pictures
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from egonet_amd import _lib, configs, synth                                      # noqa: E402
from egonet_amd.visualization import debug as dbg                                # noqa: E402

J = 33
WORKLOADS = [('w48_24', 24, 256, 256, 64, 64), ('w48_32', 32, 256, 256, 64, 64), ('ped_24', 24, 256, 192, 64, 48)]


def _summary(values):
    w = [float(v) for v in values]
    return {'median': round(float(np.median(w)), 4), 'min': round(min(w), 4), 'max': round(max(w), 4),
            'spread': round(max(w) - min(w), 4), 'passes': [round(v, 4) for v in w]}


class _NoWriter(object):
    """Takes the finished pictures and drops them: times everything before the hand-over."""

    def write_device(self, block, entries):
        self.bytes = sum(3 * h * w for _, _, (h, w) in entries)
        self.block = block

    def write_host(self, pictures):
        self.pictures = pictures


def _cfgs(out, W, H):
    return {'dirs': {'output': out}, 'heatmapModel': {'input_size': [W, H]},
            'training_settings': {'debug': {'save': True, 'save_images_kpts': True, 'save_hms_gt': True,
                                            'save_hms_pred': True}}}


def workload(N, H, W, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = synth.synth_crops(N, 3, H, W, seed=seed + 1)
    centres = torch.rand(N, J, 2, generator=g) * torch.tensor([w - 1.0, h - 1.0])
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    target = torch.exp(-((xx - centres[..., 0, None, None]) ** 2 + (yy - centres[..., 1, None, None]) ** 2) / 2.0)
    maps = (target + 0.05 * torch.randn(N, J, h, w, generator=g)).contiguous()
    coords = torch.rand(N, J, 2, generator=g)
    meta = {'transformed_joints': (torch.rand(N, J, 3, generator=g) * torch.tensor([float(W), float(H), 1.0])).numpy()}
    return x, target.contiguous(), maps, coords, meta


def _timed(fn, passes, sync=True):
    fn()
    out = []
    for _ in range(passes):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return _summary(out)


def bench_stages(name, N, H, W, h, w, passes, tmp):
    x, target, maps, coords, meta = workload(N, H, W, h, w)
    d = [t.cuda() for t in (x, target, maps, coords)]
    cfgs = _cfgs(tmp, W, H)
    sink = _NoWriter()
    res = {'workload': name, 'crops': N, 'crop_hw': [H, W], 'map_hw': [h, w], 'joints': J}

    def kernels():
        lohi = dbg.image_range(d[0], 3)
        lut = dbg._LUTS.setdefault('bench', torch.from_numpy(dbg.jet_lut()).cuda())
        _, _, gh, gw = dbg.grid_layout(N, H, W)
        dbg.compose_grid(d[0], 3, lohi, torch.empty(gh, gw, 3, dtype=torch.uint8, device='cuda'))
        for m in (d[1], d[2]):
            dbg.compose_mosaic(d[0], 3, m, lohi, lut, torch.empty(N * h, (J + 1) * w, 3, dtype=torch.uint8, device='cuda'))
    kernels()
    ev = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        kernels()
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    res['kernels_ms'] = _summary(ev)
    res['device_route_ms'] = _timed(lambda: dbg.save_debug_images(1, 0, cfgs, d[0], meta, d[1], None, (d[2], d[3]), 'train',
                                                                  writer=sink), passes)
    res['picture_bytes'] = int(sink.bytes)
    res['float_bytes'] = int(sum(t.numel() * 4 for t in d))
    pred = coords.numpy() * np.array([W, H], dtype=np.float32)
    res['marker_lists_ms'] = _timed(lambda: (dbg.build_grid_markers(pred, N, H, W), dbg.build_grid_markers(
        meta['transformed_joints'], N, H, W, colour=dbg.CYAN), dbg.build_mosaic_markers(pred, h, w),
        dbg.build_mosaic_markers(pred, h, w)), passes, sync=False)
    hx = [t.numpy() for t in (x, target, maps, coords)]
    res['host_twin_ms'] = _timed(lambda: dbg.save_debug_images(1, 0, cfgs, hx[0], meta, hx[1], None, (hx[2], hx[3]),
                                                               'train', writer=sink), max(3, passes // 2), sync=False)
    res['d2h_floats_ms'] = _timed(lambda: [t.cpu() for t in d], passes)
    pinned = torch.empty(sink.block.numel(), dtype=torch.uint8, pin_memory=True)
    res['d2h_pictures_ms'] = _timed(lambda: pinned.copy_(sink.block, non_blocking=True), passes)
    res['plain_route_ms'] = round(res['d2h_floats_ms']['median'] + res['host_twin_ms']['median'], 3)
    from PIL import Image
    pics = {os.path.basename(p).split('_', 2)[2][:-4]: a for p, a in sink.pictures}
    res['jpeg_encode_ms'] = {k: dict(_timed(lambda a=a: Image.fromarray(a, 'RGB').save(io.BytesIO(), format='JPEG',
                                                                                     quality=95), passes, sync=False),
                                     shape=list(a.shape)) for k, a in pics.items() if k != 'hm_pred'}
    return res


def bench_loop(windows, report_every, tmp):
    from egonet_amd.model.heatmapModel import hrnet
    from egonet_amd.train_hrnet import HRNetTrainStep
    N, H, W, h, w = 24, 256, 256, 64, 64
    cfg = configs.w48_config('coordinates')
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=1))
    net = net.cuda().train()
    step = HRNetTrainStep(net, lr=1e-4)
    x, target, _, _, meta = workload(N, H, W, h, w)
    x, target = x.cuda(), target.cuda()
    joints = torch.from_numpy(meta['transformed_joints'][:, :, :2]).float().cuda()
    cfgs = _cfgs(tmp, W, H)
    writer = dbg.DebugPictureWriter()

    def window(on, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(report_every):
            loss = step.step(x, target, joints)
            if b == 0:                                   # the report batch, as in trainer.train
                float(loss.item())
                if on:
                    dbg.save_debug_images(k, b, cfgs, x, meta, target, None, (step.last_maps, step.last_coords),
                                          'train', writer=writer)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for on in (True, False, True, False):
        window(on, 0)
    ms = {True: [], False: []}
    for k in range(windows):
        for on in ((True, False) if k % 2 == 0 else (False, True)):
            ms[on].append(window(on, k + 1))
    t0 = time.perf_counter()
    writer.close()
    tail = (time.perf_counter() - t0) * 1e3
    on, off = _summary(ms[True]), _summary(ms[False])
    diff = on['median'] - off['median']
    return {'model': 'W48 coordinates, 24 crops of 256x256', 'report_every': report_every, 'windows': windows,
            'window_ms_pictures_on': on, 'window_ms_pictures_off': off,
            'on_minus_off_ms_per_reported_step': round(diff, 3),
            'step_ms_off': round(off['median'] / report_every, 3),
            'exceeds_spread': bool(diff > max(on['spread'], off['spread'])),
            'writer_close_wait_ms': round(tail, 3), 'reports_written': writer.reports}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--report-every', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'debug_pictures_bench.json'))
    ap.add_argument('--no-loop', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    os.environ.setdefault('EGONET_AMD_AUTOTUNE', '0')
    out = {'device': torch.cuda.get_device_name(0), 'passes': a.passes, 'stages': []}
    with tempfile.TemporaryDirectory() as tmp:
        for name, N, H, W, h, w in WORKLOADS:
            out['stages'].append(bench_stages(name, N, H, W, h, w, a.passes, tmp))
            print(json.dumps(out['stages'][-1]), flush=True)
        if not a.no_loop:
            out['loop'] = bench_loop(a.windows, a.report_every, tmp)
            loop, st = out['loop'], out['stages'][0]
            # does the background writer hide the encoder?  hidden: on - off exceeds the windows' spread by no more
            # than the pictures' D2H.  The device route before the hand-over is on the loop's path either way.
            spread = max(loop['window_ms_pictures_on']['spread'], loop['window_ms_pictures_off']['spread'])
            loop['writer_hides_encoder'] = bool(loop['on_minus_off_ms_per_reported_step'] <=
                                                spread + st['d2h_pictures_ms']['median'])
            loop['on_minus_off_minus_device_route_ms'] = round(loop['on_minus_off_ms_per_reported_step'] -
                                                               st['device_route_ms']['median'], 3)
            print(json.dumps(loop), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
    print(a.out)


if __name__ == '__main__':
    main()
