#!/usr/bin/env python
"""What drawing predictions on the frames costs, stage by stage (csrc/overlay.hip, egonet_amd/visualization).

    python tools/overlay_bench.py [--passes 7] [--reps 20] [--out profiles/overlay_bench.json] [--no-step]

Workload: 8 frames of 375 x 1242 with 10 instances each, 49 primitives per instance (a 2-D box, 12 cuboid edges, 33
key-point discs: build_primitives on seeded records), anti-aliased.  Medians of ``--passes`` passes after a warm-up
pass, with max - min as the spread:
  launch_cull / launch_nocull   hipEvents around ``--reps`` launches on frames already in HBM, the two variants
                                alternating inside every pass (cull = 0 sends every primitive to every tile)
  host_twin                     the same overlay_math.h as a plain loop on the host, all 8 frames (host clock)
  pil_imagedraw                 PIL ImageDraw.line / .ellipse on the same segments and discs, all 8 frames: what one
                                would do without the kernel.  It does NOT anti-alias and rounds end points to pixels,
                                so it does less work and draws a different (jagged) picture
  upload_readback               the 8 frames pinned host -> device and back, one copy each way (host clock around
                                a synchronise)
  png_encode_per_frame          PIL's PNG encoder on one drawn frame (what --draw does per picture)
  infer_crops_step              the 64-crop HRNet-W48 step of bench.py, for scale
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from egonet_amd import _lib, configs, synth                                      # noqa: E402
from egonet_amd.common.img_proc import modify_bbox                               # noqa: E402
from egonet_amd.model.egonet import EgoNet                                       # noqa: E402
from egonet_amd.visualization import OverlayRenderer, build_primitives           # noqa: E402

H, W, FRAMES, INSTANCES, J = 375, 1242, 8, 10, 33


def workload(seed=0):
    rs = np.random.RandomState(seed)
    # photo-like frames for the PNG encoder: smooth ramps plus a few grey levels of noise (pure noise does not compress)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([(xx * 255 // W), (yy * 255 // H), ((xx + yy) * 255 // (H + W))], -1)
    frames = [np.clip(ramp + rs.randint(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8) for _ in range(FRAMES)]
    prims, colors, ranges, n = [], [], [], 0
    for _ in range(FRAMES):
        rec = {'bbox_resize': [], 'kpts_2d_pred': []}
        for _ in range(INSTANCES):
            bw, bh = rs.uniform(60, 300), rs.uniform(40, 160)
            x1, y1 = rs.uniform(0, W - bw), rs.uniform(100, H - bh)
            rec['bbox_resize'].append(np.array([x1, y1, x1 + bw, y1 + bh]))
            rec['kpts_2d_pred'].append((np.array([x1, y1]) + rs.uniform(0, 1, (J, 2)) * (bw, bh)).reshape(1, -1))
        p, c = build_primitives(rec)
        assert len(p) == INSTANCES * 49
        prims.append(p)
        colors.append(c)
        ranges.append((n, n + len(p)))
        n += len(p)
    return frames, np.concatenate(prims), np.concatenate(colors), ranges


def summary(vals, unit):
    return {'median_' + unit: statistics.median(vals), 'spread_' + unit: max(vals) - min(vals), 'all_' + unit: vals}


def launches(frames, prims, colors, ranges, passes, reps):
    L = _lib.lib()
    d_frames = torch.from_numpy(np.stack(frames)).cuda()
    tab = np.array([(i * H * W * 3, H, W, 3 * W, b, e) for i, (b, e) in enumerate(ranges)], dtype=np.int64)
    d_tab, d_pr = torch.from_numpy(tab).cuda(), torch.from_numpy(prims).cuda()
    d_col = torch.from_numpy(colors.view(np.int32)).cuda()
    stream = _lib.current_stream()

    def run(cull):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            _lib.check(L.egn_overlay_draw_u8(_lib.ptr(d_frames), _lib.ptr(d_tab), FRAMES, H, W, _lib.ptr(d_pr),
                                             _lib.ptr(d_col), len(colors), 1, cull, stream), 'overlay_draw')
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    cull, nocull = [], []
    for p in range(passes + 1):
        a, b = run(1), run(0)
        if p:
            cull.append(a)
            nocull.append(b)
    # the two variants and the host twin give the same bytes at this size
    fresh = torch.from_numpy(np.stack(frames))
    got = []
    for c in (1, 0):
        d_frames.copy_(fresh)
        _lib.check(L.egn_overlay_draw_u8(_lib.ptr(d_frames), _lib.ptr(d_tab), FRAMES, H, W, _lib.ptr(d_pr),
                                         _lib.ptr(d_col), len(colors), 1, c, stream), 'overlay_draw')
        got.append(d_frames.cpu().numpy())
    return cull, nocull, got


def host_twin(frames, prims, colors, ranges, passes):
    r = OverlayRenderer('cpu')
    ms = []
    for p in range(passes + 1):
        t0 = time.perf_counter()
        out = r.draw(frames, prims, colors, ranges)
        if p:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, np.stack(out)


def pil_draw(frames, prims, colors, ranges, passes):
    from PIL import Image, ImageDraw
    ms = []
    for p in range(passes + 1):
        imgs = [Image.fromarray(f) for f in frames]
        t0 = time.perf_counter()
        for im, (b, e) in zip(imgs, ranges):
            d = ImageDraw.Draw(im)
            for (x0, y0, x1, y1, r, _), c in zip(prims[b:e].tolist(), colors[b:e].tolist()):
                col = (c & 255, (c >> 8) & 255, (c >> 16) & 255)
                if x0 == x1 and y0 == y1:
                    d.ellipse((x0 - r, y0 - r, x0 + r, y0 + r), fill=col)
                else:
                    d.line((x0, y0, x1, y1), fill=col, width=int(round(2 * r)))
        if p:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def copies(frames, passes):
    pinned = torch.from_numpy(np.stack(frames)).pin_memory()
    back = torch.empty_like(pinned).pin_memory()
    dev = torch.empty_like(pinned, device='cuda')
    ms = []
    for p in range(passes + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.copy_(pinned, non_blocking=True)
        back.copy_(dev, non_blocking=True)
        torch.cuda.synchronize()
        if p:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def png(frame, passes):
    from PIL import Image
    ms, size = [], 0
    for p in range(passes + 1):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        Image.fromarray(frame).save(buf, format='PNG')
        if p:
            ms.append((time.perf_counter() - t0) * 1e3)
        size = buf.tell()
    return ms, size


def infer_step(passes, steps, batch=64):
    ego = EgoNet(configs.w48_config('coordinates'), pre_trained=False)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=1))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=2))
    ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    ego = ego.eval().cuda()
    crops = synth.synth_crops(batch, 3, 256, 256, seed=100).cuda()
    rets = [modify_bbox(b, 1.0) for b in synth.synth_boxes(batch, seed=5)]
    centers = torch.tensor(np.stack([r['c'] for r in rets]), dtype=torch.float64, device='cuda')
    scales = torch.tensor(np.stack([r['s'] for r in rets]), dtype=torch.float64, device='cuda')
    ms = []
    for p in range(passes + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            ego.infer_crops(crops, centers, scales, decode='coords', to_host=False)
        torch.cuda.synchronize()
        if p:
            ms.append((time.perf_counter() - t0) * 1e3 / steps)
    return ms


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--no-step', action='store_true', help='without the HRNet-W48 step')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'overlay_bench.json'))
    a = ap.parse_args(argv)
    if a.passes < 3:
        ap.error('--passes must be at least 3')
    if not torch.cuda.is_available():
        raise SystemExit('overlay_bench needs a GPU: nothing here is measured without one')
    os.environ.setdefault('EGONET_AMD_AUTOTUNE', '0')
    frames, prims, colors, ranges = workload()
    cull, nocull, got = launches(frames, prims, colors, ranges, a.passes, a.reps)
    twin_ms, twin = host_twin(frames, prims, colors, ranges, a.passes)
    png_ms, png_bytes = png(twin[0], a.passes)
    out = {
        'what': '%d frames of %d x %d, %d instances each, %d primitives in all, anti-aliased; medians of %d passes, '
                'spread = max - min; launches: hipEvents around %d launches' % (FRAMES, H, W, INSTANCES, len(prims),
                                                                                  a.passes, a.reps),
        'tile_capacity': _lib.lib().egn_overlay_tile_capacity(),
        'launch_cull': summary(cull, 'us'), 'launch_nocull': summary(nocull, 'us'),
        'device_equals_host_twin': bool(np.array_equal(got[0], twin)),
        'cull_equals_nocull': bool(np.array_equal(got[0], got[1])),
        'pixels_changed': int((twin != np.stack(frames)).any(-1).sum()),
        'host_twin': summary(twin_ms, 'ms'),
        'pil_imagedraw': dict(summary(pil_draw(frames, prims, colors, ranges, a.passes), 'ms'),
                              note='no anti-aliasing, end points rounded to pixels'),
        'upload_readback': summary(copies(frames, a.passes), 'ms'),
        'png_encode_per_frame': dict(summary(png_ms, 'ms'), bytes=png_bytes),
    }
    if not a.no_step:
        out['infer_crops_step_64'] = summary(infer_step(a.passes, a.steps), 'ms')
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps({k: (round(v[[m for m in v if m.startswith('median')][0]], 3) if isinstance(v, dict) else v)
                      for k, v in out.items() if k != 'what'}))
    return out


if __name__ == '__main__':
    main()
