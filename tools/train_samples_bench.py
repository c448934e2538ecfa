"""Training-sample front end (egonet_amd/common/train_samples.py) at the shipped batch and at 32 instances:
KITTI-sized synthetic uint8 frames (375 x 1242), the car config (256^2 input, 64^2 maps, sigma 1, jitter on).

Per configuration one JSON line ('mode': 'builder') with, as means over the timed batches:
  host_ms      the builder's host part: draws, box / affine / joint math, packing into the pinned buffer
  h2d_ms       the one staging copy (device events)
  warp_ms      egn_crop_frames_warp_normalize_u8 (device events)
  targets_ms   egn_gaussian_targets_f32 (device events)
  wall_ms      call to synchronise, one batch at a time
and beside it ('mode': 'hc_step') the native HRNet-W48 coordinates training step at the same instance count.

The A/B ('mode': 'ab'): the one multi-frame launch against per-frame launches of egn_crop_warp_normalize_u8 (what
crop_gpu.crop_boxes issues), alternated in one process on the same device-resident inputs, outputs asserted
equal; device-event time per batch of crops.

    python tools/train_samples_bench.py [--steps 20] [--warmup 3] [--configs 24x6,8x4] [--no-step]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egonet_amd import _lib, configs, synth                              # noqa: E402
from egonet_amd.common import crop_gpu, train_samples as ts              # noqa: E402

CFG = {'train': True,
       'dataset': {'pth_transform': {'mean': list(crop_gpu.IMAGENET_MEAN), 'std': list(crop_gpu.IMAGENET_STD)}},
       'heatmapModel': {'add_xy': False, 'jitter_bbox': True,
                        'jitter_params': {'shift': [0.1, 0.1], 'scaling': [0.4, 0.4]},
                        'input_size': [256, 256], 'heatmap_size': [64, 64], 'num_joints': 33,
                        'target_type': 'gaussian', 'sigma': 1}}


def bench_builder(records, steps, warmup):
    b = ts.TrainSampleBuilder(CFG)
    b.record_timings = True
    np.random.seed(0)
    rows = []
    for it in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = b(records)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ev = b.last_timings['events']
        if it >= warmup:
            rows.append([b.last_timings['host_ms'], ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]),
                         ev[2].elapsed_time(ev[3]), wall])
        del out
    m = np.mean(rows, axis=0)
    n = min(sum(len(r['boxes']) for r in records), ts.MAX_INS_CNT)
    staged_mb = sum(r['image'].nbytes for r in records) / 1e6
    return {'mode': 'builder', 'frames': len(records), 'instances': n, 'host_ms': round(m[0], 3),
            'h2d_ms': round(m[1], 3), 'warp_ms': round(m[2], 3), 'targets_ms': round(m[3], 3),
            'wall_ms': round(m[4], 3), 'wall_ms_min': round(float(np.min([r[4] for r in rows])), 3),
            'frames_mb': round(staged_mb, 2), 'crops_mb_out': round(n * 3 * 256 * 256 * 4 / 1e6, 1),
            'h2d_gb_per_s': round(staged_mb / 1e3 / (m[1] / 1e3), 1), 'steps': steps, 'warmup': warmup}


def bench_ab(records, steps, warmup):
    """The multi-frame launch against per-frame calls of the one-frame entry on identical device inputs."""
    b = ts.TrainSampleBuilder(CFG)
    np.random.seed(0)
    p = b.plan(records)
    dev = torch.device('cuda')
    frames = [torch.from_numpy(records[f]['image']).to(dev) for f in range(len(records))]
    offs = np.cumsum([0] + [f.numel() for f in frames])[:-1]
    packed = torch.cat([f.reshape(-1) for f in frames])
    tab = torch.tensor([[int(o), f.shape[0], f.shape[1], 3 * f.shape[1]] for o, f in zip(offs, frames)],
                       dtype=torch.int64, device=dev)
    order = np.argsort(p['frame'], kind='stable')           # per-frame calls need each frame's boxes together
    bf = torch.from_numpy(p['frame'][order].astype(np.int32)).to(dev)
    M = torch.from_numpy(np.ascontiguousarray(p['trans'][order].reshape(-1, 6))).to(dev)
    n = M.shape[0]
    mean_t, std_t = crop_gpu._norm_consts(b.mean, b.std, dev)
    L = _lib.lib()
    out_a = torch.empty(n, 3, 256, 256, device=dev)
    out_b = torch.empty_like(out_a)
    spans = []
    fr = p['frame'][order]
    for f in range(len(records)):
        idx = np.nonzero(fr == f)[0]
        if len(idx):
            spans.append((f, int(idx[0]), int(idx[-1]) + 1))

    def multi():
        _lib.check(L.egn_crop_frames_warp_normalize_u8(_lib.ptr(packed), _lib.ptr(tab), len(frames), _lib.ptr(bf),
                                                       _lib.ptr(M), n, 256, 256, _lib.ptr(mean_t), _lib.ptr(std_t),
                                                       _lib.ptr(out_a), _lib.current_stream()), 'multi')

    def per_frame():
        for f, a, e in spans:
            crop_gpu.crop_boxes(frames[f], None, None, (256, 256), b.mean, b.std, affines=M[a:e], out=out_b[a:e])

    times = {'multi': [], 'per_frame': []}
    for it in range(warmup + steps):
        for name, fn in (('multi', multi), ('per_frame', per_frame)) if it % 2 == 0 else \
                (('per_frame', per_frame), ('multi', multi)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1))
    assert torch.equal(out_a, out_b), 'multi-frame and per-frame crops differ'
    ma, mb = np.mean(times['multi']), np.mean(times['per_frame'])
    return {'mode': 'ab', 'frames': len(records), 'instances': n, 'multi_frame_ms': round(float(ma), 4),
            'per_frame_ms': round(float(mb), 4), 'multi_frame_ms_min': round(float(np.min(times['multi'])), 4),
            'per_frame_ms_min': round(float(np.min(times['per_frame'])), 4), 'per_frame_launches': len(spans),
            'speedup': round(float(mb / ma), 3), 'outputs_equal': True,
            'multi_frame_gb_per_s_written': round(n * 3 * 256 * 256 * 4 / 1e9 / (ma / 1e3), 1),
            'steps': steps, 'warmup': warmup}


def bench_step(n, steps, warmup):
    from egonet_amd.model.heatmapModel import hrnet
    from egonet_amd.train_hrnet import HRNetTrainStep
    cfg = configs.w48_config('coordinates')
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=1))
    net = net.cuda().train()
    tr = HRNetTrainStep(net, lr=1e-3)
    g = torch.Generator().manual_seed(100)
    x = synth.synth_crops(n, 3, 256, 256, seed=50).cuda()
    tgt = torch.rand(n, 33, 64, 64, generator=g).cuda()
    jt = torch.rand(n, 33, 2, generator=g) * 256
    for _ in range(warmup):
        tr.step(x, tgt, jt)
    torch.cuda.synchronize()
    ts_ = []
    for _ in range(steps):
        t0 = time.perf_counter()
        tr.step(x, tgt, jt)
        torch.cuda.synchronize()
        ts_.append((time.perf_counter() - t0) * 1e3)
    del tr, net
    torch.cuda.empty_cache()
    return {'mode': 'hc_step', 'model': 'W48 coordinates', 'instances': n, 'ms_per_step': round(float(np.mean(ts_)), 2),
            'ms_min': round(float(np.min(ts_)), 2), 'steps': steps, 'warmup': warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--configs', default='24x6,8x4', help='frames x boxes per frame, comma separated')
    ap.add_argument('--no-step', action='store_true', help='skip the native HC step beside the builder')
    ap.add_argument('--no-ab', action='store_true')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    os.environ.setdefault('EGONET_AMD_AUTOTUNE', '0')
    for spec in a.configs.split(','):
        nf, per = (int(v) for v in spec.split('x'))
        records = synth.synth_frame_records(nf, per, 33, seed=5)
        row = bench_builder(records, a.steps, a.warmup)
        print(json.dumps(row), flush=True)
        if not a.no_ab:
            print(json.dumps(bench_ab(records, a.steps, a.warmup)), flush=True)
        if not a.no_step:
            print(json.dumps(bench_step(row['instances'], max(3, a.steps // 4), 2)), flush=True)


if __name__ == '__main__':
    main()
