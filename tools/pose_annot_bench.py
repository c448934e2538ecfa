#!/usr/bin/env python
"""Measure the 2-D pose annotation build (egonet_amd.common.pose_annot) and write profiles/pose_annot_bench.json.

    python tools/pose_annot_bench.py [--frames 7481] [--per-frame 4] [--out profiles/pose_annot_bench.json]

A synthetic label set of KITTI's size (7 481 training frames, about 4 cars each; parsing excluded: the labels are
seeded arrays).  After a warm-up, the median of ``--runs`` runs of
  device_launch_ms   ``egn_pose2d_annot_f64`` alone between device events (inputs uploaded, outputs allocated;
                     ``--inner`` calls per run, so that a run is longer than the events' resolution),
  device_build_ms    ``build_device``: upload, the launches, the read-back of the totals and of every output -- a host
                     clock around work that ends in a synchronising copy,
  host_build_ms      ``build_host``, the numpy float64 path of the same commit, on the same arrays.
The build runs once per training run; the numbers say what it costs, not that it matters."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egonet_amd import _lib, synth                          # noqa: E402
from egonet_amd.common import lifter_pairs as lp            # noqa: E402
from egonet_amd.common import pose_annot as pa              # noqa: E402


def label_set(frames, per_frame, seed=1):
    records = synth.synth_kitti_labels(frames * per_frame, seed=seed, per_frame=per_frame)
    labels = np.concatenate([r['labels'] for r in records])
    lf = np.repeat(np.arange(len(records), dtype=np.int32), [len(r['labels']) for r in records])
    table = np.stack([lp.frame_row(r['P'], r['size']) for r in records])
    alpha = np.random.RandomState(seed).uniform(-np.pi, np.pi, len(labels))
    return labels, alpha, lf, table


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=7481)
    ap.add_argument('--per-frame', type=int, default=4)
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=os.path.join('profiles', 'pose_annot_bench.json'))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('pose_annot_bench: no GPU visible; nothing is measured without one')
    _lib.lib()
    cfg = {'dataset': {'interpolate': {'flag': True, 'style': 'bbox12', 'coef': [0.332, 0.667]}}}
    dev, host = pa.PoseAnnotBuilder(cfg), pa.PoseAnnotBuilder(cfg, device='cpu')
    case = label_set(a.frames, a.per_frame)
    want = host.build_host(*case)
    got = dev.build_device(*case)                           # warm-up: code objects, allocator; and the same result
    same = all(np.array_equal(got[k], want[k]) for k in ('totals', 'boxes', 'src', 'frame_raw', 'frame_kept'))
    worst = float(np.abs(got['kpts'] - want['kpts']).max())
    up = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in case]
    ws = torch.empty(_lib.lib().egn_pose2d_annot_ws_bytes(len(case[0])), dtype=torch.uint8, device='cuda')
    dev.launch(*up, ws=ws)
    torch.cuda.synchronize()
    launch_ms, build_ms, host_ms = [], [], []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            out = dev.launch(*up, ws=ws)
        e1.record()
        torch.cuda.synchronize()
        launch_ms.append(e0.elapsed_time(e1) / a.inner)
        del out
        t0 = time.perf_counter()
        dev.build_device(*case)
        build_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        host.build_host(*case)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    result = {'device': torch.cuda.get_device_name(0), 'frames': a.frames, 'labels': int(len(case[0])),
              'kept_inlier': int(want['totals'][0]), 'kept_visible': int(want['totals'][1]),
              'runs': a.runs, 'inner_launches_per_run': a.inner,
              'device_launch_ms': float(np.median(launch_ms)), 'device_launch_ms_all': launch_ms,
              'device_build_ms': float(np.median(build_ms)), 'device_build_ms_all': build_ms,
              'host_build_ms': float(np.median(host_ms)), 'host_build_ms_all': host_ms,
              'integer_outputs_equal_host': bool(same), 'largest_kpt_difference_px': worst}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(result, sort_keys=True))
    return result


if __name__ == '__main__':
    main()
