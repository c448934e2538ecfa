#!/usr/bin/env python
"""Cold start and steady state of an inference plan against the model it was exported from -> profiles/plan_bench.json.

    python tools/plan_bench.py [--batch 64] [--windows 9] [--steps 10] [--out profiles/plan_bench.json]

HRNet-W48 (coordinate head), seeded synthetic weights, ``--batch`` crops:
  cold start   two FRESH child processes, one after the other, each timed from its first line to its first finished
               ``infer_crops`` (results on the host):
                 (A) model  import, build ``EgoNet``, move it to the GPU, infer -- the engine records, plans, packs ~300
                            filters on the host and builds its programs inside that first call;
                 (B) plan   import, ``Plan(path).load()``, infer.
               The phases of each are reported beside the totals.  Cold start has no bar: it is reported.
  steady state one process, both paths interleaved window by window (``--steps`` calls with the results left on the
               device, one synchronisation per window), the median window of each and the spread (max - min) of its
               windows.  The plan issues the launches of the model's programs: its step must not be slower than the
               model's by more than that spread (``steady_ok``).
"""
import time
T0 = time.time()          # (before the heavy imports: a cold start includes them)

import argparse           # noqa: E402
import json               # noqa: E402
import os                 # noqa: E402
import subprocess         # noqa: E402
import sys                # noqa: E402
import tempfile           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = [[707.0493, 0., 604.0814], [0., 707.0493, 180.5066], [0., 0., 1.]]


def inputs(n):
    import numpy as np
    from egonet_amd import synth
    from egonet_amd.common.img_proc import modify_bbox
    crops = synth.synth_crops(n, 3, 256, 256, seed=8)
    rets = [modify_bbox(b, 1.0) for b in synth.synth_boxes(n, seed=2)]
    return crops, np.stack([r['c'] for r in rets]), np.stack([r['s'] for r in rets]), np.array(K)


def build_model():
    from egonet_amd import configs, synth
    from egonet_amd.model.egonet import EgoNet
    ego = EgoNet(configs.w48_config('coordinates'), pre_trained=False)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=6))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=7))
    ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    return ego.eval()


def child(which, plan_path, batch):
    """One cold start; prints one JSON line with the seconds since the process' first line at the end of each phase."""
    import torch
    import zlib
    phases = {'imports': time.time() - T0}
    crops, c, s, Kn = inputs(batch)
    crops = crops.cuda()
    torch.cuda.synchronize()
    phases['inputs_on_gpu'] = time.time() - T0
    if which == 'model':
        runner = build_model().cuda()
        phases['model_built'] = time.time() - T0
    else:
        from egonet_amd import plan
        runner = plan.Plan(plan_path)
        phases['plan_opened'] = time.time() - T0
        runner.load('cuda:0')
        phases['plan_loaded'] = time.time() - T0
    res = runner.infer_crops(crops, c, s, K=Kn)
    phases['first_infer_done'] = time.time() - T0
    print(json.dumps({'which': which, 'seconds': phases, 'kpts_3d_crc': zlib.crc32(res['kpts_3d'].tobytes())}), flush=True)


def run_child(which, plan_path, batch):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', which, '--plan', plan_path, '--batch', str(batch)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0:
        raise RuntimeError('%s child failed (%d): %s' % (which, r.returncode, r.stderr.decode()[-2000:]))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'plan_bench.json'))
    ap.add_argument('--child', choices=('model', 'plan'), default=None)
    ap.add_argument('--plan', default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.plan, args.batch)
    import numpy as np
    import torch
    from egonet_amd import plan
    ego = build_model().cuda()
    crops, c, s, Kn = inputs(args.batch)
    crops = crops.cuda()
    tmp = tempfile.mkdtemp(prefix='plan_bench_')
    path = os.path.join(tmp, 'w48.egnplan')
    t = time.time()
    plan.export_plan(ego, path, batch_sizes=(args.batch,))
    export_s = time.time() - t
    P = plan.Plan(path).load('cuda:0')
    want = ego.infer_crops(crops, c, s, K=Kn)
    got = P.infer_crops(crops, c, s, K=Kn)
    same = all(got[k].tobytes() == want[k].tobytes() for k in want)
    c_d = torch.as_tensor(c).cuda()
    s_d = torch.as_tensor(s).cuda()
    runners = {'model': lambda: ego.infer_crops(crops, c_d, s_d, K=Kn, to_host=False),
               'plan': lambda: P.infer_crops(crops, c_d, s_d, K=Kn, to_host=False)}
    for fn in runners.values():          # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runners}
    for _ in range(args.windows):
        for name, fn in runners.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t) * 1e3 / args.steps)
    steady = {k: {'median_ms': float(np.median(v)), 'spread_ms': float(max(v) - min(v)), 'windows_ms': [round(x, 4) for x in v]}
              for k, v in ms.items()}
    spread = max(steady['model']['spread_ms'], steady['plan']['spread_ms'])
    P.close()
    del ego
    torch.cuda.empty_cache()
    cold = {which: run_child(which, path, args.batch) for which in ('model', 'plan')}
    result = {
        'what': 'HRNet-W48 coordinate head, %d crops: EgoNet.infer_crops against Plan.infer_crops of its exported plan' % args.batch,
        'batch': args.batch, 'plan_bytes': os.path.getsize(path), 'export_seconds': round(export_s, 3),
        'outputs_bit_identical': bool(same and cold['model']['kpts_3d_crc'] == cold['plan']['kpts_3d_crc']),
        'cold_start_seconds': {k: round(v['seconds']['first_infer_done'], 3) for k, v in cold.items()},
        'cold_start_phases': {k: {p: round(t, 3) for p, t in v['seconds'].items()} for k, v in cold.items()},
        'steady_state': steady,
        'steady_ok': bool(steady['plan']['median_ms'] - steady['model']['median_ms'] <= spread),
    }
    os.remove(path)
    os.rmdir(tmp)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps({k: result[k] for k in ('cold_start_seconds', 'steady_ok', 'outputs_bit_identical')}))
    print(json.dumps({k: (v['median_ms'], v['spread_ms']) for k, v in steady.items()}))


if __name__ == '__main__':
    main()
