#!/usr/bin/env python
"""Write an inference plan (egonet_amd/plan.py): the planned, tuned and packed network of EgoNet.infer_crops as one file
that ``egonet_amd.plan.Plan`` and tools/_build/egonet_run (no Python) run.

    python tools/export_plan.py --out w48.egnplan                          # HRNet-W48, seeded synthetic weights
    python tools/export_plan.py --ckpt <dir with HC.pth, L.pth, LS.npy> --out car.egnplan
    python tools/export_plan.py --model tiny --sizes 1,4 --out tiny.egnplan --case tiny.case --case-n 5

Without a visible GPU the export takes the shipped table's tile choices (or the cost model's) and never measures.
``--case``: also write a case file of synthetic crops and boxes for egonet_run.
"""
import argparse
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_case(path, crops, centers, scales, K=None, alpha_mode='proj'):
    """The case file tools/egonet_run.cpp reads: crops [n,C,H,W] fp32, centers / scales [n,2] f64, K [3,3] or None."""
    crops = np.ascontiguousarray(crops, dtype='<f4')
    n, c, h, w = crops.shape
    fx, cx = (float(K[0][0]), float(K[0][2])) if K is not None else (1.0, 0.0)
    with open(path, 'wb') as f:
        f.write(b'EGNCASE\0' + struct.pack('<6I2d', n, c, h, w, int(K is not None), 0 if alpha_mode == 'proj' else 1, fx, cx))
        f.write(crops.tobytes())
        f.write(np.ascontiguousarray(centers, dtype='<f8').reshape(n, 2).tobytes())
        f.write(np.ascontiguousarray(scales, dtype='<f8').reshape(n, 2).tobytes())
    return path


def read_outputs(out_dir, n, J, D):
    """What egonet_run wrote, as infer_crops' dictionary."""
    def arr(name, dtype, shape):
        return np.fromfile(os.path.join(out_dir, name), dtype=dtype).reshape(shape)
    res = {'local': arr('local.f32', '<f4', (n, J, 2)), 'kpts_2d': arr('kpts_2d.f64', '<f8', (n, 2 * J)),
           'kpts_3d': arr('kpts_3d.f64', '<f8', (n, -1, 3))}
    if D == 96:
        res.update(euler=arr('euler.f64', '<f8', (n, 3)), alpha=arr('alpha.f64', '<f8', (n,)),
                   translation=res['kpts_3d'][:, 0, :])
    return res


def build_model(args):
    import torch
    from egonet_amd import configs, synth
    from egonet_amd.model.egonet import EgoNet
    cfg = {'w48': configs.w48_config, 'ped': configs.ped_config,
           'tiny': lambda head: configs.tiny_config(head, num_joints=33)}[args.model](args.head)
    if args.ckpt:
        cfg['dirs'] = {'ckpt': args.ckpt}
    ego = EgoNet(cfg, pre_trained=bool(args.ckpt), precision=args.precision)
    if not args.ckpt:
        ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=args.seed))
        ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=args.seed + 1))
        ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    ego = ego.eval()
    return ego.cuda() if torch.cuda.is_available() and not args.cpu else ego


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', required=True)
    ap.add_argument('--model', choices=('w48', 'ped', 'tiny'), default='w48')
    ap.add_argument('--head', choices=('coordinates', 'heatmap'), default='coordinates')
    ap.add_argument('--decode', choices=('auto', 'coords', 'soft', 'hard'), default='auto')
    ap.add_argument('--precision', choices=('f32', 'f16', 'f16s2', 'f16x'), default=None)
    ap.add_argument('--ckpt', default=None, help='directory with HC.pth, L.pth and LS.npy (default: seeded synthetic weights)')
    ap.add_argument('--seed', type=int, default=6)
    ap.add_argument('--sizes', default='1,2,4,8,16,32,64')
    ap.add_argument('--cpu', action='store_true', help='export without touching a GPU even if one is visible')
    ap.add_argument('--case', default=None, help='also write a case file for tools/_build/egonet_run')
    ap.add_argument('--case-n', type=int, default=4)
    args = ap.parse_args(argv)
    from egonet_amd import plan, synth
    from egonet_amd.common.img_proc import modify_bbox
    ego = build_model(args)
    sizes = tuple(int(s) for s in args.sizes.split(','))
    path = plan.export_plan(ego, args.out, batch_sizes=sizes, decode=args.decode)
    P = plan.Plan(path)
    print('%s: %d programs for %r, %d pieces, %.1f MB' % (path, P.info['n_programs'], P.info['batch_sizes'], P.info['n_pieces'],
                                                           os.path.getsize(path) / 1e6))
    if args.case:
        w, h = ego.resolution
        crops = synth.synth_crops(args.case_n, P.info['C'], h, w, seed=8).numpy()
        rets = [modify_bbox(b, h / w) for b in synth.synth_boxes(args.case_n, seed=2)]
        K = np.array([[707.0493, 0., 604.0814], [0., 707.0493, 180.5066], [0., 0., 1.]])
        write_case(args.case, crops, np.stack([r['c'] for r in rets]), np.stack([r['s'] for r in rets]), K)
        print('%s: %d crops' % (args.case, args.case_n))
    P.close()


if __name__ == '__main__':
    main()
