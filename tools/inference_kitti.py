"""End-to-end inference on a KITTI-style directory (the flow of the reference's
``tools/inference.py:main/inference`` for BASELINE config 5): frames + 2D boxes ->
GPU crops -> HRNet key-points -> lifter -> pose solve -> KITTI result files ->
(optionally) 2D AP / AOS, bird's-eye-view AP and 3D AP against labels.

    python tools/inference_kitti.py --images <dir of png> --boxes <dir of KITTI label/detection txt>
        [--calib <dir>] --out <result dir> [--ckpt <dir with HC.pth L.pth LS.npy> | --synthetic]
        [--gt <label dir>] [--classes Car] [--conf-thres 0] [--alpha-mode proj|trans] [--frames-per-step 8]
        [--refine pnp [--refine-max-shift 5.0] [--write-3d]] [--precision f32|f16|f16s2|f16x] [--activations f32|f16]
        [--draw <dir> [--draw-gt]]

``--draw DIR`` also draws every frame's predictions (2-D boxes, projected cuboids, key points) with the GPU rasteriser
(EgoNet.post_process(visualize=True), csrc/overlay.hip) and writes ``DIR/<stem>.png`` plus, where the boxes carry 3-D
placements, the top view ``DIR/<stem>_bev.png``; ``--draw-gt`` (needs ``--gt``) adds the label boxes to the top view.

``--precision f16`` (default f32) is the opt-in fast mode of the key-point network: the 3x3 / stride 1 convolutions of
HRNet's stages 2-4 run with f16 operands and fp32 accumulation (csrc/conv_h.hip); results differ from the default's at
the 1e-3 px level ("f16-operand mode").  ``--precision f16s2`` adds the 3x3 / stride 2 convolutions of the
transition and fuse layers; ``--precision f16x`` those and the 3x3 convolutions of the 32-multiple widths (HRNet-W32's
stages; layer1, the stem's second convolution and transition1 in every width).  ``--activations f16`` (default f32)
stores the tensors between two f16-operand convolutions as f16: the results keep their bits.

``--refine pnp`` fits every lifted cuboid rigidly to its own key points before the angles are read off
(EgoNet.refine_pnp, the reference's ``pnp_refine`` flow without cv2); ``rot_y`` / ``alpha`` then come from the refined
points.  ``--write-3d`` (opt-in, needs ``--refine``) also replaces ``locations`` and ``dimensions`` of the refined
instances by the fit's own (bottom-face centre = refined root + R (0, h/2, 0); l, h, w = mean edge lengths), so boxes
of a 2-D detector, which carry -1000 there, give result lines the BEV / 3-D evaluator can score.

Multi-GPU (BASELINE config 5's 8-GPU form): launch one process per GPU with
``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...``;
the frames are sharded contiguously by rank (egonet_amd.parallel.shard_range), every rank holds a
full weight copy and writes the result files of its own frames -- no collective on the data path;
rank 0 waits at a barrier, fills in the empty files and runs the evaluator.

Boxes come from KITTI lines (ground-truth labels = the reference's ``use_gt_box``, or a 2D/3D
detector's result files = ``use_pred_box``).  Every frame is uploaded once as uint8; all its
boxes are cropped in one launch (csrc/crop.hip).  Result files go to ``<out>/data/%06d.txt``
in the format the evaluator reads; frames without predictions get empty files
(tools/inference.py:198-210).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egonet_amd import configs, evaluate, synth                      # noqa: E402
from egonet_amd.common import crop_gpu                                # noqa: E402
from egonet_amd.common import format as kfmt                          # noqa: E402
from egonet_amd.model.egonet import EgoNet                            # noqa: E402

KITTI_K = np.array([[707.0493, 0., 604.0814], [0., 707.0493, 180.5066], [0., 0., 1.]])


def read_calib(path):
    """P2 of a KITTI calib file -> K (3x3); the default KITTI intrinsics when absent."""
    if path and os.path.isfile(path):
        with open(path) as f:
            for line in f:
                if line.startswith('P2:'):
                    p = np.array([float(v) for v in line.split()[1:13]]).reshape(3, 4)
                    return p[:, :3].copy()
    return KITTI_K.copy()


def read_boxes(path, classes, thres):
    rows = []
    if os.path.isfile(path):
        with open(path) as f:
            for line in f:
                if len(line.split()) >= 15:
                    d = kfmt.parse_label_line(line)
                    if d['class'].lower() in classes and d.get('score', 1.0) >= thres:
                        rows.append(d)
    return rows


def build_model(a):
    cfg = configs.w48_config('coordinates') if not a.tiny else configs.hrnet_config(
        8, (64, 64), 33, 'coordinates', modules=(1, 1, 1), num_blocks=1, lifter_neurons=128)
    if a.ckpt:
        cfg['dirs'] = {'ckpt': a.ckpt}
        return EgoNet(cfg, pre_trained=True, precision=a.precision, activations=a.activations).eval().cuda()
    ego = EgoNet(cfg, pre_trained=False, precision=a.precision, activations=a.activations)               # --synthetic: seeded random weights (no checkpoint offline)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=6))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=7))
    ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    return ego.eval().cuda()


def write_3d(record):
    """``--write-3d``: a copy of the record's ``raw_txt_format`` whose refined instances (status 1) carry the fit's own
    ``locations`` (refined root + R (0, h/2, 0), the bottom-face centre) and ``dimensions`` (l, h, w)."""
    rows = []
    for i, row in enumerate(record['raw_txt_format']):
        row = dict(row)
        if record['refine_status'][i] == 1:
            l, h, w = (float(v) for v in record['refine_dims'][i])
            R = record['refine_rt'][i, :9].reshape(3, 3)
            loc = record['translation'][i] + R @ np.array([0., 0.5 * h, 0.])
            row['locations'] = [float(v) for v in loc]
            row['dimensions'] = [l, h, w]
        rows.append(row)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', required=True)
    ap.add_argument('--boxes', required=True)
    ap.add_argument('--calib', default=None)
    ap.add_argument('--out', required=True)
    ap.add_argument('--ckpt', default=None)
    ap.add_argument('--synthetic', action='store_true')
    ap.add_argument('--tiny', action='store_true', help='tiny HC / lifter (tests)')
    ap.add_argument('--gt', default=None)
    ap.add_argument('--classes', default='Car')
    ap.add_argument('--conf-thres', type=float, default=0.0)
    ap.add_argument('--alpha-mode', default='proj', choices=['proj', 'trans'])
    ap.add_argument('--frames-per-step', type=int, default=8)
    ap.add_argument('--refine', default=None, choices=['pnp'], help='fit the lifted cuboid to its key points first')
    ap.add_argument('--refine-max-shift', type=float, default=5.0,
                    help='discard a fit whose root moved further than this (m) from the box it started at')
    ap.add_argument('--write-3d', action='store_true',
                    help="write the fit's own locations / dimensions for refined instances (needs --refine)")
    ap.add_argument('--precision', default='f32', choices=['f32', 'f16', 'f16s2'] + ['f16x'],
                    help="f16: the key-point network's 3x3 stride-1 convolutions with f16 operands (opt-in fast mode); "
                         "f16s2: those and the 3x3 stride-2 ones; f16x: those and the 3x3 convolutions of the 32-multiple widths")
    ap.add_argument('--activations', default='f32', choices=['f32', 'f16'],
                    help='f16: tensors between two f16-operand convolutions are stored as f16 (the same results, fewer bytes)')
    ap.add_argument('--draw', default=None, metavar='DIR', help='draw the predictions on the frames, PNGs into DIR')
    ap.add_argument('--draw-gt', action='store_true', help='add the label boxes of --gt to the top view')
    a = ap.parse_args(argv)
    if a.draw_gt and not (a.draw and a.gt):
        ap.error('--draw-gt needs --draw and --gt')
    if not a.ckpt and not a.synthetic:
        ap.error('give --ckpt <dir> or --synthetic')
    if a.write_3d and not a.refine:
        ap.error('--write-3d needs --refine')
    classes = {c.strip().lower() for c in a.classes.split(',')}
    data_dir = os.path.join(a.out, 'data')
    os.makedirs(data_dir, exist_ok=True)
    # one process per GPU: contiguous shard of the frame list per rank, no data-path collective
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    dist = None
    if world > 1:
        import torch.distributed as dist
        from egonet_amd.parallel import shard_range
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
        dist.init_process_group('nccl')
    ego = build_model(a)
    names = sorted(f for f in os.listdir(a.images) if f.lower().endswith(('.png', '.jpg', '.jpeg')))
    all_names = names
    if world > 1:
        lo_r, hi_r = shard_range(len(names), world, rank)
        names = names[lo_r:hi_r]
    n_inst, n_refined, n_drawn, t0 = 0, 0, 0, time.perf_counter()
    colors = {'bbox_2d': 'r', 'bbox_3d': 'r', 'kpts': ['rx', 'r']}      # tools/inference.py:185-188
    for lo in range(0, len(names), a.frames_per_step):
        annot = {'path': [], 'boxes': [], 'raw_txt_format': [], 'K': []}
        images = {}
        for name in names[lo:lo + a.frames_per_step]:
            stem = os.path.splitext(name)[0]
            rows = read_boxes(os.path.join(a.boxes, stem + '.txt'), classes, a.conf_thres)
            if not rows:
                continue
            path = os.path.join(a.images, name)
            annot['path'].append(path)
            annot['boxes'].append(np.array([r['bbox'] for r in rows], dtype=np.float64))
            annot['raw_txt_format'].append(rows)
            annot['K'].append(read_calib(os.path.join(a.calib, stem + '.txt') if a.calib else None))
            images[path] = crop_gpu.load_rgb(path)
        if not annot['path']:
            continue
        records = ego(annot, images=images)
        save = {'flag': True, 'save_dir': data_dir}
        gt_rows = None
        if a.draw:
            save['vis_dir'] = a.draw
            if a.draw_gt:
                gt_rows = {p: read_boxes(os.path.join(a.gt, os.path.splitext(os.path.basename(p))[0] + '.txt'),
                                         classes, 0.0) for p in annot['path']}
        if not a.write_3d:
            ego.post_process(records, visualize=bool(a.draw), color_dict=colors, save_dict=save,
                             alpha_mode=a.alpha_mode, refine=a.refine == 'pnp', max_shift=a.refine_max_shift,
                             images=images, gt_rows=gt_rows)
        else:       # get_pred_str stays as it is: it formats this tool's edited copy of raw_txt_format
            for path, rec in records.items():
                rec = ego.gather_lifting_results(rec, alpha_mode=a.alpha_mode, refine=True,
                                                 max_shift=a.refine_max_shift)
                n_refined += int((rec['refine_status'] == 1).sum())
                rec['raw_txt_format'] = write_3d(rec)
                rec['pred_str'] = kfmt.get_pred_str(rec)
                kfmt.save_txt_file(path, rec, save)
            if a.draw:
                ego.draw_records(records, colors, save, images, gt_rows)
        if a.draw:
            n_drawn += sum(v is not None for rec in records.values() for v in rec['plots'].values())
        n_inst += sum(len(b) for b in annot['boxes'])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dist is not None:
        cnt = torch.tensor([float(n_inst), dt], dtype=torch.float64, device='cuda')
        tmax = cnt[1:].clone()
        dist.all_reduce(cnt[:1])                         # instances of the whole job
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)      # slowest rank (also the barrier before the evaluator)
        n_inst, dt = int(cnt[0].item()), float(tmax.item())
        if rank != 0:
            dist.destroy_process_group()
            return None
    names = all_names
    written = set(os.listdir(data_dir))
    for name in names:                                   # frames without predictions: empty result files
        stem = os.path.splitext(name)[0] + '.txt'
        if stem not in written:
            open(os.path.join(data_dir, stem), 'w').close()
    out = {'frames': len(names), 'instances': n_inst, 'seconds': round(dt, 3), 'n_gpus': world,
           'instances_per_s': round(n_inst / dt, 1) if dt > 0 else None, 'result_dir': data_dir}
    if a.refine:
        out['refine'] = a.refine
    if a.write_3d and world == 1:
        out['refined_3d'] = n_refined
    if a.draw and world == 1:
        out['drawn'] = n_drawn
    if dist is not None:
        dist.destroy_process_group()
    if a.gt:
        res = evaluate.evaluate_kitti(a.gt, a.out)
        out['eval'] = {k: {s: v[s] for s in ('AP', 'AOS', 'AP_bev', 'AP_3d') if s in v}
                       for k, v in res.items() if isinstance(v, dict)}
        for k, v in out['eval'].items():
            for s, vals in v.items():
                if vals is not None:
                    print('%s %s: %.4f %.4f %.4f' % (k, s, vals[0], vals[1], vals[2]), file=sys.stderr)
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
