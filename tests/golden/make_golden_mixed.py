#!/usr/bin/env python
"""Generate the mixed-batch fixtures by RUNNING THE REFERENCE on the CPU (make_golden.py's stubs, borrowed exactly as
make_golden_train_samples.py borrows them; neither script is changed):

  mixed_samples.npz   the reference's ``instanceto2d`` batch with ``ss.flag`` on: per labelled frame
                      ``get_tensor_from_img`` then ``KITTI.extract_ss_sample`` (car_instance.py:1283-1298, 1145-1169;
                      called unbound on a stub that holds ``ss_settings``, ``ss_record``, ``hm_para``, ``pth_trans``),
                      then ``my_collate_fn`` / ``length_limit`` (car_instance.py:1344-1391), for a seeded ``np.random``.
  mixed_loss.npz      the reference's ``JointsCompositeLoss.forward`` (function.py:170-202) on 3 predictions and 2
                      targets, 33 joints, ``apply_cr_loss`` on: the total and its three terms.

As in make_golden_train_samples.py no pixels are recorded: ``warpAffine`` records its matrix, ``pth_trans`` returns zeros.
``np.random.rand`` / ``randint`` / ``choice`` are wrapped to record the reference's own draws.

Cases (prefix '<case>/'), KITTI_train_IGRs.yml heat-map settings, frames from ``egonet_amd.synth.synth_frame_records``:
  mix        3 labelled frames with 2, 1 and 3 boxes, max_per_img 4, a pool of 3 unlabelled frames with 3 boxes each:
             2, 3 and 1 unlabelled crops kept
  full       labelled frames with 4, 2 and 5 boxes, max_per_img 4: no draw for the first and the last
  valid      the 'mix' records with split 'valid': no unlabelled crops, no randint
  limit_fs   25 frames x 6 boxes, max_per_img 8: N = 200, n_fs = 150 > MAX_INS_CNT -- a choice among the labelled
             crops, the unlabelled ones dropped, no 'fs_instance_cnt'
  limit_ss   20 frames x 6 boxes, max_per_img 8: N = 160, n_fs = 120 -- the first 140 kept
Each: the labelled inputs (boxes, joints, frame index), the pool (boxes, joints), every draw in stream order, the warp
matrices in call order, per instance of the collated batch (before length_limit) its warp and source frame, the kept
indices, n_fs, the collated meta and whether it holds 'fs_instance_cnt'; cases with maps also targets and weights.

Usage:  python tests/golden/make_golden_mixed.py       (from the repo root)
The generation is deterministic: re-running leaves both files byte-identical.
"""
import json
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (the reference's import stubs; sets the repository root on sys.path)
import make_golden_train_samples as mgts  # noqa: E402  (cfgs_of / hm_para: the keys the reference's dataset reads)

CAR = mgts.CAR
NUM_JOINTS = mgts.NUM_JOINTS
POOL = (3, 3, (110, 170), 40)            # unlabelled pool: frames, boxes per frame, frame (h, w), seed
IMG_ROOT = 'unlabelled'
# name: (split, boxes of every labelled frame, max_per_img, frame (h, w), seed, store maps)
CASES = {
    'mix': ('train', [2, 1, 3], 4, (150, 310), 11, True),
    'full': ('train', [4, 2, 5], 4, (150, 310), 12, True),
    'valid': ('valid', [2, 1, 3], 4, (150, 310), 11, True),
    'limit_fs': ('train', [6] * 25, 8, (120, 200), 13, False),
    'limit_ss': ('train', [6] * 20, 8, (120, 200), 14, False),
}


def case_records(name):
    """The labelled records of a case: ``synth_frame_records`` with the largest box count, cut per frame."""
    from egonet_amd import synth
    _, per, _, hw, seed, _ = CASES[name]
    recs = synth.synth_frame_records(len(per), max(per), NUM_JOINTS, seed=seed, hw=hw)
    return [dict(r, boxes=r['boxes'][:n], joints=r['joints'][:n]) for r, n in zip(recs, per)]


def pool_records():
    """The unlabelled pool; the record's paths lie in another directory than ``img_root`` (only the basename counts,
    car_instance.py:1158-1159)."""
    from egonet_amd import synth
    n, bpf, hw, seed = POOL
    recs = synth.synth_frame_records(n, bpf, NUM_JOINTS, seed=seed, hw=hw)
    return [dict(r, path=os.path.join('elsewhere', 'apollo', os.path.basename(r['path']))) for r in recs]


def mixed_samples(lip, ci, frames, warps):
    logs = {'rand': [], 'randint': [], 'choice': []}
    orig = {k: getattr(np.random, k) for k in logs}

    def wrap(name):
        def f(*a, **k):
            v = orig[name](*a, **k)
            logs[name].append(np.array(v))
            return v
        return f
    for name in logs:
        setattr(np.random, name, wrap(name))

    pool = pool_records()
    ss_record = {'paths': [r['path'] for r in pool], 'boxes': [r['boxes'] for r in pool],
                 'kpts': [r['joints'] for r in pool]}
    arrs = {'cases': np.array(json.dumps({k: {'split': v[0], 'per_frame': v[1], 'max_per_img': v[2], 'hw': list(v[3]),
                                              'seed': v[4], 'maps': v[5], 'settings': CAR}
                                          for k, v in CASES.items()})),
            'pool': np.array(json.dumps({'n_frames': POOL[0], 'boxes_per_frame': POOL[1], 'hw': list(POOL[2]),
                                         'seed': POOL[3], 'img_root': IMG_ROOT, 'paths': ss_record['paths']})),
            'pool/frames_crc': np.array([zlib.crc32(np.ascontiguousarray(r['image']).tobytes()) for r in pool]),
            'pool/boxes': np.stack(ss_record['boxes']), 'pool/joints': np.stack(ss_record['kpts']),
            'max_ins_cnt': np.array(ci.MAX_INS_CNT)}
    try:
        for name, (split, per, max_per_img, hw, seed, maps) in CASES.items():
            cfgs = mgts.cfgs_of(CAR)
            para = mgts.hm_para(cfgs, split)
            h, w = int(para['input_size'][0]), int(para['input_size'][1])

            def pth_trans(img, h=h, w=w):
                return torch.zeros(3, h, w)
            recs = case_records(name)
            frames.clear()
            for r in recs:
                frames[r['path']] = r['image']
            for r in pool:
                frames[os.path.join(IMG_ROOT, os.path.basename(r['path']))] = r['image']
            stub = types.SimpleNamespace(ss_settings={'flag': True, 'max_per_img': max_per_img, 'img_root': IMG_ROOT},
                                         ss_record=ss_record, hm_para=para, pth_trans=pth_trans)
            del warps[:]
            for v in logs.values():
                del v[:]
            np.random.seed(2000 + seed)
            batch, fs_warp, ss_warp, ss_src = [], [], [], []
            for f, r in enumerate(recs):
                para['boxes'] = r['boxes']
                first = len(warps)
                images_fs, heatmaps_fs, weights_fs, meta_fs = lip.get_tensor_from_img(
                    r['path'], para, joints=r['joints'], pth_trans=pth_trans, rf=para['rf'], sf=para['sf'],
                    generate_hm=True)
                fs_warp += list(range(first, len(warps)))
                if split == 'train':                         # car_instance.py:1293 (use_ss is set)
                    first, drawn = len(warps), len(logs['randint'])
                    images_ss, _, _, _ = ci.KITTI.extract_ss_sample(stub, len(images_fs))
                    ss_warp += list(range(first, first + len(images_ss)))
                    if len(logs['randint']) > drawn:
                        ss_src += [len(recs) + int(logs['randint'][-1])] * len(images_ss)
                    batch.append(([images_fs, images_ss], heatmaps_fs, weights_fs, meta_fs))
                else:
                    batch.append((images_fs, heatmaps_fs, weights_fs, meta_fs))
            n_fs, n_all = len(fs_warp), len(fs_warp) + len(ss_warp)
            images, targets, weights, meta = ci.my_collate_fn(batch)
            assert len(logs['choice']) <= 1
            if logs['choice']:
                kept = logs['choice'][0]
            else:
                kept = np.arange(min(n_all, ci.MAX_INS_CNT))
            assert len(images) == len(kept) and len(targets) == len(weights) == len(meta['center'])
            p = name + '/'
            arrs[p + 'np_seed'] = np.array(2000 + seed)
            arrs[p + 'frames_crc'] = np.array([zlib.crc32(np.ascontiguousarray(r['image']).tobytes()) for r in recs])
            arrs[p + 'boxes'] = np.concatenate([r['boxes'] for r in recs])
            arrs[p + 'joints'] = np.concatenate([r['joints'] for r in recs])
            arrs[p + 'frame'] = np.concatenate([np.full(len(r['boxes']), f) for f, r in enumerate(recs)])
            arrs[p + 'rand'] = np.array(logs['rand'], dtype=np.float64).reshape(-1, 4)
            arrs[p + 'randint'] = np.array(logs['randint'], dtype=np.int64).reshape(-1)
            arrs[p + 'choice'] = (logs['choice'][0] if logs['choice'] else np.zeros(0)).astype(np.int64)
            arrs[p + 'warps'] = np.stack(warps)
            arrs[p + 'inst_warp'] = np.array(fs_warp + ss_warp, dtype=np.int64)
            arrs[p + 'inst_frame'] = np.concatenate([arrs[p + 'frame'], np.array(ss_src, dtype=np.int64)])
            arrs[p + 'kept'] = np.asarray(kept, dtype=np.int64)
            arrs[p + 'n_fs'] = np.array(len(targets))
            arrs[p + 'fs_instance_cnt'] = np.array(meta.get('fs_instance_cnt', -1))
            arrs[p + 'paths'] = np.array(json.dumps(meta['path']))
            for key in ('center', 'scale', 'transformed_joints', 'joints_vis', 'original_joints'):
                arrs[p + key] = np.asarray(meta[key])
            if maps:
                arrs[p + 'targets'] = targets.numpy()
                arrs[p + 'target_weights'] = weights.numpy()
            print('%-9s %3d labelled + %3d unlabelled, %3d kept (%3d with targets), %3d rand, %2d randint, %d choice'
                  % (name, n_fs, n_all - n_fs, len(kept), len(targets), len(logs['rand']), len(logs['randint']),
                     len(logs['choice'])))
    finally:
        for name in logs:
            setattr(np.random, name, orig[name])
    path = os.path.join(HERE, 'mixed_samples.npz')
    np.savez_compressed(path, **arrs)
    print('%-28s %8.1f KB' % ('mixed_samples.npz', os.path.getsize(path) / 1024))


def mixed_loss(ci):
    """JointsCompositeLoss.forward with more predictions than targets (function.py:183-201): L_hm and L_2d on the
    labelled prefix, L_cr and its mask over all rows."""
    import libs.loss.function as ref_loss
    cr_idx = ci.cr_indices_dict['bbox12']
    g = torch.Generator().manual_seed(505)
    w = [1.0, 0.1, 0.05]

    def criterion():
        lf = ref_loss.JointsCompositeLoss(spec_list=['mse', 'l1', 'sl1'], img_size=[256, 256], hm_size=[64, 64],
                                          loss_weights=w, cr_loss_thres=0.15)
        lf.cr_indices, lf.target_cr, lf.apply_cr_loss = cr_idx, 4 / 3, True
        return lf
    maps = torch.rand(3, 33, 8, 8, generator=g)
    coords = torch.rand(3, 33, 2, generator=g)
    target = torch.rand(2, 33, 8, 8, generator=g)
    joints = (torch.rand(2, 33, 3, generator=g) * 256).numpy()
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        lf = criterion()
        total = lf((maps, coords), target, None, {'transformed_joints': joints.copy()})
        hm = lf.calc_hm_loss(maps[:2], target) * w[0]
        coor = lf.calc_coor_loss(coords[:2], torch.from_numpy(joints[:, :, :2].astype(np.float32))) * w[1]
        mask = lf.get_cr_mask(coords.numpy(), lf.cr_loss_thres)
        cr = lf.calc_cross_ratio_loss(coords, lf.target_cr, mask) * w[2]
    finally:
        torch.Tensor.cuda = orig_cuda
    assert mask[2].sum() > 0 and mask[:2].sum() > 0          # the unlabelled row has lines in the term
    path = os.path.join(HERE, 'mixed_loss.npz')
    np.savez_compressed(path, maps=maps.numpy(), coords=coords.numpy(), target=target.numpy(), joints=joints,
                        cr_indices=np.asarray(cr_idx), weights=np.array(w), cr_loss_thres=np.array(0.15),
                        target_cr=np.array(4 / 3), img_size=np.array([256, 256]), mask=mask.numpy(),
                        total=np.array(float(total)), hm=np.array(float(hm)), coor=np.array(float(coor)),
                        cr=np.array(float(cr)))
    print('%-28s %8.1f KB   total %.8f = %.8f + %.8f + %.8f' % ('mixed_loss.npz', os.path.getsize(path) / 1024,
                                                               float(total), float(hm), float(coor), float(cr)))


def main():
    make_golden._install_stubs()
    import cv2
    frames, warps = {}, []

    def warp_affine(img, M, dsize, flags=None):
        warps.append(np.array(M, dtype=np.float64))
        return np.zeros((dsize[1], dsize[0], 3), dtype=np.uint8)

    cv2.imread = lambda path, flags=None: frames[path]
    cv2.cvtColor = lambda img, code: img
    cv2.COLOR_BGR2RGB = 4
    cv2.warpAffine = warp_affine
    sys.path.insert(0, make_golden.REF)
    import libs.common.img_proc as lip
    import libs.dataset.KITTI.car_instance as ci
    mixed_samples(lip, ci, frames, warps)
    mixed_loss(ci)


if __name__ == '__main__':
    main()
