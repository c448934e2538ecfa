#!/usr/bin/env python
"""Train the key-point sub-model HC from a KITTI tree: the counterpart of the reference's tools/train_IGRs.py:49-106.

    python tools/train_IGRs.py --kitti <dir with image_2 label_2 calib> [--split-file <stems>]
        [--valid-split-file <stems>] --out <dir> [--epochs 45] [--batch-frames 8] [--eval-every N] [--seed S]
        [--tiny] [--max-steps N] [--workers 4] [--report-every 30] [--lr 1e-3]
        [--exp-type instanceto2d|baselinealpha|baselinetheta] [--loss-type MSELoss1D|SmoothL1Loss1D]
        [--cr-weight W] [--ss-record FILE --ss-img-root DIR [--ss-max-per-img 6]] [--no-debug-pictures]
        [--checkpoint FILE] [--resume FILE]

Labels + calibration -> ``PoseAnnotBuilder`` (the 2-D pose annotations, built on the device:
egonet_amd.common.pose_annot) -> ``PoseFrames`` -> ``DataLoader(collate_fn=collate_frames)`` (frames decoded in the
workers) -> ``trainer.train(sample_builder=TrainSampleBuilder(...))`` (crops and targets on the device, the native
tape), with the settings of configs/KITTI_train_IGRs.yml.  ``HC.pth`` (a flat ``state_dict`` with the reference's
keys, what ``EgoNet(cfgs, pre_trained=True)`` loads) is written into ``--out``.

A split file holds one frame name per line ('000123'); without one every label file of the tree is used.  A batch is
``--batch-frames`` frames with all their kept cars.  ``--eval-every N`` scores the validation split (the training
frames without ``--valid-split-file``) every N batches with ``JointDistance2DSIP`` on the device; with a validation
split the run also ends with one pass over it.  ``--max-steps N`` ends the run after N steps; ``--tiny`` trains the
small network of tools/inference_kitti.py --tiny (tests).  One JSON line is printed: frames, the instances kept and
dropped at each of the two filters, steps, ``last_loss``, the output path.  ``last_loss`` is the last loss the trainer
REPORTED (every ``--report-every`` batches of an epoch, starting with batch 0), not the last step's: with
``--report-every 30 --max-steps 2`` it is step 0's.

``--exp-type baselinealpha | baselinetheta`` trains the paper's direct-regression baselines instead: the same backbone
with the 'angleregression' head on targets ``[cos r, sin r]`` of ``alpha`` / ``rot_y`` (``PoseFrames`` carries the
annotations' ``rots``, ``TrainSampleBuilder(target=...)`` emits them), the criterion ``--loss-type`` on the native step,
``AngleErrorMeter`` as the training metric and ``AngleError`` for validation; the state dict goes to
``<exp-type>.pth``.

``--ss-record FILE --ss-img-root DIR`` switch on the self-supervised mix (the ``ss`` block of KITTI_train_IGRs.yml):
``FILE`` is the reference's record of unlabelled frames (a ``.npy`` dictionary with ``paths`` and ``boxes``), ``DIR``
holds the images under their basenames.  Every labelled frame with fewer than ``--ss-max-per-img`` cars then brings
crops of one random unlabelled frame (``MixedFrames``); the heat-map and coordinate terms see the labelled crops, the
cross-ratio term and BatchNorm all of them.  ``--cr-weight W`` is the third entry of ``loss_weight_list`` ('None' in the
shipped file): the weight of the cross-ratio term, which counts from the second epoch on.  The mix needs it.

Like the shipped config (``training_settings.debug``: ``save`` and its three ``save_*`` keys, all True) the key-point
run writes the reference's debug pictures on every report batch -- ``<out>/intermediate_results/train/
<epoch>_<batch>_{keypoints,hm_gt,hm_pred}.jpg``, composed on the device and encoded on a background thread
(egonet_amd/visualization/debug.py); ``--no-debug-pictures`` sets ``debug.save`` to False.  The angle baselines have
no maps and write none (train_IGRs.py:83-88).

``--checkpoint FILE`` writes a training checkpoint after every epoch (``training_settings.checkpoint``): the model, the
native step's optimizer state -- also in ``torch.optim`` form --, the schedule, the loss history, and beside it
``FILE.rank<r>`` with the generators' states.  ``--resume FILE`` (``training_settings.resume``, the reference's key)
loads one into the freshly built run and continues at the epoch after its last, on the schedule the uninterrupted run
would follow; ``--epochs`` is the total, and a run that already completed it is refused.  The same seed and settings
are the caller's part: a differing optimizer family, head or world size is refused.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egonet_amd import configs, trainer                                  # noqa: E402
from egonet_amd.common import crop_gpu, pose_annot, train_samples          # noqa: E402
from egonet_amd.loss import function as loss_function                      # noqa: E402
from egonet_amd.metric.criterions import AngleErrorMeter, DistanceSrcMeter, Evaluator       # noqa: E402
from egonet_amd.model.heatmapModel import hrnet                            # noqa: E402


def igr_cfgs(a):
    """The keys of configs/KITTI_train_IGRs.yml that the builders, the model and the trainer read."""
    exp_type = getattr(a, 'exp_type', 'instanceto2d')
    angle = exp_type in train_samples.EXP_TARGETS
    if angle:
        # the angle head pools a 4 x 4 map behind four stride-2 blocks (hrnet.py:384-422): 256 x 256 crops, tiny or not
        cfg = configs.clone(configs.hrnet_config(8, (256, 256), 33, 'angleregression', modules=(1, 1, 1), num_blocks=1)
                            if a.tiny else configs.w48_config('angleregression'))
    else:
        # --integral-terms: the plain heat-map head, its L_2d / L_cr on the soft-arg-max of the maps (function.py:187-201)
        head = 'heatmap' if getattr(a, 'integral_terms', False) else 'coordinates'
        cfg = configs.clone(configs.hrnet_config(8, (64, 64), 33, head, modules=(1, 1, 1), num_blocks=1)
                            if a.tiny else configs.w48_config(head))
    metric = 'AngleError' if angle else 'JointDistance2DSIP'
    cfg['heatmapModel'].update(jitter_bbox=True, jitter_params={'shift': [0.1, 0.1], 'scaling': [0.4, 0.4]},
                               loss_type='JointsCompositeLoss', loss_spec_list=['mse', 'l1', 'sl1'],
                               loss_weight_list=[1.0, 0.1, _cr_weight(a)], cr_loss_threshold=0.15,
                               target_type='gaussian', sigma=1)
    if getattr(a, 'integral_terms', False) and not angle:
        cfg['heatmapModel']['integral_terms'] = True            # the key trainer.make_step reads, not loss_type
    if angle:
        cfg['heatmapModel']['loss_type'] = a.loss_type          # one criterion: no spec / weight lists
        for key in ('loss_spec_list', 'loss_weight_list', 'cr_loss_threshold'):
            del cfg['heatmapModel'][key]
    cfg.update(train=True, use_gpu=True, exp_type=exp_type,
               dataset={'name': 'KITTI', 'detect_classes': ['Car'], '3d_kpt_sample_style': 'bbox9',
                        'interpolate': {'flag': True, 'style': 'bbox12', 'coef': [0.332, 0.667]},
                        '2d_kpt_style': 'bbox9',
                        'pth_transform': {'mean': list(crop_gpu.IMAGENET_MEAN), 'std': list(crop_gpu.IMAGENET_STD)}},
               optimizer={'optim_type': 'adam', 'lr': a.lr, 'weight_decay': 0.0, 'momentum': 0.9,
                          'milestones': [10, 20, 30, 40], 'gamma': 0.5},
               training_settings={'total_epochs': a.epochs, 'batch_size': a.batch_frames, 'num_threads': a.workers,
                                  'shuffle': True, 'use_target_weight': False, 'report_every': a.report_every,
                                  'eval_every': a.eval_every, 'eval_during': a.eval_every > 0,
                                  'eval_metrics': [metric], 'plot_loss': False,
                                  'debug': {'save': not getattr(a, 'no_debug_pictures', False), 'save_images_kpts': True,
                                            'save_hms_gt': True, 'save_hms_pred': True}},
               # the validation batches are built by a device front end inside collate_fn: no worker processes
               testing_settings={'batch_size': a.batch_frames, 'num_threads': 0, 'shuffle': False,
                                 'apply_dropout': False, 'unnormalize': False, 'arg_max': 'hard',
                                 'eval_metrics': [metric], 'alpha_mode': 'proj'})
    cfg['optimizer'].update(trainer.optim_keys_from_args(a))    # --optim / --weight-decay / --no-decay-norm-bias / ...
    cfg['training_settings'].update(trainer.checkpoint_keys_from_args(a))       # --checkpoint / --resume
    if getattr(a, 'freeze', None):
        # --freeze PREFIX ...: heatmapModel.extra.freeze_layers (hrnet.py:675-690); --freeze-bn: their BatchNorm layers
        # stay in eval mode too (extra.freeze_bn), the frozen-BatchNorm fine-tune
        cfg['heatmapModel']['extra']['freeze_layers'] = list(a.freeze)
    if getattr(a, 'freeze_bn', False):
        if not getattr(a, 'freeze', None):
            raise SystemExit('--freeze-bn needs --freeze PREFIX [PREFIX ...]: it freezes the BatchNorm layers under them')
        cfg['heatmapModel']['extra']['freeze_bn'] = True
    if getattr(a, 'out', None):
        cfg['dirs'] = {'output': a.out}
    if getattr(a, 'ss_record', None):
        cfg['ss'] = {'flag': True, 'record_path': a.ss_record, 'img_root': a.ss_img_root,
                     'max_per_img': a.ss_max_per_img}
    return cfg


def _cr_weight(a):
    w = getattr(a, 'cr_weight', None)
    return 'None' if w is None or w == 0 else float(w)


def build_model(cfgs, seed):
    """Seeds numpy and torch, then makes the network: the same seed gives the same initial weights and, from there,
    the same shuffles and box jitter."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    return hrnet.get_pose_net(cfgs, is_train=True).cuda()


def read_stems(path):
    with open(path) as fh:
        return [ln.strip() for ln in fh if ln.strip()]


class _BudgetLoader(object):
    """The ``DataLoader`` ``trainer.get_loader`` would make, ended when the run's step budget is used up."""

    def __init__(self, owner, batch_size, shuffle):
        self.owner = owner
        self.loader = torch.utils.data.DataLoader(owner.frames, batch_size=batch_size, shuffle=shuffle,
                                                  num_workers=owner.workers,
                                                  collate_fn=train_samples.collate_frames)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        if self.owner.left == 0:
            return
        for batch in self.loader:
            self.owner.steps += 1
            if self.owner.left is not None:
                self.owner.left -= 1
            yield batch
            if self.owner.left == 0:
                return


class _Budgeted(object):
    """``PoseFrames`` behind the loader hook of ``trainer.get_loader``: counts the steps, stops after ``max_steps``.

    A workaround, named as one: ``device_loader`` is the hook ``get_loader`` keeps for row sets that live on the
    device (``LifterPairs``); nothing here does.  It is used because ``trainer.train`` has no step limit and a loader
    is the only place a caller can end an epoch early without the trainer's cooperation.  Once the budget is used up
    the remaining epochs still run their ``sche.step()`` over an empty loader; the weights no longer change.  A
    ``max_steps`` argument of ``trainer.train`` would replace this class."""

    def __init__(self, frames, workers, max_steps):
        self.frames, self.workers = frames, workers
        self.left = max_steps if max_steps and max_steps > 0 else None
        self.steps = 0
        self.num_joints = frames.num_joints

    def __len__(self):
        return len(self.frames)

    def device_loader(self, batch_size, shuffle):
        return _BudgetLoader(self, batch_size, shuffle)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--kitti', required=True, help='directory with image_2, label_2 and calib')
    ap.add_argument('--split-file', default=None)
    ap.add_argument('--valid-split-file', default=None)
    ap.add_argument('--out', required=True)
    ap.add_argument('--epochs', type=int, default=45)
    ap.add_argument('--batch-frames', type=int, default=8)
    ap.add_argument('--eval-every', type=int, default=0, metavar='N', help='validate every N batches (0 = off)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--tiny', action='store_true', help='tiny HC (tests)')
    ap.add_argument('--max-steps', type=int, default=0, metavar='N', help='end the run after N steps (0 = no limit)')
    ap.add_argument('--workers', type=int, default=4)
    ap.add_argument('--report-every', type=int, default=30)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--freeze', nargs='+', default=None, metavar='PREFIX',
                    help='parameter-name prefixes that do not train (freeze_layers), e.g. conv1 bn1 conv2 bn2 layer1')
    ap.add_argument('--freeze-bn', action='store_true',
                    help='keep the BatchNorm layers under --freeze in eval mode: running statistics, nothing written')
    trainer.add_optim_arguments(ap)
    trainer.add_checkpoint_arguments(ap)
    ap.add_argument('--exp-type', default='instanceto2d', choices=['instanceto2d'] + sorted(train_samples.EXP_TARGETS))
    ap.add_argument('--loss-type', default='MSELoss1D', choices=['MSELoss1D', 'SmoothL1Loss1D'],
                    help='criterion of the angle baselines (libs/loss/function.py:204-228)')
    ap.add_argument('--cr-weight', type=float, default=None, metavar='W',
                    help="weight of the cross-ratio term, from the second epoch on (default: off, the shipped 'None')")
    ap.add_argument('--integral-terms', action='store_true',
                    help="train the plain heat-map head (head_type 'heatmap') with the coordinate and cross-ratio terms "
                         'on the soft-arg-max of its maps (heatmapModel.integral_terms)')
    ap.add_argument('--ss-record', default=None, metavar='FILE',
                    help="the record of unlabelled frames (.npy dictionary with 'paths' and 'boxes'): mixed batches")
    ap.add_argument('--ss-img-root', default=None, metavar='DIR', help='directory of the unlabelled images')
    ap.add_argument('--ss-max-per-img', type=int, default=6,
                    help='a labelled frame with fewer cars is filled up to this many crops from an unlabelled frame')
    ap.add_argument('--no-debug-pictures', action='store_true',
                    help='training_settings.debug.save = False: no key-point / heat-map pictures on report batches')
    a = ap.parse_args(argv)
    if bool(a.ss_record) != bool(a.ss_img_root):
        ap.error('--ss-record and --ss-img-root go together')
    if a.ss_record and a.exp_type in train_samples.EXP_TARGETS:
        ap.error('--ss-record: the angle baselines ignore the mix (car_instance.py:1248-1271)')
    if a.ss_record and _cr_weight(a) == 'None':
        ap.error('--ss-record without --cr-weight: the cross-ratio term is the only one that reads unlabelled crops; '
                 'unlabelled crops then only change BatchNorm statistics')
    if a.integral_terms and a.exp_type in train_samples.EXP_TARGETS:
        ap.error('--integral-terms belongs to the key-point model (instanceto2d)')
    if a.cr_weight is not None and a.exp_type in train_samples.EXP_TARGETS:
        ap.error('--cr-weight belongs to the key-point model (instanceto2d)')
    logging.basicConfig(level=logging.INFO, format='%(message)s')
    logger = logging.getLogger('train_IGRs')
    cfgs = igr_cfgs(a)
    angle = a.exp_type in train_samples.EXP_TARGETS
    metric = cfgs['testing_settings']['eval_metrics'][0]
    model = build_model(cfgs, a.seed)
    # train_IGRs.py:42: the criterion named by the config; the native step reads which one it is
    loss_func = getattr(loss_function, a.loss_type)() if angle else None
    target = train_samples.EXP_TARGETS.get(a.exp_type, 'heatmap')

    annot_builder = pose_annot.PoseAnnotBuilder(cfgs, 'train')
    annot = annot_builder(pose_annot.kitti_records(a.kitti, read_stems(a.split_file) if a.split_file else None))
    counts = annot_builder.last_counts
    logger.info('train: %(frames_kept)d of %(frames)d frames, %(kept_visible)d of %(labels)d cars '
                '(%(dropped_inlier)d outside the image, %(dropped_visible)d with too few visible points)' % counts)
    if not annot['paths']:
        ap.error('no car of %s passed the visibility filters' % a.kitti)
    frames = pose_annot.PoseFrames(annot)
    if a.ss_record:
        frames = train_samples.MixedFrames(frames, a.ss_record, a.ss_img_root, a.ss_max_per_img)
        logger.info('mixed batches: %d unlabelled frames, up to %d crops per labelled frame'
                    % (len(frames.ss_paths), a.ss_max_per_img))
    train_set = _Budgeted(frames, a.workers, a.max_steps)

    valid_frames, evaluator, evaluate_fn = None, None, None
    if a.valid_split_file or a.eval_every > 0:
        valid_annot = annot if not a.valid_split_file else pose_annot.PoseAnnotBuilder(cfgs, 'valid')(
            pose_annot.kitti_records(a.kitti, read_stems(a.valid_split_file)))
        valid_frames = pose_annot.PoseFrames(valid_annot)
        valid_builder = train_samples.TrainSampleBuilder(cfgs, split='valid', target=target)      # no jitter (img_proc.py:217)
        evaluator = Evaluator([metric], cfgs)

        def valid_collate(batch):
            return valid_builder(train_samples.collate_frames(batch))

        def evaluate_fn(dataset, mdl, epoch):
            return trainer.evaluate(dataset, mdl, loss_func, cfgs, logger, evaluator, collate_fn=valid_collate,
                                    epoch=epoch)

    optim, sche = trainer.prepare_optim(model, cfgs)
    # train_IGRs.py:83-88: the angle baselines save no debug pictures, the key-point model what its config says
    save_debug = False if angle else bool(cfgs['training_settings']['debug']['save'])
    record = trainer.train(train_set, model, loss_func, optim, sche, cfgs, logger,
                           metric_func=AngleErrorMeter(cfgs) if angle else DistanceSrcMeter(cfgs),
                           valid_dataset=valid_frames, evaluate_fn=evaluate_fn, save_debug=save_debug,
                           sample_builder=train_samples.TrainSampleBuilder(cfgs, split='train', target=target))
    if a.valid_split_file:                                  # trainer.py:395-513 over the validation split
        evaluate_fn(valid_frames, model, None)
        model.train()

    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, a.exp_type + '.pth' if angle else 'HC.pth')
    logger.info('=> saving final model state to {}'.format(path))
    torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, path)
    out = dict(counts, steps=train_set.steps, last_loss=record['loss'][-1] if record['loss'] else None, out=path)
    if evaluator is not None and evaluator.metrics[0].count:
        m = evaluator.metrics[0]
        out['eval'] = {'metric': metric, 'mean': float(m.mean), 'count': int(m.count)}
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
