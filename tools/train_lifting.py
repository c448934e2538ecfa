#!/usr/bin/env python
"""Train the lifter sub-model L from KITTI labels: the counterpart of the reference's tools/train_lifting.py.

    python tools/train_lifting.py --label-dir <label_2> --calib-dir <calib> --train-list train.txt \
        --valid-list val.txt --out <dir> [--size 1242 375] [--epochs 300] [--batch-size 2048]
        [--eval-every 500 --eval-start-epoch 250 --metrics RError3D] [--checkpoint FILE] [--resume FILE]
    python tools/train_lifting.py --synthetic 2000 --out <dir>       # seeded synthetic labels, no KITTI tree

Pairs are built on the device (egonet_amd.common.lifter_pairs), normalised with the train set's statistics, fed to
``trainer.train_cascade`` from HBM, and ``L.pth`` + ``LS.npy`` are written like train_lifting.py:51-54.  A split
list holds one frame name per line ('000123'); the image size is taken from ``--size`` (the reference opens every
image for it; KITTI frames differ by a few pixels -- pass records with their own sizes through the Python API
where that matters).

``--eval-every N`` validates every N batches after ``--eval-start-epoch`` like the reference's ``eval_during``
(configs/KITTI_train_lifting.yml: eval_every 500, eval_start_epoch 250) with the metrics of ``--metrics``
(``RError3D``; ``RTError3D`` for ``--out-rep R3d+T``): rotation error and MPJPE of the unnormalised cuboids, computed
on the device (egonet_amd.metric.criterions).  The run ends with one more pass over the valid pairs.

``--checkpoint FILE`` writes a training checkpoint after every epoch (``training_settings.checkpoint``): the model, the
native step's optimizer state -- also in ``torch.optim`` form --, the schedule, the loss history, and beside it
``FILE.rank<r>`` with the generators' states and the dropout seed.  ``--resume FILE`` (``training_settings.resume``, the
reference's key) continues such a run at the epoch after its last, with the moments, the step counter, the learning
rates and the dropout stream where the uninterrupted run would have them; ``--epochs`` is the total.  The tool trains
one cascade stage, which is the stage the file belongs to."""
import argparse
import logging
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egonet_amd import configs, synth, trainer          # noqa: E402
from egonet_amd.common import lifter_pairs as lp        # noqa: E402
from egonet_amd.metric.criterions import Evaluator      # noqa: E402


def lifting_cfgs(args):
    """The keys of configs/KITTI_train_lifting.yml that the builder and the trainer read."""
    cfg = configs.clone(configs.w48_config())
    metrics = args.metrics or ['RTError3D' if args.out_rep == 'R3d+T' else 'RError3D']
    eval_during = args.eval_every > 0
    cfg['FCModel'].update(num_neurons=args.neurons, num_blocks=args.blocks, dropout=args.dropout)
    cfg.update(use_gpu=True, exp_type='2dto3d', cascade={'num_stages': 1},
               metrics={'R3D': {'T_style': 'direct', 'R_style': 'euler', 'style': 'euler'},
                        'RTError3D': {'T_style': 'direct', 'R_style': 'euler'}, 'JD3D': {'style': 'direct'}},
               dataset={'detect_classes': ['Car'], '3d_kpt_sample_style': 'bbox9',
                        'interpolate': {'flag': True, 'style': 'bbox12', 'coef': [0.332, 0.667]},
                        'lft_in_rep': 'coordinates2d', 'lft_out_rep': args.out_rep},
               optimizer={'optim_type': 'adam', 'lr': args.lr, 'weight_decay': 0.0, 'momentum': 0.9,
                          'milestones': [int(0.5 * args.epochs) or 1, int(0.75 * args.epochs) or 1], 'gamma': 0.1},
               training_settings={'total_epochs': args.epochs, 'batch_size': args.batch_size, 'num_threads': 4,
                                  'shuffle': True, 'report_every': args.report_every, 'eval_during': eval_during,
                                  'eval_every': args.eval_every, 'eval_start_epoch': args.eval_start_epoch,
                                  'eval_metrics': metrics, 'plot_loss': False, 'lft_aug': True,
                                  'lft_aug_times': args.aug_times},
               testing_settings={'batch_size': args.batch_size, 'num_threads': 4, 'shuffle': False,
                                 'unnormalize': True})
    cfg['optimizer'].update(trainer.optim_keys_from_args(args))
    cfg['training_settings'].update(trainer.checkpoint_keys_from_args(args))       # --checkpoint / --resume
    return cfg


def _mse(prediction, target, weights, meta):
    return torch.nn.functional.mse_loss(prediction, target)


def kitti_records(label_dir, calib_dir, list_path, size, classes):
    with open(list_path) as fh:
        names = [ln.strip() for ln in fh if ln.strip()]
    return [{'labels': lp.read_label_file(os.path.join(label_dir, n + '.txt'), classes),
             'P': lp.read_calib_file(os.path.join(calib_dir, n + '.txt')), 'size': size, 'path': n + '.png'}
            for n in names]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--label-dir')
    ap.add_argument('--calib-dir')
    ap.add_argument('--train-list')
    ap.add_argument('--valid-list')
    ap.add_argument('--synthetic', type=int, default=0, metavar='N', help='N seeded synthetic labels instead of KITTI')
    ap.add_argument('--out', required=True)
    ap.add_argument('--size', type=int, nargs=2, default=[1242, 375], metavar=('W', 'H'))
    ap.add_argument('--out-rep', default='R3d', choices=['R3d', 'R3d+T'])
    ap.add_argument('--aug-times', type=int, default=100)
    ap.add_argument('--epochs', type=int, default=300)
    ap.add_argument('--batch-size', type=int, default=2048)
    ap.add_argument('--lr', type=float, default=1e-3)
    trainer.add_optim_arguments(ap)
    trainer.add_checkpoint_arguments(ap)
    ap.add_argument('--neurons', type=int, default=1024)
    ap.add_argument('--blocks', type=int, default=2)
    ap.add_argument('--dropout', type=float, default=0.5)
    ap.add_argument('--report-every', type=int, default=100)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--eval-every', type=int, default=0, metavar='N',
                    help='validate every N batches during training (0 = off)')
    ap.add_argument('--eval-start-epoch', type=int, default=0, help='validate only after this epoch')
    ap.add_argument('--metrics', nargs='+', default=None,
                    help='metrics of the validation (default RError3D, RTError3D for --out-rep R3d+T)')
    args = ap.parse_args()
    logging.basicConfig(level=logging.INFO, format='%(message)s')
    logger = logging.getLogger('train_lifting')
    cfgs = lifting_cfgs(args)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if args.synthetic:
        train_rec = synth.synth_kitti_labels(args.synthetic, seed=args.seed)
        valid_rec = synth.synth_kitti_labels(max(args.synthetic // 10, 4), seed=args.seed + 1)
    else:
        if not (args.label_dir and args.calib_dir and args.train_list):
            ap.error('--label-dir, --calib-dir and --train-list are needed without --synthetic')
        classes = tuple(cfgs['dataset']['detect_classes'])
        train_rec = kitti_records(args.label_dir, args.calib_dir, args.train_list, tuple(args.size), classes)
        valid_rec = kitti_records(args.label_dir, args.calib_dir, args.valid_list, tuple(args.size), classes) \
            if args.valid_list else None
    train_set = lp.LifterPairBuilder(cfgs, 'train')(train_rec).normalize()
    logger.info('train: %d pairs of %d samples kept' % (len(train_set), len(train_set.keep)))
    valid_set = None
    if valid_rec:
        valid_set = lp.LifterPairBuilder(cfgs, 'valid')(valid_rec).normalize(train_set.statistics)
        logger.info('valid: %d pairs' % len(valid_set))
    record = trainer.train_cascade(train_set, valid_set, cfgs, logger)
    if valid_set is not None:                               # trainer.py:395-513 over the valid pairs, from HBM too
        evaluator = Evaluator(cfgs['training_settings']['eval_metrics'], cfgs, train_set.num_joints)
        trainer.evaluate(valid_set, record['cascade'][0].cuda(), _mse, cfgs, logger, evaluator)
    os.makedirs(args.out, exist_ok=True)
    torch.save(record['cascade'][0].cpu().state_dict(), os.path.join(args.out, 'L.pth'))
    np.save(os.path.join(args.out, 'LS.npy'), train_set.statistics)
    logger.info('=> wrote %s and %s' % (os.path.join(args.out, 'L.pth'), os.path.join(args.out, 'LS.npy')))


if __name__ == '__main__':
    main()
