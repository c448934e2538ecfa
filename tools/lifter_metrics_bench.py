#!/usr/bin/env python
"""One validation pass of the lifter with the 3-D metrics on the device against the same pass through the host path
of the same classes (egonet_amd.metric.criterions), on the same box.

    python tools/lifter_metrics_bench.py [--rows 14000] [--passes 7] [--out profiles/lifter_metrics_bench.json]
    python tools/lifter_metrics_bench.py --kernel-only      # a few device passes, for rocprofv3 --kernel-trace --stats

A pass is ``trainer.evaluate`` over a normalised ``LifterPairs`` valid set (batches of 1024, ``unnormalize: True``)
with ``Evaluator(['RError3D'])`` and ends with ``report()``, i.e. includes the device path's one read-back.  Host
pass: the same evaluator with ``device_update`` off, so ``evaluate`` copies every batch to the host, unnormalises
there and the classes run their numpy restatement of the reference.  Two sizes: the synthetic valid set of
tools/train_lifting.py --synthetic 2000 and N rows (about KITTI's unaugmented val.txt car set).  Medians of
``--passes`` passes after two warm-up passes; a host clock around work that ends in a device synchronise."""
import argparse
import json
import logging
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from egonet_amd import synth, trainer                       # noqa: E402
from egonet_amd.common import lifter_pairs as lp            # noqa: E402
from egonet_amd.metric.criterions import Evaluator          # noqa: E402
from egonet_amd.model import FCmodel                        # noqa: E402
import train_lifting                                        # noqa: E402


def valid_set_of(cfgs, train_stats, rows):
    """A valid set of at least ``rows`` pairs (synthetic labels, no augmentation), cut to ``rows``."""
    n_labels = rows
    while True:
        ds = lp.LifterPairBuilder(cfgs, 'valid')(synth.synth_kitti_labels(n_labels, seed=1))
        if len(ds) >= rows:
            break
        n_labels = int(n_labels * 1.3) + 8
    ds.input, ds.output, ds.total_data = ds.input[:rows], ds.output[:rows], rows
    if ds.root_list is not None:
        ds.root_list = ds.root_list[:rows]
    return ds.normalize(train_stats)


def one_pass(ds, net, cfgs, logger, device):
    ev = Evaluator(['RError3D'], cfgs, ds.num_joints)
    ev.device_update = device
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.evaluate(ds, net, None, cfgs, logger, ev)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, ev.metrics[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--rows', type=int, default=14000)
    ap.add_argument('--passes', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-only', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lifter_metrics_bench: needs the GPU')
    args = argparse.Namespace(neurons=1024, blocks=2, dropout=0.5, out_rep='R3d', lr=1e-3, epochs=1, batch_size=1024,
                              report_every=100, aug_times=100, metrics=None, eval_every=0, eval_start_epoch=0)
    cfgs = train_lifting.lifting_cfgs(args)
    logger = logging.getLogger('lifter_metrics_bench')
    logger.addHandler(logging.NullHandler())
    logger.propagate = False
    cfgs['training_settings']['lft_aug_times'] = 4
    train_set = lp.LifterPairBuilder(cfgs, 'train')(synth.synth_kitti_labels(2000, seed=0)).normalize()
    net = FCmodel.get_fc_model(1, cfgs, 66, 96)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=3))
    net = net.cuda()
    synth_valid = lp.LifterPairBuilder(cfgs, 'valid')(synth.synth_kitti_labels(200, seed=1)).normalize(
        train_set.statistics)
    sets = [('synthetic valid set', synth_valid), ('%d rows' % a.rows, valid_set_of(cfgs, train_set.statistics, a.rows))]
    if a.kernel_only:
        for _, ds in sets:
            for _ in range(3):
                one_pass(ds, net, cfgs, logger, True)
        return
    result = {'what': 'trainer.evaluate + Evaluator([RError3D]), unnormalize True, batches of 1024; seconds per pass, '
                      'median of %d after 2 warm-up passes' % a.passes, 'sizes': []}
    for label, ds in sets:
        times = {True: [], False: []}
        for i in range(a.passes + 2):
            for device in (True, False):                    # alternating: the same conditions for both
                t, m = one_pass(ds, net, cfgs, logger, device)
                if i >= 2:
                    times[device].append(t)
                if device:
                    dev_m = m
        diff = float(abs(dev_m.mean_R - m.mean_R).max())
        entry = {'label': label, 'rows': len(ds), 'device_s': statistics.median(times[True]),
                 'host_s': statistics.median(times[False]), 'device_all_s': times[True], 'host_all_s': times[False],
                 'max_abs_diff_mean_R_deg': diff}
        entry['device_faster'] = entry['device_s'] < entry['host_s']
        result['sizes'].append(entry)
        print('%-20s %6d rows: device %.3f ms, host %.3f ms per pass' % (label, len(ds), 1e3 * entry['device_s'],
                                                                       1e3 * entry['host_s']))
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(result, indent=1) + '\n')
    if not all(e['device_faster'] for e in result['sizes']):
        raise SystemExit('the device pass is not faster than the host pass')


if __name__ == '__main__':
    main()
