#!/usr/bin/env python
"""Measure the lifter-pair front end (egonet_amd.common.lifter_pairs) and write profiles/lifter_pairs_bench.json.

    python tools/lifter_pairs_bench.py [--labels 14000] [--aug-times 100] [--out profiles/lifter_pairs_bench.json]
    python tools/lifter_pairs_bench.py --build-only       # one warm-up + one build: the run to put under a profiler

Build: host time (draws + packing; parsing excluded: the labels are synthetic records), the upload, and each entry
point between device events of its own (inputs uploaded, outputs allocated) after a warm-up build; the bytes each
must move, computed from the shapes; bytes/s and the share of the HBM peak (8 TB/s).  Feeding: samples/s of ``trainer.train`` for one epoch at batch 2048 and 4096 (a)
through ``device_loader``, (b) through the ``DataLoader`` path (the same rows as host numpy, 4 workers),
alternating, three times each; beside them the bare ``LifterTrainStep`` on resident batches."""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egonet_amd import _lib, configs, synth, trainer        # noqa: E402
from egonet_amd.common import lifter_pairs as lp            # noqa: E402
from egonet_amd.model import FCmodel                        # noqa: E402

HBM_PEAK = 8.0e12


def cfgs_of(T, batch, workers=4):
    cfg = configs.clone(configs.w48_config())
    cfg.update(use_gpu=True, exp_type='2dto3d', cascade={'num_stages': 1},
               dataset={'detect_classes': ['Car'], '3d_kpt_sample_style': 'bbox9',
                        'interpolate': {'flag': True, 'style': 'bbox12', 'coef': [0.332, 0.667]},
                        'lft_in_rep': 'coordinates2d', 'lft_out_rep': 'R3d'},
               optimizer={'optim_type': 'adam', 'lr': 1e-3, 'weight_decay': 0.0, 'momentum': 0.9,
                          'milestones': [100], 'gamma': 0.1},
               training_settings={'total_epochs': 1, 'batch_size': batch, 'num_threads': workers, 'shuffle': True,
                                  'report_every': 10 ** 9, 'eval_during': False, 'plot_loss': False,
                                  'lft_aug': True, 'lft_aug_times': T})
    return cfg


class _Timed(object):
    def __init__(self):
        self.ev = []

    def mark(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev.append(e)

    def ms(self):
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in zip(self.ev[:-1], self.ev[1:])]


def measure_build(n_labels, T):
    """Every entry point between device events of its own, on arrays that are already uploaded and outputs that are
    already allocated, after a warm-up build; the per-kernel split of the three generation launches comes from the
    profiler run (--build-only under rocprofv3)."""
    records = synth.synth_kitti_labels(n_labels, seed=1)
    b = lp.LifterPairBuilder(cfgs_of(T, 2048), 'train')
    rng = np.random.RandomState(3)
    b(records, rng=rng).normalize()                         # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    labels, lf, frames = b.gather(records)
    draws = b.draw(len(labels), rng)
    host_ms = (time.perf_counter() - t0) * 1e3
    host = [np.ascontiguousarray(labels), np.ascontiguousarray(lf, dtype=np.int32), np.ascontiguousarray(frames),
            np.ascontiguousarray(draws)]
    up_bytes = sum(a.nbytes for a in host)
    t = _Timed()
    t.mark()
    dev = [torch.from_numpy(a).cuda() for a in host]
    t.mark()
    upload_ms = t.ms()[0]
    L = _lib.lib()
    A, J = len(labels), b.num_joints
    NS = A * (T + 1)
    ci, co = 2 * J, 3 * (J - 1)
    nb = L.egn_lifter_pairs_ws_bytes(A, T)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    in2d = torch.empty(NS, ci, dtype=torch.float32, device='cuda')
    out3d = torch.empty(NS, co, dtype=torch.float32, device='cuda')
    roots = torch.empty(NS, 3, dtype=torch.float64, device='cuda')
    st = _lib.current_stream()
    torch.cuda.synchronize()
    t = _Timed()
    t.mark()
    _lib.check(L.egn_lifter_pairs_f64(_lib.ptr(dev[0]), _lib.ptr(dev[1]), A, _lib.ptr(dev[2]), len(frames),
                                      _lib.ptr(dev[3]), T, b.coef[0], b.coef[1], 2, 0, _lib.ptr(ws), nb,
                                      _lib.ptr(in2d), _lib.ptr(out3d), _lib.ptr(roots), st), 'lifter pairs')
    t.mark()
    gen_ms = t.ms()[0]                                      # flags + scan + write, three launches
    N = int(ws[:8].view(torch.int64).item())
    ds = lp.LifterPairs(in2d[:N], out3d[:N], roots[:N].cpu().numpy(), ws[nb - NS:].cpu().numpy().astype(bool), 'R3d')
    ds.column_statistics(ds.input)                          # the statistics' work space comes from the allocator's cache
    torch.cuda.synchronize()
    t = _Timed()
    t.mark()
    mi, si = ds.column_statistics(ds.input)
    t.mark()
    mo, so = ds.column_statistics(ds.output)
    t.mark()
    _lib.check(L.egn_normalize_rows_f32(_lib.ptr(ds.input), N, ci, _lib.ptr(mi), _lib.ptr(si), st), 'normalise')
    _lib.check(L.egn_normalize_rows_f32(_lib.ptr(ds.output), N, co, _lib.ptr(mo), _lib.ptr(so), st), 'normalise')
    t.mark()
    st_in_ms, st_out_ms, norm_ms = t.ms()
    ds.statistics = {'mean_in': mi.cpu().numpy().reshape(1, -1), 'std_in': si.cpu().numpy().reshape(1, -1),
                     'mean_out': mo.cpu().numpy().reshape(1, -1), 'std_out': so.cpu().numpy().reshape(1, -1)}
    row = 4 * (ci + co) + 24
    # generation: the flag pass reads labels / draws and writes NS flags, the write pass reads them again and
    # stores N rows; statistics read the rows twice (mean, then deviation); normalise reads and writes them once
    out = {'labels': n_labels, 'aug_times': T, 'samples': NS, 'kept': N,
           'host_ms': host_ms, 'upload_ms': upload_ms, 'upload_bytes': up_bytes,
           'generate_ms': gen_ms, 'generate_bytes': N * row + 2 * NS + 2 * up_bytes,
           'statistics_in_ms': st_in_ms, 'statistics_in_bytes': 2 * N * 4 * ci,
           'statistics_out_ms': st_out_ms, 'statistics_out_bytes': 2 * N * 4 * co,
           'normalize_ms': norm_ms, 'normalize_bytes': 2 * N * 4 * (ci + co)}
    for k in ('generate', 'statistics_in', 'statistics_out', 'normalize'):
        bps = out[k + '_bytes'] / max(out[k + '_ms'], 1e-9) * 1e3
        out[k + '_bytes_per_s'] = bps
        out[k + '_share_of_hbm_peak'] = bps / HBM_PEAK
    return out, ds


class _Host(torch.utils.data.Dataset):
    """The parent path: the same rows as host numpy, one row per item (car_instance.py:1241-1247)."""

    def __init__(self, ds):
        self.x, self.y = ds.input.cpu().numpy(), ds.output.cpu().numpy()
        self.sizes = ds.get_input_output_size()

    def get_input_output_size(self):
        return self.sizes

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.y[i], np.zeros((0, 1)), {}


def _model(ds, cfg):
    isz, osz = ds.get_input_output_size()
    cfg['FCModel']['input_size'], cfg['FCModel']['output_size'] = isz, osz
    return FCmodel.get_fc_model(1, cfgs=cfg, input_size=isz, output_size=osz).cuda()


def epoch_rate(dataset, batch, logger):
    cfg = cfgs_of(100, batch)
    model = _model(dataset, cfg)
    optim, sche = trainer.prepare_optim(model, cfg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.train(dataset, model, None, optim, sche, cfg, logger)
    torch.cuda.synchronize()
    return len(dataset) / (time.perf_counter() - t0)


def bare_rate(ds, batch, steps=200):
    cfg = cfgs_of(100, batch)
    model = _model(ds, cfg)
    step = trainer.make_step(model, cfg, None, trainer.prepare_optim(model, cfg)[0])
    x, y = ds.input[:batch].clone(), ds.output[:batch].clone()
    for _ in range(10):
        step.step(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.step(x, y)
    torch.cuda.synchronize()
    return steps * batch / (time.perf_counter() - t0)


def measure_feeding(ds, rows):
    logger = logging.getLogger('lifter_pairs_bench')
    logger.handlers = [logging.NullHandler()]
    logger.propagate = False
    sub = lp.LifterPairs(ds.input[:rows], ds.output[:rows], ds.root_list[:rows], ds.keep, 'R3d')
    host = _Host(sub)
    out = {'rows': len(sub)}
    for batch in (2048, 4096):
        epoch_rate(sub, batch, logger)                      # warm-up of the step at this batch size
        a, b, bare = [], [], []
        for _ in range(3):
            a.append(epoch_rate(sub, batch, logger))
            b.append(epoch_rate(host, batch, logger))
            bare.append(bare_rate(sub, batch))
        out['batch_%d' % batch] = {'device_loader_samples_per_s': a, 'dataloader_4_workers_samples_per_s': b,
                                   'bare_step_samples_per_s': bare,
                                   'bare_step_spread': (max(bare) - min(bare)) / max(bare),
                                   'device_loader_vs_bare': float(np.median(a) / np.median(bare)),
                                   'dataloader_vs_bare': float(np.median(b) / np.median(bare))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--labels', type=int, default=14000)
    ap.add_argument('--aug-times', type=int, default=100)
    ap.add_argument('--feed-rows', type=int, default=1000000)
    ap.add_argument('--build-only', action='store_true')
    ap.add_argument('--out', default=os.path.join('profiles', 'lifter_pairs_bench.json'))
    args = ap.parse_args()
    _lib.lib()
    build, ds = measure_build(args.labels, args.aug_times)
    result = {'device': torch.cuda.get_device_name(0), 'hbm_peak_bytes_per_s': HBM_PEAK, 'build': build}
    if not args.build_only:
        result['feeding'] = measure_feeding(ds, min(args.feed_rows, len(ds)))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write('\n')
    print(json.dumps(result, sort_keys=True))


if __name__ == '__main__':
    main()
