"""Measure the paired launch of stage 4's two coarse branches (csrc/conv_wino4.hip, conv_wino4_pair_kernel) against the
two tabled single convolutions and write the entries of egonet_amd/tuned/gfx950_pairs.json (tuner.tune_pair: the pair op
as a one-op program against the sum of the two singles, each a one-op program; kept only where it is faster).

    python tools/tune_pairs.py --out /tmp/gfx950_pairs.json [--batches 64,128] [--a 16,192] [--b 8,384]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from egonet_amd import tuner                                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--batches', default='64')
    ap.add_argument('--a', default='16,192', help='map size, channels of the 16-divisible half')
    ap.add_argument('--b', default='8,384', help='map size, channels of the 8 x 8 half')
    a = ap.parse_args()
    (ha, ca), (hb, cb) = [tuple(int(v) for v in s.split(',')) for s in (a.a, a.b)]
    table = {}
    if os.path.isfile(tuner.PAIRS_PATH):
        with open(tuner.PAIRS_PATH) as f:
            table = json.load(f)
    dev = torch.device('cuda:0')
    for n in (int(v) for v in a.batches.split(',')):
        for res in (False, True):
            ka = (n, ha, ha, ca, ca, ca, ca, 3, 3, 1, 1, res, False)
            kb = (n, hb, hb, cb, cb, cb, cb, 3, 3, 1, 1, res, False)
            if tuner.pair_plans(ka, kb) is None:
                continue
            entry = tuner.tune_pair(dev, ka, kb)
            table[tuner.pair_key(ka, kb)] = entry
            print(tuner.pair_key(ka, kb), entry)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(table, f, indent=0, sort_keys=True)


if __name__ == '__main__':
    main()
