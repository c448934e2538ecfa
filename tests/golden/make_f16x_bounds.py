"""Writes tests/golden/f16x_mode_bounds.json: E, the error precision = 'f16x' is ALLOWED, measured on the CPU.

    python tests/golden/make_f16x_bounds.py

As tests/golden/make_f16_bounds.py and make_f16s2_bounds.py (same quantities and file shape), on the W32 model of
tests/f16x_mode_case.py: engine.f16_emulation(net, precision='f16x') rounds the input and the filter of every
``engine.f16_eligible``, ``engine.f16s2_eligible`` AND ``engine.f16x_eligible`` convolution to f16.  E = the maximum
deviation of that emulation from the plain fp32 CPU forward; the device result must stay within 2 E of the fp32 CPU
forward.  No GPU is involved; the file records the torch version it was written with."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import f16x_mode_case as case  # noqa: E402


def compute():
    torch.manual_seed(0)
    out = {'_doc': 'E per head type and batch: max |f16x emulation - fp32| of the CPU forwards '
                   '(tests/golden/make_f16x_bounds.py); the device result must be within 2 E of the fp32 CPU forward',
           '_torch': torch.__version__}
    for head in case.HEADS:
        net = case.model(head)
        out[head] = {}
        for which in case.BATCHES:
            x = case.crops(which)
            ref = case.cpu_f32(net, x)
            emu, hit, hit_x = case.cpu_emulated(net, x)
            assert hit == hit_x > 0           # a W32 model: every lowered layer is one of the 32-multiple widths
            out[head][which] = dict(case.deviations(emu, ref), f16_convs=hit, f16x_convs=hit_x,
                                    scale={k: float(v.abs().max()) for k, v in ref.items()})
    return out


def main():
    out = compute()
    with open(case.BOUNDS_PATH, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
