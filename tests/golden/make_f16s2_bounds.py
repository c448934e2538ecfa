"""Writes tests/golden/f16s2_mode_bounds.json: E, the error precision = 'f16s2' is ALLOWED, measured on the CPU.

    python tests/golden/make_f16s2_bounds.py

As tests/golden/make_f16_bounds.py (same model, batches, quantities and file shape; tests/f16_mode_case.py), with the
emulation of the wider mode: engine.f16_emulation(net, precision='f16s2') rounds the input and the filter of every
``engine.f16_eligible`` AND every ``engine.f16s2_eligible`` convolution to f16.  E = the maximum deviation of that
emulation from the plain fp32 CPU forward; the device result must stay within 2 E of the fp32 CPU forward.  No GPU is
involved; the file records the torch version it was written with."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import f16s2_mode_case as case  # noqa: E402


def main():
    torch.manual_seed(0)
    out = {'_doc': 'E per head type and batch: max |f16s2 emulation - fp32| of the CPU forwards '
                   '(tests/golden/make_f16s2_bounds.py); the device result must be within 2 E of the fp32 CPU forward',
           '_torch': torch.__version__}
    for head in case.HEADS:
        net = case.model(head)
        out[head] = {}
        for which in case.BATCHES:
            x = case.crops(which)
            ref = case.cpu_f32(net, x)
            emu, hit, hit_s2 = case.cpu_emulated(net, x)
            assert hit > hit_s2 > 0
            out[head][which] = dict(case.deviations(emu, ref), f16_convs=hit, f16s2_convs=hit_s2,
                                    scale={k: float(v.abs().max()) for k, v in ref.items()})
    with open(case.BOUNDS_PATH, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
