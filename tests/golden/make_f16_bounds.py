"""Writes tests/golden/f16_mode_bounds.json: E, the error the f16-operand mode is ALLOWED, measured on the CPU.

    python tests/golden/make_f16_bounds.py

The network-level error of precision = 'f16' cannot be derived, and must not be taken from the kernels under test.  It is
taken from the CPU emulation (engine.f16_emulation: the model's own fp32 torch forward with the input and the filter of
every ``engine.f16_eligible`` convolution rounded to f16): E = the maximum deviation of that emulation from the plain
fp32 CPU forward, per output quantity (tests/f16_mode_case.py), for each head type and each test batch.  The device
result must stay within 2 E of the fp32 CPU forward: |gpu - f32| <= |gpu - emulation| + E, and the first term is made of
the same f16 rounding decisions flipped by fp32-level differences, so it is of the size of E and not larger.
No GPU is involved; the file records the torch version it was written with."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import f16_mode_case as case  # noqa: E402


def main():
    torch.manual_seed(0)
    out = {'_doc': 'E per head type and batch: max |f16 emulation - fp32| of the CPU forwards (tests/golden/make_f16_bounds.py); '
                   'the device result must be within 2 E of the fp32 CPU forward',
           '_torch': torch.__version__}
    for head in case.HEADS:
        net = case.model(head)
        out[head] = {}
        for which in case.BATCHES:
            x = case.crops(which)
            ref = case.cpu_f32(net, x)
            emu, hit = case.cpu_emulated(net, x)
            assert hit > 0
            out[head][which] = dict(case.deviations(emu, ref), f16_convs=hit,
                                    scale={k: float(v.abs().max()) for k, v in ref.items()})
    with open(case.BOUNDS_PATH, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
