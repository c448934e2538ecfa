"""The paired convolution op captured into a hipGraph and replayed (egn_program_capture / egn_program_replay), as a
stand-alone case run in a process of its own by tests/test_gpu_conv_pair.py (tests/graph_case.py's style: graph replays
stay out of the suite's own process):

    python tests/conv_pair_graph_case.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def case():
    from egonet_amd import _lib
    import test_gpu_conv_pair as tp
    L = _lib.lib()
    ta, tb = tp.half(3, 16, 16, 32, 96, True, 1), tp.half(5, 8, 8, 32, 48, True, 1)
    want_a, want_b = tp.run_single(ta, 86), tp.run_single(tb, 82)
    prog, keep = tp.pair_program(ta, tb, 0)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            st = _lib.current_stream()
            _lib.check(L.egn_program_run(prog, st))
            s.synchronize()
            assert torch.equal(ta['y'], want_a) and torch.equal(tb['y'], want_b)
            _lib.check(L.egn_program_capture(prog, st), 'capture')
            n0 = L.egn_launch_count()
            for _ in range(2):
                ta['y'].fill_(float('nan'))
                tb['y'].fill_(float('nan'))
                _lib.check(L.egn_program_replay(prog, st), 'replay')
                s.synchronize()
                assert torch.equal(ta['y'], want_a) and torch.equal(tb['y'], want_b)
            assert L.egn_launch_count() - n0 == 2          # one kernel node per replay
    finally:
        L.egn_program_destroy(prog)
    print('conv pair graph case ok')


if __name__ == '__main__':
    case()
