"""The f16-operand convolution op of the 32-multiple widths captured into a hipGraph and replayed
(egn_program_capture / egn_program_replay), as a stand-alone case run in a process of its own by
tests/test_gpu_conv_hx.py (tests/conv_h_graph_case.py's style: graph replays stay out of the suite's own process):

    python tests/conv_hx_graph_case.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def case():
    from egonet_amd import _lib
    import test_gpu_conv_hx as th
    L = _lib.lib()
    for shape in (th.SHAPES[1], th.SHAPES[6]):          # one per stride
        t = th.make(*shape, seed=4)
        want = th.run_direct(t).clone()
        y = torch.full_like(want, th.CANARY)
        prog = th._program(t, y, lanes=False)
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                st = _lib.current_stream()
                _lib.check(L.egn_program_run(prog, st))
                s.synchronize()
                assert torch.equal(y, want)
                _lib.check(L.egn_program_capture(prog, st), 'capture')
                n0 = L.egn_launch_count()
                for _ in range(2):
                    y.fill_(th.CANARY)
                    _lib.check(L.egn_program_replay(prog, st), 'replay')
                    s.synchronize()
                    assert torch.equal(y, want)
                assert L.egn_launch_count() - n0 == 2          # one kernel node per replay
        finally:
            L.egn_program_destroy(prog)
    print('conv hx graph case ok')


if __name__ == '__main__':
    case()
