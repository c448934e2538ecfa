"""The older block order of csrc/gemm.hip (EGONET_AMD_GEMM_RASTER=0, read once per process), as a stand-alone case run in
a process of its own by tests/test_gpu_gemm_sweep.py (tests/conv_h_graph_case.py's style):

    EGONET_AMD_GEMM_RASTER=0 python tests/gemm_raster_case.py OUT.pt

Replays gemm_sweep.raster_requests() on both sets of inputs with every check of the sweep and saves each C to OUT.pt;
the parent requires the bits of its own default-order launches.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def case(out):
    assert os.environ.get('EGONET_AMD_GEMM_RASTER') == '0', 'this case is about the older block order'
    import gemm_sweep as G
    import test_gpu_gemm_sweep as tg
    res = {}
    for k, r in enumerate(G.raster_requests()):
        for c in G.CASES:
            w, fails, got = tg._replay(r, c)
            assert not fails, (r['srcs'], c, fails)
            res['%d-%s' % (k, c)] = got.cpu()
    torch.save(res, out)
    print('gemm raster case ok')


if __name__ == '__main__':
    case(sys.argv[1])
