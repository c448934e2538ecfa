"""Capture / replay of a program with point-to-point dependencies (EGONET_AMD_DEPS=1) as a stand-alone case, run in a
process of its own by tests/test_gpu_program_deps.py::test_capture_and_replay_keep_the_bits (graph replays stay out of
the suite's process, as tests/graph_case.py does):

    python tests/program_deps_case.py tiny|w48

Under capture the runner lowers the dependencies to joins of all lanes (csrc/program.hip), so the graph has the fork /
join shape of the program recorded with joins; every side lane is joined at the end of its stage and the capture ends
with all streams back on the origin.  Three replays equal the eager run of the same program and the run with the joins.
Every step is announced on stderr, unbuffered: a process that dies says how far it came.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

os.environ['EGONET_AMD_AUTOTUNE'] = '0'
os.environ['EGONET_AMD_GRAPH_MAX_N'] = '0'
os.environ['EGONET_AMD_PAIR'] = '0'
os.environ['EGONET_AMD_DEPS_MIN_N'] = '1'          # (2 and 3 crops: below the default threshold of 16)

from egonet_amd import configs, engine, synth                           # noqa: E402
from egonet_amd.engine import SLOT_USER0                                 # noqa: E402
from egonet_amd.model.heatmapModel import hrnet as hip_hrnet             # noqa: E402


def _say(what):
    sys.stderr.write('program deps case: %s\n' % what)
    sys.stderr.flush()


def case(which):
    cfg, n, size = (configs.w48_config('heatmap'), 2, 256) if which == 'w48' else (configs.tiny_config('heatmap'), 3, 64)
    net = hip_hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=4))
    net = net.eval().cuda()
    x = synth.synth_crops(n, 3, size, size, seed=31).cuda()
    engs = {}
    for deps in ('0', '1'):
        os.environ['EGONET_AMD_DEPS'] = deps
        engs[deps] = engine.HRNetEngine(net)
    want = torch.utils._pytree.tree_leaves(engs['0'].forward(x, decode_mode=1))
    eager = torch.utils._pytree.tree_leaves(engs['1'].forward(x, decode_mode=1))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, want))
    _say('eager runs equal')
    prog = engs['1'].program(x, 1)
    forks = lambda p: sum(m['kind'] == 'fork' for m in p.meta)
    assert 0 < forks(prog) < forks(engs['0'].program(x, 1))             # the recording with dependencies
    shp = prog.out_shapes
    nn_, k = shp['maps'][:2]
    outs = [torch.empty(shp['maps'], device='cuda'), torch.empty(nn_, k, 2, device='cuda'),
            torch.empty(nn_, k, 1, device='cuda'), torch.empty(nn_, k, dtype=torch.int32, device='cuda')]
    prog.bind(SLOT_USER0, x)
    prog.bind(SLOT_USER0 + 1, outs[0])
    for j in range(3):
        prog.bind(shp['decode_slot'] + j, outs[1 + j])
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        prog.capture()
        _say('captured')
        for k in range(3):
            for t in outs:
                t.zero_()
            prog.replay()
            st.synchronize()
            _say('replay %d done' % k)
            assert all(torch.equal(a, b) for a, b in zip(outs, want)), which
    torch.cuda.synchronize()
    del prog, engs
    _say('programs released')


if __name__ == '__main__':
    case(sys.argv[1] if len(sys.argv) > 1 else 'tiny')
    print('program deps case ok')
