"""Point-to-point dependencies in the program runner (egn_program_set_deps; engine: EGONET_AMD_DEPS=1) on the GPU: the
recording in which fuse term (i, j) waits for branch j alone computes the bits of the recording with the joins
(EGONET_AMD_DEPS=0) -- no kernel, no argument and no association order differs, only when launches may start.

Shapes: the smallest that still have all four branches -- W48 at 2 crops of 256 x 256 and the fixtures' tiny config
(3 crops of 64 x 64); a second or two per case.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from egonet_amd import _lib, configs, engine, synth
from egonet_amd.model.heatmapModel import hrnet as hip_hrnet

pytestmark = pytest.mark.gpu

EGN_E_BADARG, EGN_E_STATE = -1, -3            # include/egonet_hip.h
CASES = {'w48': (lambda: configs.w48_config('heatmap'), 2, 256), 'tiny': (lambda: configs.tiny_config('heatmap'), 3, 64)}
_built = {}


def _engines(which, monkeypatch):
    """(net's engine with the joins, its engine with dependencies, crops, second crops): built once per model."""
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    monkeypatch.setenv('EGONET_AMD_PAIR', '0')
    monkeypatch.setenv('EGONET_AMD_GRAPH_MAX_N', '0')
    monkeypatch.setenv('EGONET_AMD_DEPS_MIN_N', '1')        # (these shapes are below the default threshold of 16 crops)
    if which not in _built:
        cfg, n, size = CASES[which]
        net = hip_hrnet.get_pose_net(cfg(), is_train=False)
        net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=4))
        net = net.eval().cuda()
        engs = []
        for deps in ('0', '1'):
            monkeypatch.setenv('EGONET_AMD_DEPS', deps)
            engs.append(engine.HRNetEngine(net))
        xs = [synth.synth_crops(n, 3, size, size, seed=31 + k).cuda() for k in range(2)]
        # the reference: the joined program's maps, soft-arg-max, maxima and indices; computed once, never written again
        want = [[t.clone() for t in torch.utils._pytree.tree_leaves(engs[0].forward(x, decode_mode=1))] for x in xs]
        torch.cuda.synchronize()
        _built[which] = (engs[0], engs[1], xs, want)
    return _built[which]


def _same(got, want):
    got = torch.utils._pytree.tree_leaves(got)
    assert len(got) == len(want) == 4
    return all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize('which', ['tiny', 'w48'])
def test_three_runs_equal_the_joined_program(which, monkeypatch):
    eng0, eng1, xs, want = _engines(which, monkeypatch)
    L = _lib.lib()
    prog0, prog1 = eng0.program(xs[0], 1), eng1.program(xs[0], 1)
    kinds = lambda p: sorted(m['kind'] for m in p.meta if m['kind'] not in ('fork', 'join'))
    forks = lambda p: sum(m['kind'] in ('fork', 'join') for m in p.meta)
    assert kinds(prog0) == kinds(prog1) and forks(prog1) < forks(prog0)
    assert L.egn_program_num_ops(prog1.handle) == len(prog1.meta)          # one meta entry per op: the ms array lines up
    n0 = L.egn_launch_count()
    for _ in range(3):
        got = eng1.forward(xs[0], decode_mode=1)
        torch.cuda.synchronize()
        assert _same(got, want[0])
    assert L.egn_launch_count() - n0 == 3 * len(kinds(prog1))
    # the serial timed run ignores the dependencies: same bits, one time per op
    got = eng1.forward(xs[0], decode_mode=1, timed=True)
    assert _same(got, want[0]) and len(eng1.last_ms) == len(prog1.meta)


@pytest.mark.parametrize('which', ['tiny', 'w48'])
def test_two_slots_in_flight_on_two_streams(which, monkeypatch):
    """Slot 0 and slot 1 are programs of their own -- own arena, own side streams, own events -- and run beside each other."""
    eng0, eng1, xs, want = _engines(which, monkeypatch)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    got = []
    for _ in range(3):
        for slot in (0, 1):
            with torch.cuda.stream(streams[slot]):
                got.append((slot, eng1.forward(xs[slot], decode_mode=1, slot=slot)))
    torch.cuda.synchronize()
    assert eng1.program(xs[0], 1, 0) is not eng1.program(xs[1], 1, 1)
    assert all(_same(g, want[slot]) for slot, g in got)


def _ramp_op(L, prog, k):
    """Coordinate ramps into the k-th [1, 4, 4, 4] tensor of the buffer: the smallest op a program has."""
    _lib.check(L.egn_program_add_ramps(prog, _lib.Ref(0, 256 * k), 1, 4, 4, 4, 1))


def test_a_wait_names_an_earlier_signal_or_is_refused():
    L = _lib.lib()
    buf = torch.zeros(3, 64, device='cuda')
    prog = C.c_void_p(L.egn_program_create(2))
    try:
        _lib.check(L.egn_program_bind(prog, 0, _lib.ptr(buf)))
        ints = lambda *v: (C.c_int * len(v))(*v)
        assert L.egn_program_set_deps(prog, 1, None, 0) == EGN_E_STATE                 # no op yet
        _lib.check(L.egn_program_fork(prog))                                           # op 0
        assert L.egn_program_set_deps(prog, 1, None, 0) == EGN_E_BADARG                # a fork carries no dependency
        _lib.check(L.egn_program_set_lane(prog, 1))
        _ramp_op(L, prog, 0)                                                           # op 1, lane 1: signals
        _lib.check(L.egn_program_set_deps(prog, 1, None, 0))
        _ramp_op(L, prog, 1)                                                           # op 2, lane 1: does not
        _lib.check(L.egn_program_set_lane(prog, 0))
        _ramp_op(L, prog, 2)                                                           # op 3, lane 0
        for bad in (3, 4, 7, -1, 2, 0):          # itself, later ops, nonsense, an op that does not signal, the fork
            assert L.egn_program_set_deps(prog, 0, ints(bad), 1) == EGN_E_BADARG, bad
        assert L.egn_program_set_deps(prog, 0, ints(1, 3), 2) == EGN_E_BADARG          # one bad wait refuses the call
        assert L.egn_program_set_deps(prog, 0, None, 1) == EGN_E_BADARG
        _lib.check(L.egn_program_set_deps(prog, 1, ints(1), 1))                        # the earlier signal: taken
        _lib.check(L.egn_program_join(prog))
        for _ in range(2):
            _lib.check(L.egn_program_run(prog, _lib.current_stream(buf.device)))
        torch.cuda.synchronize()
        assert all(float(buf[k].abs().sum()) > 0 for k in range(3)) and torch.equal(buf[0], buf[1]) and \
            torch.equal(buf[0], buf[2])
    finally:
        L.egn_program_destroy(prog)


@pytest.mark.parametrize('which', ['tiny', 'w48'])
def test_capture_and_replay_keep_the_bits(which):
    """tests/program_deps_case.py in a process of its own, as the other graph-replay case of the suite runs."""
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'program_deps_case.py'), which],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and 'program deps case ok' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
