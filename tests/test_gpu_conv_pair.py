"""The paired F(4x4,3x3) launch on the GPU (csrc/conv_wino4.hip, conv_wino4_pair_kernel; egn_program_add_conv2d_pair).

One op runs two independent 3x3 convolutions -- ``a`` the way tile configuration 86 (conv_wino4w_kernel) runs it, ``b`` the
way 82 (conv_wino4c_kernel<0, 1>) does -- in two shares of one grid.  The bodies, the item order of each share and the
MFMA order per accumulator are those of the single kernels, so both outputs must equal the two one-op programs BIT FOR
BIT (``torch.equal``); those are held to float64 by tests/test_gpu_kernels.py and tests/test_gpu_conv_sweep.py.
Reference for the layers: libs/model/heatmapModel/hrnet.py:49-76 (BasicBlock), :286-287 (independent branches)."""
import os
import subprocess
import sys

import pytest
import torch

from egonet_amd import _lib, engine

pytestmark = pytest.mark.gpu


def half(n, h, w, cin, cout, use_res, act, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + cin + cout + h)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, act=act,
                x=torch.randn(n, h, w, cin, generator=g).cuda(), wp=engine.pack_for_kind(wt, 3).cuda(),
                sc=(torch.rand(cout, generator=g) + 0.5).cuda(), sh=torch.randn(cout, generator=g).cuda(),
                res=torch.randn(n, h, w, cout, generator=g).cuda() if use_res else None,
                y=torch.full((n, h, w, cout), float('nan'), device='cuda'))


def _bind(L, prog, t, slot0):
    refs = []
    for k, name in enumerate(('x', 'wp', 'sc', 'sh', 'res', 'y')):
        if t[name] is None:
            refs.append(_lib.NULL_REF)
            continue
        _lib.check(L.egn_program_bind(prog, slot0 + k, _lib.ptr(t[name])))
        refs.append(_lib.Ref(slot0 + k, 0))
    return refs


def run_single(t, cfg):
    """The half as a one-op program under ``cfg``; returns a copy of its output."""
    L = _lib.lib()
    prog = L.egn_program_create(8)
    assert prog
    try:
        refs = _bind(L, prog, t, 0)
        _lib.check(L.egn_program_add_conv2d(prog, *refs, t['n'], t['h'], t['w'], t['cin'], t['cin'], t['cout'], t['cout'],
                                            3, 3, 1, 1, t['act'], 0, cfg), 'single cfg %d' % cfg)
        t['y'].fill_(float('nan'))
        _lib.check(L.egn_program_run(prog, _lib.current_stream()))
        torch.cuda.synchronize()
        out = t['y'].clone()
    finally:
        L.egn_program_destroy(prog)
    assert torch.isfinite(out).all()
    t['y'].fill_(float('nan'))
    return out


def pair_program(ta, tb, grid_cap):
    L = _lib.lib()
    prog = L.egn_program_create(16)
    assert prog
    args = []
    for t, slot0 in ((ta, 0), (tb, 6)):
        args += _bind(L, prog, t, slot0) + [t['n'], t['h'], t['w'], t['cin'], t['cout'], t['act']]
    _lib.check(L.egn_program_add_conv2d_pair(prog, *(args + [grid_cap])), 'pair')
    assert L.egn_program_num_ops(prog) == 1
    return prog, (ta, tb)


def _pair_equals_singles(ta, tb, grid_cap=0, beside=None):
    L = _lib.lib()
    want_a, want_b = run_single(ta, 86), run_single(tb, 82)
    prog, _ = pair_program(ta, tb, grid_cap)
    try:
        if beside is not None:
            beside.feed()
        _lib.check(L.egn_program_run(prog, _lib.current_stream()))
        busy = beside is not None and not (beside.s_bw.query() and beside.s_mm.query())
        torch.cuda.synchronize()
        ms = (C_float * 1)()
        _lib.check(L.egn_program_run_timed(prog, _lib.current_stream(), ms, 1))      # one op: one time slot
    finally:
        L.egn_program_destroy(prog)
    assert torch.equal(ta['y'], want_a), (ta['y'] - want_a).abs().max()
    assert torch.equal(tb['y'], want_b), (tb['y'] - want_b).abs().max()
    assert ms[0] > 0
    return busy


import ctypes                # noqa: E402
C_float = ctypes.c_float


@pytest.mark.parametrize('res_a,res_b,act_a,act_b', [(True, True, 1, 1), (False, False, 0, 0), (True, False, 0, 1),
                                                     (False, True, 1, 0)])
def test_smallest_shapes_with_padding_blocks_and_images_past_n(res_a, res_b, act_a, act_b):
    """a 32 -> 96 @ 16 x 16, 3 images (3 of its 8 blocks have an item); b 32 -> 48 @ 8 x 8, 5 images: the second
    four-image region has three images past N that load zeros and store nothing (2 of its 8 blocks have an item)."""
    _pair_equals_singles(half(3, 16, 16, 32, 96, res_a, act_a), half(5, 8, 8, 32, 48, res_b, act_b))


@pytest.mark.parametrize('a,b', [
    # item order 0 in both shares: 24 items (two regions per image) on 8 blocks, 32 items (two co-tiles) on 16
    ((10, 16, 32, 32, 96), (40, 8, 8, 32, 96)),
    # item order 1 (four co-tile pairs / four co-tiles on the XCDs): 40 items on 32 blocks in each share
    ((10, 16, 16, 32, 384), (36, 8, 8, 32, 192)),
    # an odd number of 16-channel stages in both bodies (48 input channels), more co-tiles in b than in a
    ((9, 16, 16, 48, 96), (21, 8, 8, 48, 384)),
])
def test_persistent_loops_iterate_under_a_grid_cap(a, b):
    """The test-only grid cap plans for 16 compute units: every share has more items than blocks, the counts differ."""
    _pair_equals_singles(half(*a, True, 1, seed=1), half(*b, True, 1, seed=1), grid_cap=16)


def test_real_widths_beside_two_busy_streams():
    """Stage 4 of HRNet-W48: 192 -> 192 @ 16 x 16 beside 384 -> 384 @ 8 x 8, 8 crops, once alone and once while a bandwidth
    hog and an MFMA hog run on two other streams (one run: every vector-memory wait of both bodies is vmcnt(0))."""
    from test_gpu_stress_streams import _Hogs
    ta, tb = half(8, 16, 16, 192, 192, True, 1, seed=2), half(8, 8, 8, 384, 384, True, 1, seed=2)
    _pair_equals_singles(ta, tb)
    hogs = _Hogs('conv')
    busy = _pair_equals_singles(ta, tb, beside=hogs)
    hogs.join()
    assert busy, 'the side streams drained: not a stress run'


def test_the_op_refuses_what_the_plan_refuses_and_reports_summed_work():
    L = _lib.lib()
    ta, tb = half(3, 16, 16, 32, 96, True, 1), half(5, 8, 8, 32, 48, False, 1)
    prog, _ = pair_program(ta, tb, 0)
    try:
        kind, flops, nbytes = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        _lib.check(L.egn_program_op_info(prog, 0, kind, flops, nbytes, None, 0))
        assert flops.value == 2.0 * 9 * (3 * 256 * 96 * 32 + 5 * 64 * 48 * 32)
        assert nbytes.value == 4.0 * (3 * 256 * (32 + 2 * 96) + 9 * 96 * 32 + 5 * 64 * (32 + 48) + 9 * 48 * 32)
        args = []
        for t, slot0 in ((tb, 0), (ta, 6)):          # the halves swapped: an 8 x 8 map for a, a 16 x 16 one for b
            args += _bind(L, prog, t, slot0) + [t['n'], t['h'], t['w'], t['cin'], t['cout'], t['act']]
        assert L.egn_program_add_conv2d_pair(prog, *(args + [0])) != 0
        assert L.egn_program_num_ops(prog) == 1
    finally:
        L.egn_program_destroy(prog)


def test_replay_of_a_captured_pair_in_a_process_of_its_own():
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_pair_graph_case.py')],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'conv pair graph case ok' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_w48_paired_equals_the_two_single_configurations(monkeypatch):
    """HRNet-W48 @ 256 x 256, 2 crops: EGONET_AMD_PAIR=force against EGONET_AMD_PAIR=0 with configurations 86 / 82 handed
    to the two paired classes -- heat-maps and decode outputs bit-identical, 24 launches fewer (3 modules x 4 blocks x 2
    convolutions of stage 4's two coarse branches)."""
    from egonet_amd import configs, synth, tuner
    from egonet_amd.model.heatmapModel import hrnet as hip_hrnet
    L = _lib.lib()
    real_choose = tuner.choose

    def choose(device, key, kinds=tuner.DIRECT, *a, **kw):
        key = tuple(key)
        if key[7:11] == (3, 3, 1, 1) and 3 in kinds and (key[1], key[3], key[5]) in ((16, 192, 192), (8, 384, 384)):
            return 86 if key[1] == 16 else 82
        return real_choose(device, key, kinds, *a, **kw)
    monkeypatch.setattr(tuner, 'choose', choose)
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    net = hip_hrnet.get_pose_net(configs.w48_config('heatmap'), is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=1))
    net = net.eval().cuda()
    x = synth.synth_crops(2, 3, 256, 256, seed=11).cuda()
    outs, launches, npairs = [], [], []
    for mode in ('0', 'force'):
        monkeypatch.setenv('EGONET_AMD_PAIR', mode)
        net._engine = None
        eng = net._hip_engine()
        n0 = L.egn_launch_count()
        o = eng.forward(x, decode_mode=1)
        torch.cuda.synchronize()
        launches.append(L.egn_launch_count() - n0)
        meta = eng.program(x, 1).meta
        npairs.append(sum(1 for m in meta if m['kind'] == 'convpair'))
        if mode == '0':
            cfgs = {m['klass']: m['cfg'] for m in meta if m['kind'] == 'conv'}
            assert cfgs['conv3x3s1 192->192@16x16'] == 86 and cfgs['conv3x3s1 384->384@8x8'] == 82, cfgs
        outs.append(torch.utils._pytree.tree_leaves(o))
    assert npairs == [0, 24] and launches[0] - launches[1] == 24, (npairs, launches)
    assert len(outs[0]) == len(outs[1]) == 4
    for a, b in zip(*outs):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    pm = [m for m in meta if m['kind'] == 'convpair'][0]
    assert pm['klass'] == 'convpair3x3s1 192->192@16x16 + 384->384@8x8' and pm['flops'] > 0 and pm['bytes'] > 0
