"""The f16-operand 3x3 / STRIDE 2 / pad 1 convolution (csrc/conv_h.hip with S = 2, precision = 'f16s2') element by element
against float64.

As tests/test_gpu_conv_h.py: the reference is ``train_checks.conv_ref64`` on the ROUNDED operands -- x16 = f16(clamp(x,
+-65504)), w16 = f16(w), both round-to-nearest-even -- so what is left is the kernel's own arithmetic.  A product of two
f16 values is exact in fp32 (22 significant bits); only the fp32 summation and the epilogue round.  Bound:
conv_sweep.C_BOUND[0] (18) * U * A with A = ``conv_sweep.bound_A`` at stride 2 on |x16|, |w16|, |scale|, |shift|: derived,
the same constant as for the fp32 direct sums of the same length.  Non-zero magnitudes below 2^-14 are snapped to zero in
the inputs.  H, W are the INPUT size; the output is (H - 1) / 2 + 1 x (W - 1) / 2 + 1.  The layers in the reference:
libs/model/heatmapModel/hrnet.py, the stride-2 units of the transition and fuse layers (fp32 torch calls)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import conv_sweep as cs
from train_checks import conv_ref64
from egonet_amd import _lib, engine

pytestmark = pytest.mark.gpu
F16_MAX = 65504.0
CANARY = -12345.0
GUARD = 4096          # floats in front of and behind y
KIND_CONVH2 = 13

# (n, h, w, cin, cout, act): each the smallest shape that has its edge
SHAPES = [
    (1, 8, 8, 48, 48, engine.ACT_RELU),            # one tile
    (3, 16, 16, 48, 96, engine.ACT_NONE),          # Cin != Cout
    (2, 12, 20, 96, 192, engine.ACT_RELU),         # partial tiles in both axes (6 x 10 output)
    (2, 7, 9, 48, 48, engine.ACT_RELU),            # odd sizes: the bottom and right padding exist
    (5, 4, 4, 192, 384, engine.ACT_NONE),          # several images per tile, a ragged image group
    (4, 2, 2, 96, 384, engine.ACT_RELU),           # 1 x 1 outputs
    (1, 32, 32, 96, 96, engine.ACT_NONE),          # several tiles: the stress shape
]


def out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def _snap(t):
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def make(n, h, w, cin, cout, act, seed=0, spike=None):
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + h * w + cin + cout)
    x = _snap(cs.act_like(n, h, w, cin, cin, g))
    if spike is not None:
        x[0, h // 2, w // 2, 5] = spike
        x[n - 1, 0, 0, cin - 1] = -spike
    wt = _snap(cs.filt(cout, cin, 3, 3, g))
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g)
    ho, wo = out_hw(h, w)
    buf = torch.full((GUARD + n * ho * wo * cout + GUARD,), CANARY).cuda()
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, act=act, x=x.cuda(), wt=wt, wp=engine.pack_conv_weight_f16(wt).cuda(),
                sc=sc.cuda(), sh=sh.cuda(), buf=buf, y=buf[GUARD:GUARD + n * ho * wo * cout].view(n, ho, wo, cout))


def run_direct(t, y=None):
    L = _lib.lib()
    y = t['y'] if y is None else y
    _lib.check(L.egn_conv3x3s2_h_f32(_lib.ptr(t['x']), _lib.ptr(t['wp']), _lib.ptr(t['sc']), _lib.ptr(t['sh']), _lib.ptr(y),
                                     t['n'], t['h'], t['w'], t['cin'], t['cout'], t['act'], _lib.current_stream()),
               'conv3x3s2_h')
    torch.cuda.synchronize()
    return y


def reference(t):
    """(want, A) in float64 NHWC, on the device."""
    x16 = t['x'].clamp(-F16_MAX, F16_MAX).half().double().permute(0, 3, 1, 2)
    w16 = t['wt'].cuda().half().double()
    sc, sh = t['sc'].double(), t['sh'].double()
    want = conv_ref64(x16, w16, 2, 1, sc, sh, None, t['act'])
    A = cs.bound_A(x16, w16, 2, 1, sc, sh, None, t['act'])
    return want.permute(0, 2, 3, 1), A.permute(0, 2, 3, 1)


def check(t, label):
    y = run_direct(t)
    want, A = reference(t)
    assert want.shape == y.shape, (label, want.shape, y.shape)
    assert torch.isfinite(y).all(), label
    r = cs.ratio(y, want, A)
    print('%s: worst |y - y64| / (U A) = %.3f (bound %.0f)' % (label, float(r.max()), cs.C_BOUND[0]))
    assert float(r.max()) <= cs.C_BOUND[0], (label, float(r.max()))
    # nothing outside the tensor was written
    assert (t['buf'][:GUARD] == CANARY).all() and (t['buf'][-GUARD:] == CANARY).all(), label
    return y


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d_%d-%d_a%d' % tuple(int(v) for v in s))
def test_kernel_against_float64_on_rounded_operands(shape):
    L = _lib.lib()
    n, h, w, cin, cout, act = shape
    assert L.egn_conv3x3s2_h_applies(n, h, w, cin, cin, cout, cout, act) == 1
    t = make(*shape)
    y = check(t, str(shape)).clone()
    # two runs are bit-identical
    t['y'].fill_(CANARY)
    assert torch.equal(run_direct(t), y)


def test_inputs_beyond_the_f16_range_saturate():
    """An input of 1e6 enters the products as 65504 (not inf): the result is that of the clamped input, finite."""
    t = make(2, 8, 8, 48, 48, engine.ACT_NONE, seed=3, spike=1.0e6)
    check(t, 'saturation')          # (``reference`` clamps before it rounds)
    assert float(t['y'].abs().max()) > 1.0e3         # the spikes are in the result


def _program(t, y, lanes=True):
    """One-op program on ``t`` writing ``y``; ``lanes``: inside a fork / join region, on lane 1."""
    L = _lib.lib()
    prog = ctypes.c_void_p(L.egn_program_create(8))
    assert prog
    refs = []
    for slot, ten in enumerate((t['x'], t['wp'], t['sc'], t['sh'], y)):
        _lib.check(L.egn_program_bind(prog, slot, _lib.ptr(ten)))
        refs.append(_lib.Ref(slot, 0))
    if lanes:
        _lib.check(L.egn_program_fork(prog))
        _lib.check(L.egn_program_set_lane(prog, 1))
    _lib.check(L.egn_program_add_conv3x3s2_h(prog, *refs, t['n'], t['h'], t['w'], t['cin'], t['cout'], t['act']), 'add')
    _lib.check(L.egn_program_tag(prog, b'the.f16s2.op', 0.0, 0.0))
    if lanes:
        _lib.check(L.egn_program_join(prog))
    return prog


@pytest.mark.parametrize('shape', [SHAPES[2], SHAPES[4]], ids=['12x20', '4x4'])
def test_program_op_equals_the_direct_entry_point(shape):
    L = _lib.lib()
    t = make(*shape, seed=1)
    want = run_direct(t).clone()
    n, h, w, cin, cout = shape[:5]
    ho, wo = out_hw(h, w)
    st = _lib.current_stream()
    # plain: one launch
    y = torch.full_like(want, CANARY)
    prog = _program(t, y, lanes=False)
    try:
        n0 = L.egn_launch_count()
        _lib.check(L.egn_program_run(prog, st), 'run')
        torch.cuda.synchronize()
        assert torch.equal(y, want) and L.egn_launch_count() - n0 == 1
        kind, flops, nbytes = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        tag = ctypes.create_string_buffer(32)
        _lib.check(L.egn_program_op_info(prog, 0, kind, flops, nbytes, tag, 32))
        assert kind.value == KIND_CONVH2 and tag.value == b'the.f16s2.op'
        assert flops.value == 2.0 * 9 * n * ho * wo * cout * cin
    finally:
        L.egn_program_destroy(prog)
    # inside a fork / join lane, timed
    y = torch.full_like(want, CANARY)
    prog = _program(t, y, lanes=True)
    try:
        ms = (ctypes.c_float * 3)()
        n0 = L.egn_launch_count()
        _lib.check(L.egn_program_run_timed(prog, st, ms, 3), 'run_timed')
        torch.cuda.synchronize()
        assert torch.equal(y, want) and ms[1] > 0.0 and L.egn_launch_count() - n0 == 1
        # shapes the predicate refuses are refused here too
        refs = [_lib.Ref(k, 0) for k in range(5)]
        assert L.egn_program_add_conv3x3s2_h(prog, *refs, n, h, w, 40, cout, 1) != 0
        assert L.egn_program_add_conv3x3s2_h(prog, *refs, n, h, w, cin, cout, engine.ACT_SIGMOID) != 0
        assert L.egn_program_num_ops(prog) == 3
    finally:
        L.egn_program_destroy(prog)


def test_direct_entry_point_refuses_what_the_predicate_refuses():
    L = _lib.lib()
    t = make(*SHAPES[0])
    args = [_lib.ptr(t[k]) for k in ('x', 'wp', 'sc', 'sh', 'y')]
    st = _lib.current_stream()
    assert L.egn_conv3x3s2_h_f32(*args, 1, 8, 8, 40, 48, engine.ACT_RELU, st) != 0
    assert L.egn_conv3x3s2_h_f32(*args, 1, 8, 8, 48, 48, engine.ACT_SIGMOID, st) != 0
    assert L.egn_conv3x3s2_h_f32(*args, 1, 1, 8, 48, 48, engine.ACT_RELU, st) != 0
    torch.cuda.synchronize()
    assert (t['buf'] == CANARY).all()


def test_replay_of_a_captured_op_in_a_process_of_its_own():
    """Graph replays stay out of the suite's own process (tests/graph_case.py's style)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_h2_graph_case.py')],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'conv h2 graph case ok' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_bit_identical_beside_two_busy_streams():
    """As tests/test_gpu_stress_streams.py does for the other families: every repetition beside a bandwidth hog and an
    MFMA hog reproduces the solo run bit for bit (the kernel waits for its loads with compiler-counted waits only)."""
    from test_gpu_stress_streams import _Hogs, _stress, REPS
    t = make(*SHAPES[6], seed=2)

    def launch():
        L = _lib.lib()
        _lib.check(L.egn_conv3x3s2_h_f32(_lib.ptr(t['x']), _lib.ptr(t['wp']), _lib.ptr(t['sc']), _lib.ptr(t['sh']),
                                         _lib.ptr(t['y']), t['n'], t['h'], t['w'], t['cin'], t['cout'], t['act'],
                                         _lib.current_stream()), 'conv3x3s2_h')
    bad, overlapped, checks = _stress(launch, t['y'], _Hogs('conv'))
    print('conv3x3s2_h %s: %d of %d repetitions differ; side streams busy at %d of %d checkpoints'
          % (SHAPES[6], bad, REPS, overlapped, checks))
    assert overlapped >= checks // 2, 'the side streams drained: not a stress run'
    assert bad == 0, bad
