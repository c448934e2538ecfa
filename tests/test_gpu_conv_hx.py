"""The f16-operand 3x3 / pad 1 convolution of the 32-MULTIPLE widths (csrc/conv_h.hip with CK = 32, precision = 'f16x'),
stride 1 and stride 2, element by element against float64.

As tests/test_gpu_conv_h.py and tests/test_gpu_conv_h2.py: the reference is ``train_checks.conv_ref64`` on the ROUNDED
operands -- x16 = f16(clamp(x, +-65504)), w16 = f16(w), both round-to-nearest-even -- so what is left is the kernel's own
arithmetic: a product of two f16 values is exact in fp32, only the fp32 summation and the epilogue round.  Bound:
conv_sweep.C_BOUND[0] (18) * U * A with A = ``conv_sweep.bound_A`` on |x16|, |w16|, |scale|, |shift|, |res|; the constant
was calibrated for direct fp32 sums of up to 9 * 384 terms and these are at most 9 * 256 long.  Non-zero magnitudes below
2^-14 are snapped to zero in the inputs.  H, W are the INPUT size.  The layers in the reference:
libs/model/heatmapModel/hrnet.py (fp32 torch calls): the BasicBlocks and the transition / fuse units of HRNet-W32, layer1's
3x3, the stem's second convolution and transition1."""
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
KIND_CONVHX = 14
RELU, NONE = engine.ACT_RELU, engine.ACT_NONE

# (n, h, w, cin, cout, residual, act, stride): the smallest shapes that reach every instance and every edge
SHAPES = [
    (1, 8, 8, 32, 32, 0, RELU, 1),               # one chunk, the 32-channel tile
    (3, 16, 12, 64, 64, 1, RELU, 1),             # the 64-channel tile; a partial tile in x
    (2, 8, 6, 256, 256, 1, RELU, 1),             # 8 chunks
    (5, 2, 2, 128, 128, 1, RELU, 1),             # many images per tile, a ragged group
    (2, 6, 5, 32, 64, 1, NONE, 1),               # Cin != Cout
    (2, 8, 8, 256, 48, 0, RELU, 1),              # transition1: the 48-channel tile on chunks of 32
    (2, 16, 12, 64, 128, 0, RELU, 2),
    (3, 9, 7, 32, 32, 0, NONE, 2),               # odd maps: the bottom and right padding exist
    (1, 4, 4, 128, 256, 0, RELU, 2),
    (2, 16, 16, 64, 64, 0, RELU, 2),             # the stem's second convolution
    (1, 12, 20, 256, 96, 0, RELU, 2),            # transition1: the 96-channel tile on chunks of 32
]
STRESS = (4, 16, 16, 64, 64, 1, RELU, 1)


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def _snap(t):
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def make(n, h, w, cin, cout, use_res, act, stride, seed=0, spike=None):
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + h * w + cin + cout + stride)
    x = _snap(cs.act_like(n, h, w, cin, cin, g))
    if spike is not None:
        x[0, h // 2, w // 2, 5] = spike
        x[n - 1, 0, 0, cin - 1] = -spike
    wt = _snap(cs.filt(cout, cin, 3, 3, g))
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g)
    ho, wo = out_hw(h, w, stride)
    res = torch.randn(n, ho, wo, cout, generator=g) if use_res else None
    buf = torch.full((GUARD + n * ho * wo * cout + GUARD,), CANARY).cuda()
    return dict(n=n, h=h, w=w, cin=cin, cout=cout, act=act, stride=stride, x=x.cuda(), wt=wt,
                wp=engine.pack_conv_weight_f16x(wt).cuda(), sc=sc.cuda(), sh=sh.cuda(),
                res=None if res is None else res.cuda(), buf=buf,
                y=buf[GUARD:GUARD + n * ho * wo * cout].view(n, ho, wo, cout))


def launch_direct(t, y=None):
    L = _lib.lib()
    y = t['y'] if y is None else y
    return L.egn_conv3x3_hx_f32(_lib.ptr(t['x']), _lib.ptr(t['wp']), _lib.ptr(t['sc']), _lib.ptr(t['sh']),
                                _lib.ptr(t['res']), _lib.ptr(y), t['n'], t['h'], t['w'], t['cin'], t['cout'], t['act'],
                                t['stride'], _lib.current_stream())


def run_direct(t, y=None):
    _lib.check(launch_direct(t, y), 'conv3x3_hx')
    torch.cuda.synchronize()
    return t['y'] if y is None else y


def reference(t):
    """(want, A) in float64 NHWC, on the device."""
    x16 = t['x'].clamp(-F16_MAX, F16_MAX).half().double().permute(0, 3, 1, 2)
    w16 = t['wt'].cuda().half().double()
    sc, sh = t['sc'].double(), t['sh'].double()
    res = None if t['res'] is None else t['res'].double().permute(0, 3, 1, 2)
    want = conv_ref64(x16, w16, t['stride'], 1, sc, sh, res, t['act'])
    A = cs.bound_A(x16, w16, t['stride'], 1, sc, sh, res, t['act'])
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


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d_%d-%d_r%d_a%d_s%d' % tuple(int(v) for v in s))
def test_kernel_against_float64_on_rounded_operands(shape):
    L = _lib.lib()
    n, h, w, cin, cout, use_res, act, stride = shape
    assert L.egn_conv3x3_hx_applies(n, h, w, cin, cin, cout, cout, int(use_res), act, stride) == 1
    t = make(*shape)
    y = check(t, str(shape)).clone()
    # two runs are bit-identical
    t['y'].fill_(CANARY)
    assert torch.equal(run_direct(t), y)


def test_inputs_beyond_the_f16_range_saturate():
    """An input of 1e6 enters the products as 65504 (not inf): the result is that of the clamped input, finite."""
    t = make(2, 8, 8, 32, 32, 0, NONE, 1, seed=3, spike=1.0e6)
    check(t, 'saturation')          # (``reference`` clamps before it rounds)
    assert float(t['y'].abs().max()) > 1.0e3         # the spikes are in the result


def _program(t, y, lanes=True):
    """One-op program on ``t`` writing ``y``; ``lanes``: inside a fork / join region, on lane 1."""
    L = _lib.lib()
    prog = ctypes.c_void_p(L.egn_program_create(8))
    assert prog
    refs = []
    for slot, ten in enumerate((t['x'], t['wp'], t['sc'], t['sh'], t['res'], y)):
        if ten is None:
            refs.append(_lib.NULL_REF)
            continue
        _lib.check(L.egn_program_bind(prog, slot, _lib.ptr(ten)))
        refs.append(_lib.Ref(slot, 0))
    if lanes:
        _lib.check(L.egn_program_fork(prog))
        _lib.check(L.egn_program_set_lane(prog, 1))
    _lib.check(L.egn_program_add_conv3x3_hx(prog, *refs, t['n'], t['h'], t['w'], t['cin'], t['cout'], t['act'],
                                            t['stride']), 'add')
    _lib.check(L.egn_program_tag(prog, b'the.f16x.op', 0.0, 0.0))
    if lanes:
        _lib.check(L.egn_program_join(prog))
    return prog


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[6]], ids=['s1_16x12', 's2_16x12'])
def test_program_op_equals_the_direct_entry_point(shape):
    L = _lib.lib()
    t = make(*shape, seed=1)
    want = run_direct(t).clone()
    n, h, w, cin, cout, use_res, act, stride = shape
    ho, wo = out_hw(h, w, stride)
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
        assert kind.value == KIND_CONVHX and tag.value == b'the.f16x.op'
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
        refs = [_lib.Ref(k, 0) for k in range(6)]
        none = list(refs)
        none[4] = _lib.NULL_REF
        assert L.egn_program_add_conv3x3_hx(prog, *none, n, h, w, 40, cout, RELU, stride) != 0
        assert L.egn_program_add_conv3x3_hx(prog, *none, n, h, w, 48, cout, RELU, stride) != 0
        assert L.egn_program_add_conv3x3_hx(prog, *none, n, h, w, cin, 192, RELU, stride) != 0
        assert L.egn_program_add_conv3x3_hx(prog, *none, n, h, w, cin, cout, engine.ACT_SIGMOID, stride) != 0
        assert L.egn_program_add_conv3x3_hx(prog, *none, n, h, w, cin, cout, RELU, 3) != 0
        assert L.egn_program_add_conv3x3_hx(prog, *refs, n, h, w, cin, cout, RELU, 2) != 0      # a residual at stride 2
        assert L.egn_program_num_ops(prog) == 3
    finally:
        L.egn_program_destroy(prog)


def test_direct_entry_point_refuses_what_the_predicate_refuses():
    L = _lib.lib()
    t = make(*SHAPES[0])
    args = [_lib.ptr(t[k]) for k in ('x', 'wp', 'sc', 'sh')]
    y, st = _lib.ptr(t['y']), _lib.current_stream()
    assert L.egn_conv3x3_hx_f32(*args, None, y, 1, 8, 8, 40, 32, RELU, 1, st) != 0
    assert L.egn_conv3x3_hx_f32(*args, None, y, 1, 8, 8, 48, 48, RELU, 1, st) != 0
    assert L.egn_conv3x3_hx_f32(*args, None, y, 1, 8, 8, 32, 32, engine.ACT_SIGMOID, 1, st) != 0
    assert L.egn_conv3x3_hx_f32(*args, None, y, 1, 1, 8, 32, 32, RELU, 1, st) != 0
    assert L.egn_conv3x3_hx_f32(*args, None, y, 1, 8, 8, 32, 32, RELU, 3, st) != 0
    assert L.egn_conv3x3_hx_f32(*args, y, y, 1, 8, 8, 32, 32, RELU, 2, st) != 0                # a residual at stride 2
    torch.cuda.synchronize()
    assert (t['buf'] == CANARY).all()


def test_replay_of_a_captured_op_in_a_process_of_its_own():
    """Graph replays stay out of the suite's own process (tests/graph_case.py's style)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'conv_hx_graph_case.py')],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'conv hx graph case ok' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_bit_identical_beside_two_busy_streams():
    """As tests/test_gpu_stress_streams.py does for the other families: every repetition beside a bandwidth hog and an
    MFMA hog reproduces the solo run bit for bit (the kernel waits for its loads with compiler-counted waits only)."""
    from test_gpu_stress_streams import _Hogs, _stress, REPS
    t = make(*STRESS, seed=2)

    def launch():
        _lib.check(launch_direct(t), 'conv3x3_hx')
    bad, overlapped, checks = _stress(launch, t['y'], _Hogs('conv'))
    print('conv3x3_hx %s: %d of %d repetitions differ; side streams busy at %d of %d checkpoints'
          % (STRESS, bad, REPS, overlapped, checks))
    assert overlapped >= checks // 2, 'the side streams drained: not a stress run'
    assert bad == 0, bad
