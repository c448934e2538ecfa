"""f16 STORAGE between two f16-operand 3x3 convolutions (csrc/conv_h.hip: ConvHArgs::x16 / y16, activations = 'f16'),
bit for bit against the EXISTING entry points -- no tolerance anywhere in this file.

The claim: a reader of the family rounds every fp32 element of x to f16 (clamp to +-65504, nearest-even)
while it stages it.  With ``y_f16`` the producer applies that very rounding in its epilogue and stores f16; with ``x_f16``
the reader stages the f16 as it lies.  So
  1. new(x_f16 = 1) on  f16(clamp(x))          ==  old on x                      (fp32 outputs, ``torch.equal``)
  2. new(y_f16 = 1) on  x                      ==  f16(clamp(old on x))          (the int16 views are equal)
  3. both flags                                ==  f16(clamp(old on x))
and a chain producer -> reader with the tensor between them in f16 equals the fp32-storage chain.  Canaries in front of
and behind every y: the f16 y is half the size, a stray 4-byte stride would overrun it.  H, W are the INPUT size."""
import ctypes

import pytest
import torch

import conv_sweep as cs
from egonet_amd import _lib, engine

pytestmark = pytest.mark.gpu
F16_MAX = 65504.0
CANARY = -1234.0          # (exact in f16 and in fp32)
RELU, NONE = engine.ACT_RELU, engine.ACT_NONE

# (ck, (n, h, w, cin, cout, residual, act, stride)): the smallest shapes that reach every instance and every edge
SHAPES = [
    (32, (1, 8, 8, 32, 32, 0, RELU, 1)),             # the 32-channel tile
    (32, (3, 16, 12, 64, 64, 1, RELU, 1)),           # a partial tile in x
    (32, (2, 8, 6, 256, 256, 1, RELU, 1)),           # 8 chunks
    (32, (5, 2, 2, 128, 128, 1, RELU, 1)),           # many images per tile, a ragged group
    (32, (2, 8, 8, 256, 48, 0, RELU, 1)),            # the 48-channel tile on chunks of 32
    (32, (3, 9, 7, 32, 32, 0, NONE, 2)),             # odd maps
    (32, (2, 16, 12, 64, 128, 0, RELU, 2)),          # stride 2
    (32, (1, 12, 20, 256, 96, 0, RELU, 2)),          # the 96-channel tile at stride 2
    (48, (2, 8, 8, 48, 48, 1, RELU, 1)),             # the 48-channel tile
    (48, (3, 16, 12, 96, 96, 1, RELU, 1)),           # the 96-channel tile, a partial tile
    (48, (5, 2, 2, 384, 384, 1, RELU, 1)),           # many images per tile
    (48, (1, 9, 7, 48, 96, 0, RELU, 2)),             # odd maps at stride 2
    (48, (2, 4, 4, 192, 384, 0, NONE, 2)),           # stride 2
]


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def guarded(numel, dtype):
    """(buffer, view of ``numel`` elements) with canaries in front of and behind the view: at least as many as the view
    holds, so that a writer striding 4 bytes through a 2-byte tensor lands in them."""
    guard = max(4096, numel)
    buf = torch.full((guard + numel + guard,), CANARY, dtype=dtype, device='cuda')
    return buf, buf[guard:guard + numel], guard


def intact(buf, guard):
    return bool((buf[:guard] == CANARY).all()) and bool((buf[-guard:] == CANARY).all())


def make(ck, shape, seed=0, spike=None, gain=1.0):
    n, h, w, cin, cout, use_res, act, stride = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + h * w + cin + cout + stride + ck)
    x = cs.act_like(n, h, w, cin, cin, g)
    if spike is not None:
        x[0, h // 2, w // 2, 5] = spike
        x[n - 1, 0, 0, cin - 1] = -spike
    wt = cs.filt(cout, cin, 3, 3, g)
    sc = (torch.rand(cout, generator=g) + 0.5) * gain
    sh = torch.randn(cout, generator=g)
    ho, wo = out_hw(h, w, stride)
    res = torch.randn(n, ho, wo, cout, generator=g).cuda() if use_res else None
    pack = engine.pack_conv_weight_f16x if ck == 32 else engine.pack_conv_weight_f16
    x = x.cuda().contiguous()
    return dict(ck=ck, n=n, h=h, w=w, cin=cin, cout=cout, act=act, stride=stride, ho=ho, wo=wo, x=x,
                x16=x.clamp(-F16_MAX, F16_MAX).half().contiguous(), wp=pack(wt).cuda(), sc=sc.cuda(), sh=sh.cuda(), res=res)


def run_old(t, x=None, res=None):
    """The existing entry point of (ck, stride) on fp32 ``x``: a fresh fp32 [n, ho, wo, cout]."""
    L = _lib.lib()
    x = t['x'] if x is None else x
    y = torch.full((t['n'], t['ho'], t['wo'], t['cout']), CANARY, device='cuda')
    head = [_lib.ptr(x), _lib.ptr(t['wp']), _lib.ptr(t['sc']), _lib.ptr(t['sh'])]
    dims = [t['n'], t['h'], t['w'], t['cin'], t['cout'], t['act']]
    st = _lib.current_stream()
    if t['ck'] == 32:
        rc = L.egn_conv3x3_hx_f32(*head, _lib.ptr(res), _lib.ptr(y), *dims, t['stride'], st)
    elif t['stride'] == 1:
        rc = L.egn_conv3x3_h_f32(*head, _lib.ptr(res), _lib.ptr(y), *dims, st)
    else:
        assert res is None
        rc = L.egn_conv3x3s2_h_f32(*head, _lib.ptr(y), *dims, st)
    _lib.check(rc, 'old entry')
    torch.cuda.synchronize()
    return y


def run_new(t, x_f16, y_f16, x=None, res=None):
    """egn_conv3x3_h16_f32 into a guarded y of the dtype ``y_f16`` says; returns (y as [n, ho, wo, cout], buf, guard)."""
    L = _lib.lib()
    if x is None:
        x = t['x16'] if x_f16 else t['x']
    assert x.dtype == (torch.float16 if x_f16 else torch.float32)
    numel = t['n'] * t['ho'] * t['wo'] * t['cout']
    buf, y, guard = guarded(numel, torch.float16 if y_f16 else torch.float32)
    _lib.check(L.egn_conv3x3_h16_f32(_lib.ptr(x), _lib.ptr(t['wp']), _lib.ptr(t['sc']), _lib.ptr(t['sh']), _lib.ptr(res),
                                     _lib.ptr(y), t['n'], t['h'], t['w'], t['cin'], t['cout'], t['act'], t['stride'],
                                     t['ck'], int(x_f16), int(y_f16), _lib.current_stream()), 'h16 entry')
    torch.cuda.synchronize()
    return y.view(t['n'], t['ho'], t['wo'], t['cout']), buf, guard


def as_f16(y):
    return y.clamp(-F16_MAX, F16_MAX).half()


def same_bits(a, b):
    bits = torch.int16 if a.dtype == torch.float16 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


@pytest.mark.parametrize('ck,shape', SHAPES, ids=lambda s: str(s) if isinstance(s, int) else
                         '%dx%dx%d_%d-%d_r%d_a%d_s%d' % tuple(int(v) for v in s))
def test_f16_storage_keeps_the_bits_of_the_existing_entry_points(ck, shape):
    L = _lib.lib()
    n, h, w, cin, cout, use_res, act, stride = shape
    t = make(ck, shape)
    assert L.egn_conv3x3_h16_applies(n, h, w, cin, cin, cout, cout, int(use_res), act, stride, ck, 1, 0) == 1
    assert L.egn_conv3x3_h16_applies(n, h, w, cin, cin, cout, cout, 0, act, stride, ck, 1, 1) == 1
    old = run_old(t, res=t['res'])
    old_plain = run_old(t) if use_res else old
    # both flags 0: the existing entry point's bits
    y, buf, guard = run_new(t, 0, 0, res=t['res'])
    assert same_bits(y, old) and intact(buf, guard), 'flags 0'
    # 1. f16 input, fp32 output, with the residual where the shape has one
    y, buf, guard = run_new(t, 1, 0, res=t['res'])
    assert same_bits(y, old) and intact(buf, guard), 'x_f16'
    # 2. f16 output (never with a residual)
    y2, buf, guard = run_new(t, 0, 1)
    assert same_bits(y2, as_f16(old_plain)) and intact(buf, guard), 'y_f16'
    # 3. both
    y3, buf, guard = run_new(t, 1, 1)
    assert same_bits(y3, as_f16(old_plain)) and intact(buf, guard), 'x_f16 and y_f16'
    # 4. two runs are bit-identical
    again, buf, guard = run_new(t, 1, 1)
    assert same_bits(again, y3) and intact(buf, guard), 'second run'
    again, buf, guard = run_new(t, 1, 0, res=t['res'])
    assert same_bits(again, old) and intact(buf, guard), 'second run, x_f16'
    # f16 output beside a residual is refused, and nothing is written
    if use_res:
        numel = n * t['ho'] * t['wo'] * cout
        buf, yv, guard = guarded(numel, torch.float16)
        assert L.egn_conv3x3_h16_f32(_lib.ptr(t['x']), _lib.ptr(t['wp']), _lib.ptr(t['sc']), _lib.ptr(t['sh']),
                                     _lib.ptr(t['res']), _lib.ptr(yv), n, h, w, cin, cout, act, stride, ck, 0, 1,
                                     _lib.current_stream()) != 0
        torch.cuda.synchronize()
        assert bool((buf == CANARY).all())


def test_outputs_beyond_the_f16_range_are_stored_saturated():
    """Input spikes of 1e6 and a scale that drives outputs past 65504: the stored f16 is +-65504, never inf, and a reader
    of it computes what the reader of the fp32 tensor computes (which clamps while it stages)."""
    shape = (2, 8, 8, 32, 32, 0, NONE, 1)
    t = make(32, shape, seed=3, spike=1.0e6, gain=1.0e3)
    old = run_old(t)
    assert float(old.max()) > F16_MAX and float(old.min()) < -F16_MAX and bool(torch.isfinite(old).all())
    y16, buf, guard = run_new(t, 0, 1)
    assert intact(buf, guard)
    assert bool(torch.isfinite(y16).all()) and float(y16.max()) == F16_MAX and float(y16.min()) == -F16_MAX
    assert same_bits(y16, as_f16(old))
    y16b, buf, guard = run_new(t, 1, 1)
    assert same_bits(y16b, y16) and intact(buf, guard)
    # the consumer: a second layer of the same shape reading the tensor
    t2 = make(32, shape, seed=4)
    want = run_old(t2, x=old)
    got, buf, guard = run_new(t2, 1, 0, x=y16.contiguous())
    assert same_bits(got, want) and intact(buf, guard)
    assert bool(torch.isfinite(want).all())


def _two_op_program(t1, t2, mid, y, f16):
    """conv1 (t1: x -> mid) and conv2 (t2: mid -> y, residual x) on lane 1 of a fork / join region.  ``f16``: ``mid`` is
    stored as f16, both ops through egn_program_add_conv3x3_h16; else fp32 storage through the existing add entries."""
    L = _lib.lib()
    prog = ctypes.c_void_p(L.egn_program_create(12))
    assert prog
    tensors = (t1['x'], t1['wp'], t1['sc'], t1['sh'], mid, t2['wp'], t2['sc'], t2['sh'], y)
    for slot, ten in enumerate(tensors):
        _lib.check(L.egn_program_bind(prog, slot, _lib.ptr(ten)))
    R = [_lib.Ref(k, 0) for k in range(len(tensors))]
    dims = (t1['n'], t1['h'], t1['w'], t1['cin'], t1['cout'])
    _lib.check(L.egn_program_fork(prog))
    _lib.check(L.egn_program_set_lane(prog, 1))
    if f16:
        _lib.check(L.egn_program_add_conv3x3_h16(prog, R[0], R[1], R[2], R[3], _lib.NULL_REF, R[4], *dims, RELU, 1, t1['ck'],
                                                 0, 1), 'add conv1')
        _lib.check(L.egn_program_add_conv3x3_h16(prog, R[4], R[5], R[6], R[7], R[0], R[8], *dims, RELU, 1, t1['ck'], 1, 0),
                   'add conv2')
    elif t1['ck'] == 48:
        _lib.check(L.egn_program_add_conv3x3_h(prog, R[0], R[1], R[2], R[3], _lib.NULL_REF, R[4], *dims, RELU), 'add conv1')
        _lib.check(L.egn_program_add_conv3x3_h(prog, R[4], R[5], R[6], R[7], R[0], R[8], *dims, RELU), 'add conv2')
    else:
        _lib.check(L.egn_program_add_conv3x3_hx(prog, R[0], R[1], R[2], R[3], _lib.NULL_REF, R[4], *dims, RELU, 1), 'add conv1')
        _lib.check(L.egn_program_add_conv3x3_hx(prog, R[4], R[5], R[6], R[7], R[0], R[8], *dims, RELU, 1), 'add conv2')
    _lib.check(L.egn_program_join(prog))
    return prog


@pytest.mark.parametrize('ck,kind,shape', [(48, 12, (2, 8, 8, 48, 48, 0, RELU, 1)), (32, 14, (3, 16, 12, 64, 64, 0, RELU, 1))],
                         ids=['ck48', 'ck32'])
def test_two_op_program_with_f16_storage_between_the_ops(ck, kind, shape):
    """A BasicBlock: conv1 (y16) -> conv2 (x16, the block's input as residual), inside a fork / join region on lane 1."""
    L = _lib.lib()
    t1, t2 = make(ck, shape, seed=5), make(ck, shape, seed=6)
    n, h, w, c = shape[0], shape[1], shape[2], shape[3]
    numel = n * h * w * c
    st = _lib.current_stream()
    out = {}
    for f16 in (False, True):
        mbuf, mid, mguard = guarded(numel, torch.float16 if f16 else torch.float32)
        ybuf, y, yguard = guarded(numel, torch.float32)
        prog = _two_op_program(t1, t2, mid, y, f16)
        try:
            n0 = L.egn_launch_count()
            _lib.check(L.egn_program_run(prog, st), 'run')
            torch.cuda.synchronize()
            assert L.egn_launch_count() - n0 == 2
            assert intact(mbuf, mguard) and intact(ybuf, yguard)
            kinds, nbytes = [], []
            for i in range(L.egn_program_num_ops(prog)):
                k, fl, nb = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
                tag = ctypes.create_string_buffer(32)
                _lib.check(L.egn_program_op_info(prog, i, k, fl, nb, tag, 32))
                if k.value in (12, 13, 14):
                    kinds.append(k.value)
                    nbytes.append(nb.value)
                    assert fl.value == 2.0 * 9 * numel * c
            assert kinds == [kind, kind]
            wbytes = 2.0 * 9 * c * c
            if f16:      # conv1: x 4 + y 2 bytes; conv2: x 2 + y 4 + residual 4
                assert nbytes == [numel * 6.0 + wbytes, numel * 10.0 + wbytes]
            else:
                assert nbytes == [numel * 8.0 + wbytes, numel * 12.0 + wbytes]
            out[f16] = (mid.clone(), y.clone())
        finally:
            L.egn_program_destroy(prog)
    assert same_bits(out[True][0], as_f16(out[False][0]))
    assert same_bits(out[True][1], out[False][1])
    # and the fp32 chain is what the direct entry points compute
    want = run_old(t2, x=run_old(t1), res=t1['x'])
    assert same_bits(out[False][1].view_as(want), want)
