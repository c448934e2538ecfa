"""The packed filter layouts of the conv kernels: their names, the float64 host packers the inference engine uses, and
the device packers the training tape uses.

A layout is a contract between a packer and a kernel's load addresses; include/egonet_hip.h describes each one
(egn_conv_config_kind: the kinds; the pack entries; egn_pack_conv_weights_batch_f32: the descriptor's work units).
This module is the only place that maps a kind to a host packer, a C entry or a descriptor code.
"""
import torch

from . import _lib

# the filter kinds, the values egn_conv_config_kind returns
DIRECT, WINO2, WINO43, WINO4 = 0, 1, 2, 3

CK = 16                 # input channels per K chunk (EGN_CK in csrc/egn_internal.h)
H_CK, H_KS = 48, 14     # csrc/conv_h.hip: input channels per chunk, MFMA K steps of 32 per chunk (9 * 48 = 432 -> 448)
HX_CK = 32              # ... of its CK = 32 instances ('f16x'): 9 * 32 = 288, nine K steps, one per tap


def _round_up(v, m):
    return (v + m - 1) // m * m


# ---------------------------------------------------------------------------
# on the host
# ---------------------------------------------------------------------------
def pack_conv_weight(w):
    """[Cout,Cin,KH,KW] -> flat fp32 [nchunk][KH*KW][CK/4][CoutP][4]
    (ci = chunk*16 + quad*4 + r; zero padded)."""
    w = w.detach().to(torch.float32).cpu()
    cout, cin, kh, kw = w.shape
    coutp = _round_up(cout, 16)
    nchunk = (cin + CK - 1) // CK
    wp = torch.zeros(coutp, nchunk * CK, kh * kw, dtype=torch.float32)
    wp[:cout, :cin] = w.reshape(cout, cin, kh * kw)
    wp = wp.view(coutp, nchunk, CK // 4, 4, kh * kw).permute(1, 4, 2, 0, 3).contiguous()
    return wp.reshape(-1)


def wino_cot(cout):
    """Output channels per block (co-tile) of the Winograd kernels: 48 where Cout allows (the W48
    widths), else 32 (the W32 / Pedestrian widths and 64-channel layers); 0 = not supported
    (egn_wino_cot in csrc/egn_internal.h)."""
    return 48 if cout % 48 == 0 else (32 if cout % 32 == 0 else 0)


def pack_wino_weight(w):
    """[Cout,Cin,3,3] -> the Winograd F(2x2,3x3) filter U = G g G^T (float64, rounded once to
    fp32) in the layout conv_wino.hip stages through LDS:
    flat fp32 [co-tile = Cout/T][chunk = Cin/16][f = 4i+j][quad][T][4], T = wino_cot(Cout)
    (ci = chunk*16 + quad*4 + r), one contiguous slab (48 KB for T = 48) per (co-tile, chunk)."""
    w = w.detach().to(torch.float64).cpu()
    cout, cin, kh, kw = w.shape
    cot = wino_cot(cout)
    assert (kh, kw) == (3, 3) and cot and cin % CK == 0, w.shape
    G = torch.tensor([[1., 0., 0.], [.5, .5, .5], [.5, -.5, .5], [0., 0., 1.]], dtype=torch.float64)
    u = torch.einsum('ia,ocab,jb->ocij', G, w, G).to(torch.float32)        # [Cout,Cin,4,4]
    u = u.reshape(cout // cot, cot, cin // CK, CK // 4, 4, 16)             # ct, co, chunk, quad, r, f
    return u.permute(0, 2, 5, 3, 1, 4).contiguous().reshape(-1)


def pack_wino43_weight(w):
    """[Cout,Cin,3,3] -> the Winograd F(4x4,3x3) filter U = G g G^T (points 0, +-1, +-2; float64, rounded once to
    fp32) in the layout conv_wino43_kernel stages through LDS:
    flat fp32 [co-tile = Cout/48][K step = Cin/4][f = 6i+j][kq = ci % 4][48], one contiguous 27 KB slab per
    (co-tile, K step)."""
    w = w.detach().to(torch.float64).cpu()
    cout, cin, kh, kw = w.shape
    assert (kh, kw) == (3, 3) and cout % 48 == 0 and cin % 4 == 0, w.shape
    G = torch.tensor([[1 / 4., 0., 0.], [-1 / 6., -1 / 6., -1 / 6.], [-1 / 6., 1 / 6., -1 / 6.],
                      [1 / 24., 1 / 12., 1 / 6.], [1 / 24., -1 / 12., 1 / 6.], [0., 0., 1.]], dtype=torch.float64)
    u = torch.einsum('ia,ocab,jb->ocij', G, w, G).to(torch.float32)        # [Cout,Cin,6,6]
    u = u.reshape(cout // 48, 48, cin // 4, 4, 36)                          # ct, col, step, kq, f
    return u.permute(0, 2, 4, 3, 1).contiguous().reshape(-1)


def pack_wino4_weight(w):
    """[Cout,Cin,3,3] -> the Winograd F(4x4,3x3) filter U = G g G^T (float64, rounded once to fp32) in the layout
    conv_wino4_kernel's waves load straight into MFMA B registers (csrc/conv_wino4.hip), three dwordx4 per wave
    and k-group: flat fp32 [co-tile = Cout/48][stage = Cin/8][k-group g][wave 0..11][q 0..2][lane = 16 kq + li][4]
    where value p = 4 q + r (p = 3 pl + nt < 9, the rest is padding) is point 3 wave + pl, co = 48 ct + 16 nt + li,
    ci = 8 stage + 4 g + kq."""
    w = w.detach().to(torch.float64).cpu()
    cout, cin, kh, kw = w.shape
    assert (kh, kw) == (3, 3) and cout % 48 == 0 and cin % 8 == 0, w.shape
    G = torch.tensor([[1 / 4., 0., 0.], [-1 / 6., -1 / 6., -1 / 6.], [-1 / 6., 1 / 6., -1 / 6.],
                      [1 / 24., 1 / 12., 1 / 6.], [1 / 24., -1 / 12., 1 / 6.], [0., 0., 1.]], dtype=torch.float64)
    u = torch.einsum('ia,ocab,jb->ocij', G, w, G).to(torch.float32).reshape(cout, cin, 36)
    #   co = (ct, nt, li)          ci = (stage, g, kq)        pt = (wave, pl)
    u = u.reshape(cout // 48, 3, 16, cin // 8, 2, 4, 12, 3)   # ct nt li stage g kq wave pl
    u = u.permute(0, 3, 4, 6, 7, 1, 5, 2).contiguous()        # ct stage g wave pl nt kq li
    ct, st = cout // 48, cin // 8
    u = u.reshape(ct, st, 2, 12, 9, 64)                        # ... p = 3 pl + nt, lane = 16 kq + li
    pad = torch.zeros(ct, st, 2, 12, 12, 64, dtype=torch.float32)
    pad[:, :, :, :, :9] = u
    return pad.reshape(ct, st, 2, 12, 3, 4, 64).permute(0, 1, 2, 3, 4, 6, 5).contiguous().reshape(-1)   # q lane r


def pack_conv_weight_f16(w):
    """[Cout,Cin,3,3] -> the filter rounded ONCE to f16 (``w.half()``: round-to-nearest-even) in the layout the waves of
    csrc/conv_h.hip load straight into MFMA B registers, 16 bytes per lane:
    flat f16 [co-tile = Cout/16][chunk = Cin/48][step 0..13][lane = 16 g + li][j 0..7] holding W[16 ct + li][48 chunk + c][tap]
    at k = 32 step + 8 g + j = 48 tap + c; k >= 432 is zero padding.  Returned as a flat fp32 VIEW of those bytes (the
    weights blob is one fp32 tensor); ``unpack_conv_weight_f16`` is the inverse."""
    w = w.detach().to(torch.float32).cpu()
    cout, cin, kh, kw = w.shape
    assert (kh, kw) == (3, 3) and cout % 16 == 0 and cin % H_CK == 0, w.shape
    ct, nch = cout // 16, cin // H_CK
    u = w.half().reshape(ct, 16, nch, H_CK, 9).permute(0, 2, 4, 3, 1).reshape(ct, nch, 9 * H_CK, 16)   # ct chunk k li
    pad = torch.zeros(ct, nch, H_KS * 32, 16, dtype=torch.float16)
    pad[:, :, :9 * H_CK] = u
    pad = pad.reshape(ct, nch, H_KS, 4, 8, 16).permute(0, 1, 2, 3, 5, 4).contiguous()                   # ... g li j
    return pad.reshape(-1).view(torch.float32)


def unpack_conv_weight_f16(packed, cout, cin):
    """The f16 filter [Cout,Cin,3,3] a ``pack_conv_weight_f16`` result holds."""
    ct, nch = cout // 16, cin // H_CK
    u = packed.view(torch.float16).reshape(ct, nch, H_KS, 4, 16, 8).permute(0, 1, 2, 3, 5, 4)            # ... g j li
    u = u.reshape(ct, nch, H_KS * 32, 16)[:, :, :9 * H_CK].reshape(ct, nch, 9, H_CK, 16)
    return u.permute(0, 4, 1, 3, 2).reshape(cout, cin, 3, 3).contiguous()


def pack_conv_weight_f16x(w):
    """[Cout,Cin,3,3] -> the filter rounded ONCE to f16 (round-to-nearest-even) in the layout the CK = 32 instances of
    csrc/conv_h.hip load (precision = 'f16x'): flat f16 [co-tile = Cout/16][chunk = Cin/32][tap 0..8][lane = 16 g + li][j 0..7]
    holding W[16 ct + li][32 chunk + 8 g + j][tap] -- K step = tap, lane group = channel group, no padding.  Returned as a
    flat fp32 VIEW of those bytes; ``unpack_conv_weight_f16x`` is the inverse."""
    w = w.detach().to(torch.float32).cpu()
    cout, cin, kh, kw = w.shape
    assert (kh, kw) == (3, 3) and cout % 16 == 0 and cin % HX_CK == 0, w.shape
    ct, nch = cout // 16, cin // HX_CK
    u = w.half().reshape(ct, 16, nch, 4, 8, 9).permute(0, 2, 5, 3, 1, 4).contiguous()     # ct chunk tap g li j
    return u.reshape(-1).view(torch.float32)


def unpack_conv_weight_f16x(packed, cout, cin):
    """The f16 filter [Cout,Cin,3,3] a ``pack_conv_weight_f16x`` result holds."""
    ct, nch = cout // 16, cin // HX_CK
    u = packed.view(torch.float16).reshape(ct, nch, 9, 4, 16, 8).permute(0, 4, 1, 3, 5, 2)               # ct li chunk g j tap
    return u.reshape(cout, cin, 3, 3).contiguous()


def pack_for_kind(w, kind):
    """The filter in the layout the kernels of a tile-configuration KIND read (tuner.kind_of), packed on the host."""
    if kind == WINO4:
        return pack_wino4_weight(w)
    return pack_wino43_weight(w) if kind == WINO43 else (pack_wino_weight(w) if kind == WINO2 else pack_conv_weight(w))


# ---------------------------------------------------------------------------
# on the device (csrc/filter_pack.h)
# ---------------------------------------------------------------------------
# kind -> (descriptor code without the direction bit, floats per work unit of egn_pack_conv_weights_batch_f32)
DEVICE_PACK = {DIRECT: (0, 4), WINO2: (2, 64), WINO4: (4, 48)}


def device_floats(kind, shape, dgrad):
    """Floats of the device-packed filter of a [Cout,Cin,KH,KW] weight (``dgrad``: the data-gradient filter)."""
    cout, cin, kh, kw = shape
    L, nfl = _lib.lib(), 0
    if kind == DIRECT:
        nfl = L.egn_packed_weight_floats(cout, cin, kh, kw, dgrad)
    elif kind in (WINO2, WINO4) and (kh, kw) == (3, 3):
        nfl = (L.egn_wino_weight_floats if kind == WINO2 else L.egn_wino4_pack_weight_floats)(cout, cin, dgrad)
    if nfl <= 0:
        raise ValueError('no packed layout %r for a %s filter' % (kind, tuple(shape)))
    return nfl


def pack_on_device(weight, kind, dgrad, dst, stream):
    """Pack the device tensor ``weight`` into ``dst`` (``device_floats`` floats) on ``stream``."""
    cout, cin, kh, kw = weight.shape
    L, w, d = _lib.lib(), _lib.ptr(weight), _lib.ptr(dst)
    if kind == DIRECT:
        _lib.check(L.egn_pack_conv_weight_f32(w, cout, cin, kh, kw, dgrad, d, stream), 'pack')
    elif kind == WINO2:
        _lib.check(L.egn_wino_pack_weight_f32(w, cout, cin, dgrad, d, stream), 'wino pack')
    elif kind == WINO4:
        _lib.check(L.egn_wino4_pack_weight_f32(w, cout, cin, dgrad, d, stream), 'wino4 pack')
    else:
        raise ValueError('no device packer for filter kind %r' % (kind,))
