"""The weight-gradient requests the product makes, a supplement for every kernel no product request selects, the
inputs and the element-wise bound of the sweep.

Helper module of tests/test_wgrad_sweep_cpu.py and tests/test_gpu_wgrad_sweep.py (imported, not a conftest): the
companion of tests/conv_sweep.py for the third conv family of the training step.  ``egn_conv2d_wgrad_plan_query``
says which row of the dispatch table (csrc/conv_wgrad.hip: kWgradTable) a request selects, with which tile, split
count, reduce width and slab order.

A request is a dict:
  key   (n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad): what a caller passes to egn_conv2d_wgrad_f32
  src   where it was seen (model / batch / layer, or 'supplement: why')
"""
import ctypes as C

import numpy as np
import torch

from egonet_amd import _lib, configs

import conv_sweep
from conv_sweep import U, act_like, ratio                    # noqa: F401  (re-exported to the two test modules)

PLAN_FIELDS = ('row', 'form', 'TH', 'TW', 'TNB', 'co_tiles', 'ci_tiles', 'ntiles', 'tiles_per_split', 'nsplit',
               'lanes', 'frag', 'lds', 'shrink_tnb', 'shrink_th', 'shrink_tw')
FORM_NAMES = {0: 'direct', 1: 'Winograd 8x16', 2: 'Winograd pairs'}
BATCHES = (1, 2, 3)
LIFTER_ROWS = (1, 7, 100)

# |dw - dw64| <= C_BOUND[form] * U * g(K) * A on every element of [Cout, Cin, KH, KW], K = N Ho Wo, g = 1.
#   direct form:   A = wgrad_ref64(|x|, |dy|), per element
#   Winograd form: A = that, summed over the nine taps of its (co, ci): G^T dU G cancels terms the size of the
#                  largest tap (csrc/conv_wgrad_wino.hip), so a per-tap A is no valid bound there
# CALIBRATION.  CPU emulation only: nothing measured on a GPU backs these constants until a hardware run of
# tests/test_gpu_wgrad_sweep.py is recorded beside them.  ``python tests/test_wgrad_sweep_cpu.py`` prints the table;
# inputs ``inputs()`` below, honest fp32 = torch's fp32 conv2d backward (direct) / ``wgrad_wino`` in float32
# (Winograd), 15 layers (tests/test_wgrad_sweep_cpu.py: CAL_SHAPES), K 64 .. 12 288, Cin 3 .. 192.
#   worst honest ratio |err| / (U A):  direct 12.2 (K 512; 9.4 at K 429, 6.6 at K 100, 2.9 at K 64, 2.7 at K 3072,
#       0.9 at K 12 288), Winograd 1.67 (K 64; 1.1 at K 72 / 80, 0.8 at K 720 / 2048, 0.3 at K 12 288).
#   shape of g: the honest ratio does not grow with K (it falls: the products dy x have zero mean, so the rounding
#       errors of a long sum average out faster than A = sum |dy| |x| grows) -- g = 1; sqrt(K) or log K would only
#       loosen the bound where K is large, which is where the slips are smallest.
#   constants: about 4x the worst honest ratio (the margin of conv_sweep.C_BOUND, for rounding-order differences
#       between the emulation and MFMA): direct 48, Winograd 7 (both geometries: same arithmetic).
#   smallest ratio any slip produced (``slips()``; all at K 12 288, where one rounding matters least): direct 316
#       (operands rounded to TF32), Winograd 50 (TF32 in the 16 lowest-scale output channels); every other slip
#       (partial tile row, slab or image dropped / doubled, taps transposed, 16-channel blocks swapped) measures
#       8.5e4 .. 5.7e7.  Every constant stays below.
#   the old max-norm tolerance of test_conv_wgrad, 2e-6 max|dw| max(1, sqrt(K)/8), on the same inputs: ACCEPTS the
#       TF32 slip in the 16 lowest-scale output channels on all 7 direct and 6 of the 8 Winograd layers (not at K 64 /
#       80 on 48 output channels); it rejects every other slip of the list, the block swap in the low-scale channels
#       included -- a swap is a 100 % error of elements that are 1e-2 .. 1e-3 of the largest, far above 2e-6.
C_BOUND = {0: 48.0, 1: 7.0, 2: 7.0}


def _round_up(v, m):
    return (v + m - 1) // m * m


def _request(key, src):
    return dict(key=tuple(int(v) for v in key), src=src)


# ---------------------------------------------------------------------------------------------------------------
# the plan query
# ---------------------------------------------------------------------------------------------------------------
def num_variants():
    return int(_lib.lib().egn_conv2d_wgrad_num_variants())


def plan(key):
    """dict of PLAN_FIELDS, or None where the planner refuses the request."""
    out = (C.c_int * len(PLAN_FIELDS))()
    if _lib.lib().egn_conv2d_wgrad_plan_query(*(list(key) + [out])) != 0:
        return None
    return dict(zip(PLAN_FIELDS, [int(v) for v in out]))


def ws_bytes(key):
    return int(_lib.lib().egn_conv2d_wgrad_ws_bytes(*key))


def shrink_branch(p):
    """Which branches of the tile-shrinking loop the plan took: subset of {'TNB', 'TH', 'TW'}."""
    return frozenset(k for k, f in (('TNB', 'shrink_tnb'), ('TH', 'shrink_th'), ('TW', 'shrink_tw')) if p[f] > 0)


def plan_tuple(p):
    """What the reference-time rule thins by (never by the table row alone)."""
    return (p['row'], p['TNB'], p['nsplit'], p['lanes'], shrink_branch(p))


# ---------------------------------------------------------------------------------------------------------------
# host-derived requests: forward hooks on a CPU forward of the torch modules
# ---------------------------------------------------------------------------------------------------------------
def _hooked_layers(net, x):
    """[(module name, module, input shape)] of every nn.Conv2d / nn.Linear call of ``net(x)``, in call order."""
    seen, handles = [], []
    names = {m: k for k, m in net.named_modules()}

    def hook(mod, inp, out):
        seen.append((names[mod], mod, tuple(inp[0].shape)))
    for m in net.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
            handles.append(m.register_forward_hook(hook))
    try:
        with torch.no_grad():
            net(x)
    finally:
        for h in handles:
            h.remove()
    return seen


def hrnet_requests(name, cfg, batches=BATCHES):
    """One request per trainable Conv2d / Linear of the HRNet ``cfg`` builds, per batch size, with the channel
    strides of train_hrnet._Tape: every activation lives in an NHWC buffer whose channel stride is its channel
    count rounded up to 4 (engine.Buf); the one exception is the coordinate head's 'head1', whose output buffer
    also holds the two coordinate ramps (J + 2 channels).  One CPU forward at batch 1 gives the shapes."""
    from egonet_amd.model.heatmapModel import hrnet
    net = hrnet.get_pose_net(cfg, is_train=False).eval()
    iw, ih = cfg['heatmapModel']['input_size']
    layers = _hooked_layers(net, torch.zeros(1, 3, ih, iw))
    J = net.num_joints
    reqs = []
    for n in batches:
        for lname, mod, shp in layers:
            if not mod.weight.requires_grad:
                continue
            if isinstance(mod, torch.nn.Linear):
                cout, cin = mod.weight.shape
                h = w = kh = kw = stride = 1
                pad = 0
            else:
                cout, cin, kh, kw = mod.weight.shape
                h, w = shp[2], shp[3]
                stride, pad = mod.stride[0], mod.padding[0]
            cs_out = _round_up(J + 2, 4) if lname == 'head1.0' else _round_up(cout, 4)
            reqs.append(_request((n, h, w, cin, _round_up(cin, 4), cout, cs_out, kh, kw, stride, pad),
                                 '%s/b%d:%s' % (name, n, lname)))
    return reqs


def lifter_model():
    from egonet_amd.model import FCmodel
    return FCmodel.get_fc_model(1, configs.w48_config(), 66, 96)


def lifter_requests(rows=LIFTER_ROWS):
    """The lifter's Linear layers as 1x1 convolutions on 1x1 maps, with the leading dimensions of
    train_lifter.LifterTrainStep: the input rows are padded to a multiple of 4 floats, every other matrix is dense."""
    net = lifter_model().eval()
    layers = _hooked_layers(net, torch.zeros(2, 66))
    reqs = []
    for n in rows:
        for k, (lname, mod, shp) in enumerate(layers):
            cout, cin = mod.weight.shape
            reqs.append(_request((n, 1, 1, cin, _round_up(cin, 4) if k == 0 else cin, cout, cout, 1, 1, 1, 0),
                                 'lifter/b%d:%s' % (n, lname)))
    return reqs


def model_config(name):
    for mname, mk, _ in conv_sweep.INFERENCE_MODELS:
        if mname == name:
            return mk()
    raise KeyError(name)


_CORPUS = None


def corpus():
    """[(group name, [requests])]: the models conv_sweep.INFERENCE_MODELS names at 1, 2 and 3 crops and the lifter
    at 1, 7 and 100 rows; duplicates (same key) dropped, the first sighting kept."""
    global _CORPUS
    if _CORPUS is None:
        seen, groups = set(), []
        for name, mk, _ in conv_sweep.INFERENCE_MODELS:
            groups.append((name, hrnet_requests(name, mk())))
        groups.append(('lifter', lifter_requests()))
        out = []
        for name, reqs in groups:
            kept = []
            for r in reqs:
                if r['key'] not in seen:
                    seen.add(r['key'])
                    kept.append(r)
            out.append((name, kept))
        _CORPUS = out
    return _CORPUS


def corpus_requests():
    return [r for _, reqs in corpus() for r in reqs]


# ---------------------------------------------------------------------------------------------------------------
# the supplement: what no product request selects.  Each entry names what it is there for; the CPU coverage test
# fails an entry whose purpose the product corpus already serves.
#   row=<table row>          that row of kWgradTable
#   shrink=<'TNB'|'TH'|'TW'> that branch of the tile-shrinking loop
#   reduce=(lanes, frag)     that reduce width in that slab order
# Shapes found with the plan query (``python tests/wgrad_sweep.py`` lists the plans per row).  The product corpus
# reaches both Winograd rows, every 1x1 row, all three shrink branches (TNB: the 4x4 / 4x3 valid convolutions of the
# coordinate heads, TH: every strided 3x3, TW: head2.0.downsample) and every reduce width in both slab orders
# (fragment order at 32 lanes: 48 -> 48 on 64 x 64 maps at 3 crops, 96 tiles), so none of those has an entry.
# ---------------------------------------------------------------------------------------------------------------
SUPPLEMENT = [
    # <9,1,1,1,3,3,5>: at most 9 taps but not 3x3 (no K slicing), 48 channels pad less to 48 than to 64 (J = 3),
    # stride 1 (128-pixel tiles, a_it 3).  The product has no such filter: its non-3x3 filters are 1x1, 4x4, 4x3.
    ((3, 9, 13, 48, 48, 48, 48, 1, 3, 1, 0), ('row', 4), '1x3 stride 1 on 48 -> 48'),
    # <9,1,1,1,3,2,5>: the same with stride 2 (64-pixel tiles): five of the nine tap waves idle
    ((3, 10, 14, 48, 48, 48, 48, 2, 2, 2, 0), ('row', 5), '2x2 stride 2 on 48 -> 48'),
    # <8,2,1,1,4,2,5>: 10 .. 16 taps with channel counts that pad less to 64 (J = 4); the product's 4x4 / 4x3
    # filters are 66 -> 66 (J = 3)
    ((3, 6, 5, 64, 64, 64, 64, 4, 4, 1, 0), ('row', 8), '4x4 valid on 64 -> 64'),
]


def supplement_requests():
    return [_request(key, 'supplement: ' + why) for key, _, why in SUPPLEMENT]


# ---------------------------------------------------------------------------------------------------------------
# inputs, the reference and the bound
# ---------------------------------------------------------------------------------------------------------------
def out_hw(key):
    n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad = key
    return (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1


def grad_like(n, ho, wo, c, cs, gen, device='cpu'):
    """NHWC [n, ho, wo, cs] fp32 shaped like the gradient of a layer's output: zero mean, per-channel scales spread
    log-uniformly over three decades (channel 0 the largest: 1, the last 1e-3), a few spatial positions zero in
    every channel (a loss that masks joints), pad channels zero."""
    scale = 10.0 ** (-3.0 * torch.arange(c, dtype=torch.float64) / max(c - 1, 1))
    dy = torch.randn(n, ho, wo, c, generator=gen) * scale.float()
    npos = n * ho * wo
    dead = torch.randperm(npos, generator=gen)[:min(3, npos // 4)]
    dy.view(npos, c)[dead] = 0.0
    out = torch.zeros(n, ho, wo, cs)
    out[..., :c] = dy
    return out.to(device)


def inputs(key, gen, device='cpu'):
    n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad = key
    ho, wo = out_hw(key)
    return act_like(n, h, w, cin, cs_in, gen, device), grad_like(n, ho, wo, cout, cs_out, gen, device)


def nchw64(t, c):
    """NHWC [n, h, w, cs] fp32 -> NCHW [n, c, h, w] float64 on the same device."""
    return t[..., :c].permute(0, 3, 1, 2).double()


def reference(key, x, dy):
    """(dw64, A) of a request from its NHWC fp32 inputs, on their device: train_checks.wgrad_ref64 on the values and
    on the absolute values; for the Winograd forms A is summed over the nine taps of each (co, ci)."""
    from train_checks import wgrad_ref64
    n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad = key
    x64, dy64 = nchw64(x, cin), nchw64(dy, cout)
    want = wgrad_ref64(x64, dy64, kh, kw, stride, pad)
    A = wgrad_ref64(x64.abs(), dy64.abs(), kh, kw, stride, pad)
    return want, A


def bound_A(A, form):
    return A.sum(dim=(2, 3), keepdim=True).expand_as(A) if form else A


def worst(got, want, A, form):
    """(worst ratio |got - want| / (U A[form]), its (co, ci, tap)) over EVERY element."""
    r = ratio(got, want, bound_A(A, form))
    i = int(r.reshape(-1).argmax())
    taps = r.shape[2] * r.shape[3]
    return float(r.reshape(-1)[i]), (i // (r.shape[1] * taps), (i // taps) % r.shape[1], i % taps)


def old_tolerance(want, K):
    """The max-norm tolerance tests/test_gpu_train_ops.py::test_conv_wgrad uses."""
    return 2e-6 * float(want.abs().max()) * max(1.0, K ** 0.5 / 8)


# ---------------------------------------------------------------------------------------------------------------
# the algebra of csrc/conv_wgrad_wino.hip in numpy, in the dtype of its inputs (float64: the pinned restatement of
# tests/test_wgrad_wino_math_cpu.py; float32: the honest-fp32 model of the Winograd form for the bound's calibration)
# ---------------------------------------------------------------------------------------------------------------
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)


def wgrad_wino(x, dy):
    """x [N,Ci,H,W], dy [N,Co,H,W] (H, W even) -> dg [Co,Ci,3,3], the kernel's organisation: eight "waves"
    (frequency row i, column pair jb), each reading only the patch rows / columns its frequencies touch with ONE
    sign per direction (both transforms negate frequency 3), folding its two columns into the two values (q0, q1)
    the three tap columns need, and the fixed-order sum over the waves with the coefficients G[i][tap row] and the
    (q, sign) table of the source wave's jb.  Computes in x.dtype."""
    dt = x.dtype
    n, ci, h, w = x.shape
    co = dy.shape[1]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    one, half = dt.type(1.0), dt.type(0.5)
    parked = {}                                            # (i, jb) -> (q0, q1), each [Co, Ci]
    for i in range(4):
        ra, rb = [(0, 2), (1, 2), (2, 1), (3, 1)][i]       # patch rows (a, b); T = a + sr b
        sr = one if i == 1 else -one
        ea, eb = (1, 0) if i == 3 else (0, 1)              # dy rows (a, b); R = a + tr b
        tr = dt.type({0: 0.0, 1: 1.0, 2: -1.0, 3: 0.0}[i])
        for jb in range(2):
            ca, cb, cc = (0, 2, 1) if jb == 0 else (3, 1, 2)
            sc = one if jb == 0 else -one
            da, db = (0, 1) if jb == 0 else (1, 0)
            acc = np.zeros((2, co, ci), dtype=dt)
            for ty in range(h // 2):
                for tx in range(w // 2):
                    d = xp[:, :, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]          # [N,Ci,4,4]
                    e = dy[:, :, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2]          # [N,Co,2,2]
                    T = d[:, :, ra, :] + sr * d[:, :, rb, :]                    # [N,Ci,4]
                    V = np.stack([T[..., ca] - T[..., cb], T[..., cc] + sc * T[..., cb]])      # [2,N,Ci]
                    R = e[:, :, ea, :] + tr * e[:, :, eb, :]                    # [N,Co,2]
                    M = np.stack([R[..., da], R[..., db] + sc * R[..., da]])    # [2,N,Co]
                    acc += np.einsum('fnc,fnd->fcd', M, V)
            h_ = half * acc[1]
            parked[(i, jb)] = (acc[0] + h_, h_)
    dg = np.zeros((co, ci, 3, 3), dtype=dt)
    for ta in range(3):
        for tb in range(3):
            s = np.zeros((co, ci), dtype=dt)
            for i in range(4):
                g = dt.type(G[i, ta])
                if g == 0:
                    continue
                v0 = parked[(i, 0)][0 if tb == 0 else 1]                        # jb = 0: (q0, q1, q1)
                v1 = parked[(i, 1)][0 if tb == 2 else 1]                        # jb = 1: (q1, -q1, q0)
                s += g * (v0 - v1 if tb == 1 else v0 + v1)
            dg[:, :, ta, tb] = s
    return dg


# ---------------------------------------------------------------------------------------------------------------
# honest fp32 and the slips (CPU), for the bound's validation
# ---------------------------------------------------------------------------------------------------------------
def honest_fp32(key, x, dy, form):
    """dw [Cout,Cin,KH,KW] the way an honest fp32 implementation of the form computes it: torch's fp32 conv2d
    backward (direct), ``wgrad_wino`` in float32 (Winograd)."""
    n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad = key
    xs = x[..., :cin].permute(0, 3, 1, 2).contiguous()
    ds = dy[..., :cout].permute(0, 3, 1, 2).contiguous()
    if form:
        return torch.from_numpy(wgrad_wino(xs.numpy(), ds.numpy()))
    wt = torch.zeros(cout, cin, kh, kw, requires_grad=True)
    with torch.enable_grad():
        torch.nn.functional.conv2d(xs, wt, None, stride, pad).backward(ds)
    return wt.grad.detach()


def tf32(t):
    """Round an fp32 tensor to TF32's 10-bit mantissa (nearest even)."""
    b = t.contiguous().view(torch.int32)
    b = (b + 0xfff + ((b >> 13) & 1)) & ~0x1fff
    return b.view(torch.float32)


def slips(key, x, dy, want, nsplit=8):
    """{name: wrong dw (float64)}: what a subtly wrong kernel would return for the request, each computed exactly
    (float64) so that only the slip separates it from ``want``."""
    from train_checks import wgrad_ref64
    n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad = key
    ho, wo = out_hw(key)
    x64, dy64 = nchw64(x, cin), nchw64(dy, cout)

    def ref(a, b):
        return wgrad_ref64(a, b, kh, kw, stride, pad)
    out = {'tf32 operands': ref(nchw64(tf32(x), cin), nchw64(tf32(dy), cout))}
    if cout >= 32:
        wrong = want.clone()
        wrong[cout - 16:] = out['tf32 operands'][cout - 16:]
        out['tf32 operands in the low-scale co block'] = wrong
    if ho % 8:
        d = dy64.clone()
        d[:, :, ho // 8 * 8:] = 0                            # the rows of the last, partial 8-row tile
        out['last partial tile row dropped'] = ref(x64, d)
    d = dy64.permute(1, 0, 2, 3).reshape(cout, -1).clone()   # pixels in (n, oy, ox) order: one of nsplit ranges
    K = d.shape[1]
    s = nsplit // 2
    d[:, K * s // nsplit:K * (s + 1) // nsplit] = 0
    out['one of %d slabs dropped' % nsplit] = ref(x64, d.view(cout, n, ho, wo).permute(1, 0, 2, 3))
    if kh == kw and kh > 1:
        out['taps transposed'] = want.transpose(2, 3).contiguous()
    if cout >= 48 and cin >= 48:
        # the fragment-order reduce scatters 16 x 16 (co, ci) blocks of a 48 x 48 tile: two ci blocks swapped in
        # the co block of the LAST tile row, which holds the lowest-scale channels
        wrong = want.clone()
        c0 = cout - 16
        wrong[c0:, 0:16], wrong[c0:, 16:32] = want[c0:, 16:32], want[c0:, 0:16]
        out['two ci blocks swapped in the low-scale co block'] = wrong
    if n % 2:
        out['last image of the odd batch counted twice'] = want + ref(x64[-1:], dy64[-1:])
    return out


if __name__ == '__main__':
    rows = {}
    for r in corpus_requests() + supplement_requests():
        p = plan(r['key'])
        rows.setdefault(p['row'] if p else None, []).append((r, p))
    for row in sorted(rows, key=lambda v: -1 if v is None else v):
        print('row', row, len(rows[row]), 'requests')
        for r, p in rows[row][:4]:
            print('   ', r['key'], r['src'], p and {k: p[k] for k in PLAN_FIELDS[1:]})
