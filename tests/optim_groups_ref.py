"""The grouped optimizer step (csrc/optim.hip, egonet_amd/optim.py) against torch's own optimizers in float64.

Helper module of tests/test_optim_groups_cpu.py and tests/test_gpu_optim_groups.py (imported, not a conftest).

A case is a dict: ``variant`` (a row of VARIANTS: the family and three groups' hyper-parameters, rounded to fp32 as the
kernel's table holds them), ``layout`` (a row of LAYOUTS: the parameters in buffer order as (numel, group)),
``step0`` (the step counter before the launch: 0, 1 or 999, the counts tests/train_ops_sweep.py uses), and for
clipping ``max_norm`` and ``grad`` ('below', 'above', 'zero', 'inf').  ``inputs`` draws the fp32 state the way
train_ops_sweep does (gradients over nine decades with exact zeros); every comparison is ONE step from that state.

``reference``: torch.optim.Adam / AdamW / SGD on CPU float64 copies of the parameters, the state injected
(``state[p] = {'step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'}`` or ``{'momentum_buffer'}``), clipping by
``torch.nn.utils.clip_grad_norm_``.  ``emulate``: the header's formula in torch, per element with per-element
hyper-parameters, in fp32 (what the kernel computes: bias corrections and the AdamW factor in double rounded once,
the norm summed in double) or in float64 (it agrees with the torch reference to 1e-12 of A: the formula IS torch's),
and the first-order magnitude A of every output, as ``train_ops_sweep._optimizer`` does it -- the quotient's A is
the propagation of A_m and A_v through m' / (sqrt(v') / bc2 + eps).

The bound, per output and element:  |got - want64| <= C[variant] * 2^-24 * A;  where A is 0 or want64 is not finite,
got equals want64 (NaN matches NaN).  Parameters, moments, vmax and buf are each held to it; ``total_norm`` to
C['norm'] * 2^-24 * total_norm.  Each constant is about four times the worst ratio of the fp32 emulation against
the float64 reference over ``edge_cases()``, measured on the CPU (tests/test_optim_groups_cpu.py prints the
ratios), plus 6 where the variant has sqrtf and the two divisions -- the rule of train_ops_sweep's table (adam 3.13 ->
18, adam_l2 5.33 -> 28, sgd 3.28 -> 13).  Never against the kernel.

  variant            worst emulation ratio   C
  adam               3.84                    16 + 6 (sqrtf, two divisions)
  adamw              2.45                    10 + 6
  adam_amsgrad       4.33                    18 + 6
  adamw_amsgrad      2.54                    10 + 6
  sgd                3.04                    12     (momentum and dampening)
  sgd_nesterov       2.95                    12
  sgd_plain          2.40                    10     (momentum 0, no buffer)
  with clipping      worst added 0.82        + 4    (the coefficient rounded to fp32 once, g * coef rounded once;
                                                     adamw 3.27 against 2.45; adam 4.41 on the 1 M element case)
  norm               0.62                    2      (a double sum rounded to fp32 once: 0.5 at the most)

A wrong kernel of the kinds in MUTANTS breaks these bounds on the same inputs (checked on the CPU).
"""
import numpy as np
import torch

from egonet_amd import optim

U = 2.0 ** -24
ITEM = 1024                       # egn_optim_item_floats(); the GPU test checks the library says the same


def _f32(v):
    return float(np.float32(v))


def _hp(**kw):
    return {k: (tuple(_f32(b) for b in v) if k == 'betas' else (_f32(v) if isinstance(v, float) else v))
            for k, v in kw.items()}


_ADAM = [_hp(lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8),
         _hp(lr=3e-4, weight_decay=0.0, betas=(0.8, 0.99), eps=1e-6),
         _hp(lr=0.0, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8)]
_AMS = [dict(g, amsgrad=(k == 1)) for k, g in enumerate(_ADAM)]          # AMSGrad in one group only
_SGD = [_hp(lr=1e-2, weight_decay=1e-3, momentum=0.9, dampening=0.0),
        _hp(lr=3e-3, weight_decay=0.0, momentum=0.8, dampening=0.1),
        _hp(lr=0.0, weight_decay=1e-3, momentum=0.9, dampening=0.0)]
_NEST = [dict(_SGD[0], nesterov=True), dict(_SGD[1]), dict(_hp(lr=2e-3, weight_decay=1e-3, momentum=0.5, dampening=0.0),
                                                           nesterov=True)]
_PLAIN = [dict(g, momentum=0.0, dampening=0.0) for g in _SGD]
VARIANTS = {
    'adam': ('adam', _ADAM), 'adamw': ('adamw', _ADAM), 'adam_amsgrad': ('adam', _AMS),
    'adamw_amsgrad': ('adamw', _AMS), 'sgd': ('sgd', _SGD), 'sgd_nesterov': ('sgd', _NEST),
    'sgd_plain': ('sgd', _PLAIN),
}
C_BOUND = {
    'adam': 22.0, 'adamw': 16.0, 'adam_amsgrad': 24.0, 'adamw_amsgrad': 16.0, 'sgd': 12.0, 'sgd_nesterov': 12.0,
    'sgd_plain': 10.0, 'norm': 2.0,
}
C_CLIP = 4.0

# the parameters in buffer order: (numel, group).  Flat sizes: 4; 1020; 1028; one segment of more than two work items
# with a partial last one; 4-float segments alternating between three groups; 1, 15 and 17 elements (the padding rule)
LAYOUTS = {
    'n4': [(4, 0)],
    'n1020': [(1020, 0)],
    'n1028': [(1028, 0)],
    'long': [(2 * ITEM + 520, 0), (12, 1)],
    'alt3': [(4, i % 3) for i in range(30)],
    'pad': [(1, 0), (15, 1), (17, 0), (6, 1), (3, 2)],
    # more than one trip of the norm kernels' grid (1024 blocks x 256 threads x 4 floats), ragged
    'big': [(1024 * 256 * 4 + 3000, 0), (1028, 1)],
}
MUTANTS = ('adamw_coupled_decay', 'amsgrad_max_after_bias_correction', 'nesterov_buf_alone',
           'dampening_on_first_step', 'clip_coef_not_clamped', 'clip_no_eps', 'segment_shifted_one_float4',
           'group1_reads_group0_lr')


def case(variant, layout, step0, max_norm=None, grad='normal'):
    return dict(variant=variant, layout=layout, step0=step0, max_norm=max_norm, grad=grad)


def problem(variant, family, rows, params, step0, max_norm=None):
    """A case outside the edge list: ``rows`` = the groups' hyper-parameters (rounded to fp32 here, as the table
    holds them), ``params`` = (numel, group) in buffer order; ``variant`` names the constant it is held to."""
    return dict(variant=variant, layout='model', family=family, rows=[_hp(**r) for r in rows], params=list(params),
                step0=step0, max_norm=max_norm, grad='normal')


def case_id(c):
    s = '%s-%s-t%d' % (c['variant'], c['layout'], c['step0'])
    return s if c['max_norm'] is None else s + '-clip%g-%s' % (c['max_norm'], c['grad'])


def edge_cases():
    E = []
    for v in VARIANTS:
        for lay in ('n4', 'n1020', 'n1028', 'long', 'alt3', 'pad'):
            for step0 in (0, 1, 999):
                E.append(case(v, lay, step0))
    # clipping: norm below max_norm (coefficient 1), above, all zero (with max_norm 1 and 0), one inf
    for v in ('adamw', 'adam_amsgrad', 'sgd_nesterov'):
        for lay in ('long', 'alt3'):
            E.append(case(v, lay, 1, 1e9, 'below'))
            E.append(case(v, lay, 1, 0.5, 'above'))
            E.append(case(v, lay, 1, 1.0, 'zero'))
            E.append(case(v, lay, 1, 0.0, 'zero'))
            E.append(case(v, lay, 1, 1.0, 'inf'))
    E.append(case('sgd_plain', 'n4', 0, 0.5, 'above'))                 # the norm kernels on 4 floats
    E.append(case('adam', 'big', 1, 0.5, 'above'))                     # ... and on more than one trip of their grid
    return E


def c_of(c):
    return C_BOUND[c['variant']] + (C_CLIP if c['max_norm'] is not None else 0.0)


# ---------------------------------------------------------------------------------------------------------------
# layout, spec and inputs
# ---------------------------------------------------------------------------------------------------------------
def layout_of(c):
    """-> (offsets, numels, groups, flat size): every parameter padded to a multiple of 4 floats (FlatParams)."""
    if 'params' in c:                                # an explicit problem (``problem``): a model's flat buffer
        lay = c['params']
    else:
        lay = LAYOUTS[c['layout']]
    offs, total = [], 0
    for n, _ in lay:
        offs.append(total)
        total += (n + 3) // 4 * 4
    return offs, [n for n, _ in lay], [k for _, k in lay], total


def group_rows(c):
    """The groups the layout uses, in table order."""
    if 'params' in c:
        return c['family'], [dict(r) for r in c['rows']]
    fam, rows = VARIANTS[c['variant']]
    ng = max(k for _, k in LAYOUTS[c['layout']]) + 1
    return fam, [dict(r) for r in rows[:ng]]


def spec_of(c, params):
    """The product's spec for the case: ``params`` = one tensor per parameter of the layout."""
    fam, rows = group_rows(c)
    _, _, grp, _ = layout_of(c)
    return optim.spec(fam, [dict(params=[p for p, k in zip(params, grp) if k == gi], **r) for gi, r in enumerate(rows)])


def tables(c):
    """-> (group table, item table, segments) through the product's builders."""
    offs, nums, grp, total = layout_of(c)
    params = [torch.zeros(n, requires_grad=True) for n in nums]
    sp = spec_of(c, params)
    segs = optim.segments(params, offs, total, sp)
    return optim.group_table(sp), optim.work_items(segs, ITEM), segs


def element_groups(c, items=None):
    """int64 [flat size]: the group of every float of the buffer, read from the item table."""
    if items is None:
        items = tables(c)[1]
    _, _, _, total = layout_of(c)
    eg = torch.full((total,), -1, dtype=torch.int64)
    for b, n, k in zip(items['begin'], items['length'], items['group']):
        eg[int(b):int(b) + int(n)] = int(k)
    return eg


def uses(c):
    """The state buffers the case has beside p and g."""
    fam, rows = group_rows(c)
    if fam == 'sgd':
        return ('buf',) if any(r['momentum'] != 0 for r in rows) else ()
    return ('m', 'v', 'vmax') if any(r.get('amsgrad') for r in rows) else ('m', 'v')


def inputs(c, seed=0):
    """fp32 CPU tensors p, g (+ m, v, vmax | buf) of the flat size, padding words 0, and the scalars."""
    offs, nums, grp, total = layout_of(c)
    g = torch.Generator().manual_seed(1000 * seed + 7 * c['step0'] + len(c['layout']) + 13 * len(c['variant']))
    mask = torch.zeros(total, dtype=torch.bool)
    for o, n in zip(offs, nums):
        mask[o:o + n] = True
    x = {'mask': mask, 'step0': c['step0']}
    x['p'] = 0.1 * torch.randn(total, generator=g)
    mag = 10.0 ** (9.0 * torch.rand(total, generator=g) - 6.0)           # 1e-6 .. 1e3
    grad = mag * torch.where(torch.rand(total, generator=g) < 0.5, -1.0, 1.0)
    grad[torch.rand(total, generator=g) < 0.05] = 0.0                    # exact zeros among them
    if c['grad'] == 'zero':
        grad = torch.zeros(total)
    elif c['grad'] == 'inf':
        grad = 1e-3 * torch.randn(total, generator=g)
        grad[offs[-1]] = float('inf')
    x['g'] = grad
    fresh = c['step0'] == 0
    for a in uses(c):
        st = torch.randn(total, generator=g) * 0.01
        if a == 'vmax':                                                  # above and below the new v' among them
            st = x['v'] * (0.5 + torch.rand(total, generator=g))
        x[a] = torch.zeros(total) if fresh else (st * st if a == 'v' else st)
    for a in ('p', 'g') + uses(c):
        x[a] = torch.where(mask, x[a], torch.zeros(())).float().contiguous()
    return x


# ---------------------------------------------------------------------------------------------------------------
# the header's formula per element: fp32 emulation, float64 twin, A; the mutants
# ---------------------------------------------------------------------------------------------------------------
def _per_element(rows, eg, key, dt, sub=None):
    vals = [r[key] if sub is None else r[key][sub] for r in rows]
    return torch.tensor(vals, dtype=torch.float64)[eg].to(dt)


def clip_scalars(c, x, dt, mut=None):
    """(total_norm, coef) as the norm launches write them: the sum of squares in double either way."""
    if c['max_norm'] is None:
        return None, 1.0
    norm = float(x['g'].double().pow(2).sum().sqrt())
    eps = 0.0 if mut == 'clip_no_eps' else 1e-6
    with np.errstate(all='ignore'):
        coef = np.float64(c['max_norm']) / (np.float64(norm) + eps)
    if mut != 'clip_coef_not_clamped':
        coef = np.float64(1.0) if coef > 1.0 else coef
    if dt == torch.float32:
        return _f32(norm), float(np.float32(coef))
    return norm, float(coef)


def emulate(c, x, dt=torch.float32, mut=None):
    """name -> (value in ``dt``, A in float64) for p and the state buffers; 'total_norm' with clipping."""
    fam, rows = group_rows(c)
    _, items, _ = tables(c)
    eg = element_groups(c, items)
    if mut == 'segment_shifted_one_float4':          # every boundary between two groups one float4 late
        eg = torch.cat([eg[:4], eg[:-4]])
    t = c['step0'] + 1
    P = lambda key, sub=None: _per_element(rows, eg, key, dt, sub)
    lr_rows = [r['lr'] for r in rows]
    if mut == 'group1_reads_group0_lr' and len(rows) > 1:
        lr_rows[1] = lr_rows[0]
    norm, coef = clip_scalars(c, x, dt, mut)
    p, g = x['p'].to(dt), x['g'].to(dt)
    out = {}
    if norm is not None:
        out['total_norm'] = (torch.tensor([norm], dtype=dt), torch.tensor([abs(norm)], dtype=torch.float64))
    gc = g * torch.tensor(coef, dtype=dt) if norm is not None else g
    A_gc = gc.abs().double()
    wd = P('weight_decay')
    if fam == 'sgd':
        lr = torch.tensor(lr_rows, dtype=torch.float64)[eg].to(dt)
        mu, damp = P('momentum'), P('dampening')
        nest = torch.tensor([bool(r.get('nesterov')) for r in rows])[eg]
        gi, A_g = gc + wd * p, A_gc + (wd * p).abs().double()
        upd, A_u = gi, A_g
        if 'buf' in x:
            buf = x['buf'].to(dt)
            keep = torch.ones((), dtype=dt) - damp
            if t <= 1 and mut != 'dampening_on_first_step':
                bi, A_b = gi, A_g
            else:
                old = torch.zeros_like(buf) if t <= 1 else buf
                bi, A_b = mu * old + keep * gi, (mu * old).abs().double() + keep.double() * A_g
            has = mu != 0
            bi, A_b = torch.where(has, bi, buf), torch.where(has, A_b, torch.zeros_like(A_b))
            out['buf'] = (bi, A_b)
            step_n = bi if mut == 'nesterov_buf_alone' else gi + mu * bi
            upd = torch.where(has, torch.where(nest, step_n, bi), gi)
            A_u = torch.where(has, torch.where(nest, A_g + mu.double() * A_b, A_b), A_g)
        out['p'] = (p - lr * upd, p.abs().double() + lr.double() * A_u)
        return out
    b1, b2, eps = P('betas', 0), P('betas', 1), P('eps')
    m, v = x['m'].to(dt), x['v'].to(dt)
    ams = torch.tensor([bool(r.get('amsgrad')) for r in rows])[eg]
    # per group, in double, rounded once where the kernel rounds: lr / (1 - b1^t), sqrt(1 - b2^t), 1 - lr wd
    ss = [lr_rows[k] / (1.0 - r['betas'][0] ** t) for k, r in enumerate(rows)]
    bc = [(1.0 - r['betas'][1] ** t) ** 0.5 for r in rows]
    dec = [1.0 - lr_rows[k] * r['weight_decay'] for k, r in enumerate(rows)]
    step_size, bc2, decay = (torch.tensor(q, dtype=torch.float64)[eg].to(dt) for q in (ss, bc, dec))
    decoupled = fam == 'adamw' and mut != 'adamw_coupled_decay'
    pc = p * decay if decoupled else p
    if decoupled:
        gi, A_g = gc, A_gc
    else:
        gi, A_g = gc + wd * pc, A_gc + (wd * pc).abs().double()
    one = torch.ones((), dtype=dt)
    mi = b1 * m + (one - b1) * gi
    vi = b2 * v + (one - b2) * gi * gi
    A_m = (b1 * m).abs().double() + (one - b1).double() * A_g
    A_v = (b2 * v).abs().double() + (one - b2).double() * A_g * A_g
    out['m'], out['v'] = (mi, A_m), (vi, A_v)
    vd, A_vd = vi, A_v
    if 'vmax' in x:
        vx = x['vmax'].to(dt)
        if mut == 'amsgrad_max_after_bias_correction':
            new = torch.maximum(vx, vi / (bc2 * bc2))
            den_ams = new.sqrt() + eps
        else:
            new = torch.maximum(vx, vi)
            den_ams = new.sqrt() / bc2 + eps
        new, A_x = torch.where(ams, new, vx), torch.where(ams, torch.maximum(vx.abs().double(), A_v),
                                                          torch.zeros_like(A_v))
        out['vmax'] = (new, A_x)
        vd, A_vd = torch.where(ams, new, vi), torch.where(ams, A_x, A_v)
    den = vd.sqrt() / bc2 + eps
    if 'vmax' in x and mut == 'amsgrad_max_after_bias_correction':
        den = torch.where(ams, den_ams, den)
    upd = step_size * (mi / den)
    den64, rt = den.double(), vd.double().sqrt()
    A_q = A_m / den64 + torch.where(rt > 0, mi.double().abs() * A_vd /
                                    (2 * rt.clamp_min(1e-300) * bc2.double() * den64 ** 2), torch.zeros_like(rt))
    out['p'] = (pc - upd, p.abs().double() + step_size.double().abs() * A_q)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the reference: torch's own optimizers in float64
# ---------------------------------------------------------------------------------------------------------------
def reference(c, x):
    """name -> float64 flat tensor (p and the state buffers; 'total_norm' with clipping), from torch.optim on CPU
    float64 parameters; padding words come from the float64 formula (they are no parameter of torch's)."""
    fam, rows = group_rows(c)
    offs, nums, grp, total = layout_of(c)
    ps = [torch.nn.Parameter(x['p'][o:o + n].double().clone()) for o, n in zip(offs, nums)]
    groups = []
    for gi, r in enumerate(rows):
        groups.append(dict(params=[p for p, k in zip(ps, grp) if k == gi], **r))
    cls = {'adam': torch.optim.Adam, 'adamw': torch.optim.AdamW, 'sgd': torch.optim.SGD}[fam]
    opt = cls(groups)
    for p, o, n, k in zip(ps, offs, nums, grp):
        p.grad = x['g'][o:o + n].double().clone()
        sl = slice(o, o + n)
        if fam == 'sgd':
            if c['step0'] > 0 and rows[k]['momentum'] != 0:
                opt.state[p] = {'momentum_buffer': x['buf'][sl].double().clone()}
        else:
            st = {'step': torch.tensor(float(c['step0'])), 'exp_avg': x['m'][sl].double().clone(),
                  'exp_avg_sq': x['v'][sl].double().clone()}
            if rows[k].get('amsgrad'):
                st['max_exp_avg_sq'] = x['vmax'][sl].double().clone()
            opt.state[p] = st
    want = {k: val.double().clone() for k, (val, _) in emulate(c, x, torch.float64).items()}
    if c['max_norm'] is not None:
        tn = torch.nn.utils.clip_grad_norm_(ps, c['max_norm'])
        want['total_norm'] = tn.detach().double().reshape(1)
    opt.step()
    names = {'m': 'exp_avg', 'v': 'exp_avg_sq', 'vmax': 'max_exp_avg_sq', 'buf': 'momentum_buffer'}
    for p, o, n in zip(ps, offs, nums):
        want['p'][o:o + n] = p.detach()
        for a in uses(c):
            st = opt.state[p].get(names[a])
            if st is not None:
                want[a][o:o + n] = st
    return want


def ratio(got, want, A):
    """(worst |got - want| / (2^-24 A) over the elements with finite want and A > 0, number of elements that had to
    be equal and are not: A == 0 or a non-finite want, where NaN matches NaN)."""
    got, want, A = got.double().reshape(-1), want.double().reshape(-1), A.double().reshape(-1)
    fin = torch.isfinite(want) & torch.isfinite(A) & (A > 0)
    err = (got - want).abs()
    worst = float((err[fin] / (U * A[fin])).nan_to_num(nan=float('inf')).max()) if bool(fin.any()) else 0.0
    rest = ~fin
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))
    return worst, int((rest & ~same).sum())


def check(c, got, want, A, C=None):
    """-> list of violations (empty: every output within its bound); prints nothing."""
    C = c_of(c) if C is None else C
    bad = []
    for name in want:
        Cn = C_BOUND['norm'] if name == 'total_norm' else C
        worst, unequal = ratio(got[name], want[name], A[name])
        if worst > Cn or unequal:
            bad.append('%s %s: ratio %.2f (C %.0f), %d unequal' % (case_id(c), name, worst, Cn, unequal))
    return bad
