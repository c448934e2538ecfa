"""The training-ops sweep's own parts, without a GPU: its float64 references against torch in float64 (autograd,
torch.optim), its fp32 emulations inside the bounds on the sweep's inputs, reference-side mutants outside them, the
ReLU-gate cap on the edge list, and the recorder on a stub."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import train_ops_sweep as T
from egonet_amd import _lib


def _bn_x(rows, cols, g, res, mask):
    z = torch.randn(rows, cols, generator=g, dtype=torch.float64) * 2 + 0.5
    m = z.mean(0)
    x = dict(z=z, mean=m, invstd=(z.var(0, unbiased=False) + 1e-5).rsqrt(),
             gamma=torch.rand(cols, generator=g, dtype=torch.float64) + 0.5,
             beta=torch.randn(cols, generator=g, dtype=torch.float64),
             dy=torch.randn(rows, cols, generator=g, dtype=torch.float64))
    if res:
        x['res'] = torch.randn(rows, cols, generator=g, dtype=torch.float64)
    if mask:
        x['mask'] = (torch.rand(rows, cols, generator=g) < 0.5).double()
    return x


@pytest.mark.parametrize('flag', [0, 1, 2, 0x11, 0x12])
@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('mask', [False, True])
def test_batchnorm_references_vs_autograd(flag, res, mask):
    g = torch.Generator().manual_seed(flag * 4 + res * 2 + mask)
    rows, cols = 29, 10
    x = _bn_x(rows, cols, g, res, mask)
    keep = 2.0 if mask else 1.0
    null = (() if res else ('res',)) + (() if mask else ('mask',))
    d = dict(rows=rows, cols=cols, ld=cols, keep_scale=keep)
    leaf = {k: x[k].clone().requires_grad_(True) for k in ('z', 'gamma', 'beta') + (('res',) if res else ())}
    o = F.batch_norm(leaf['z'], None, None, leaf['gamma'], leaf['beta'], True, 0.0, 1e-5)
    after = bool(flag & 0x10)
    if res and not after:
        o = o + leaf['res']
    o = F.leaky_relu(o, 0.01) if flag & 0xf == 2 else (torch.relu(o) if flag & 0xf else o)
    if mask:
        o = o * x['mask'] * keep
    if res and after:
        o = leaf['res'] + o
    y = T.reference(T._req('egn_bn_act_fwd_f32', 't', null=null, relu=flag, **d), x)['y'][0]
    assert float((y - o.detach()).abs().max()) < 1e-10
    if after:
        return          # the backward entry points take 0, 1, 2: the block tail's residual gradient is dy itself
    o.backward(x['dy'])
    sums = T.reference(T._req('egn_bn_bwd_sums_f32', 't', null=null, relu=flag, **d), x)
    assert float((sums['dbeta'][0] - leaf['beta'].grad).abs().max()) < 1e-9
    assert float((sums['dgamma'][0] - leaf['gamma'].grad).abs().max()) < 1e-9
    x2 = dict(x, dbeta=sums['dbeta'][0], dgamma=sums['dgamma'][0])
    dz = T.reference(T._req('egn_bn_bwd_dz_f32', 't', null=null, relu=flag, **d), x2)
    assert float((dz['dz'][0] - leaf['z'].grad).abs().max()) < 1e-9
    if res:
        assert float((dz['dres'][0] - leaf['res'].grad).abs().max()) < 1e-10


def test_statistics_reference_vs_torch():
    g = torch.Generator().manual_seed(3)
    rows, cols = 50, 7
    z = torch.randn(rows, cols, generator=g, dtype=torch.float64) + 2
    rm, rv = torch.randn(cols, generator=g, dtype=torch.float64), torch.rand(cols, generator=g, dtype=torch.float64)
    r = T._req('egn_bn_stats_f32', 't', rows=rows, cols=cols, ld=cols, eps=1e-5, momentum=0.1)
    out = T.reference(r, dict(z=z, running_mean=rm, running_var=rv))
    mom = r['s']['momentum']
    rm2, rv2 = rm.clone(), rv.clone()
    F.batch_norm(z, rm2, rv2, None, None, True, mom, r['s']['eps'])
    assert float((out['mean'][0] - z.mean(0)).abs().max()) < 1e-12
    assert float((out['invstd'][0] - (z.var(0, unbiased=False) + r['s']['eps']).rsqrt()).abs().max()) < 1e-10
    assert float((out['var_unbiased'][0] - z.var(0)).abs().max()) < 1e-10
    assert float((out['running_mean'][0] - rm2).abs().max()) < 1e-10
    assert float((out['running_var'][0] - rv2).abs().max()) < 1e-10


@pytest.mark.parametrize('crit', [0, 1, 2])
@pytest.mark.parametrize('acc', [0, 1])
def test_loss_references_vs_torch(crit, acc):
    g = torch.Generator().manual_seed(crit)
    rows, cols = 13, 9
    p = (torch.randn(rows, cols, generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    t = torch.randn(rows, cols, generator=g, dtype=torch.float64)
    d0 = torch.randn(rows, cols, generator=g, dtype=torch.float64)
    fn = (F.mse_loss, F.l1_loss, F.smooth_l1_loss)[crit]
    loss = 0.5 * fn(p, t)
    loss.backward()
    x = dict(pred=p.detach(), tgt=t, dpred=d0, loss=torch.tensor([0.75], dtype=torch.float64))
    reqs = [T._req('egn_elem_loss_f32', 't', rows=rows, cols=cols, ld_pred=cols, ld_tgt=cols, crit=crit, weight=0.5,
                   accumulate=acc)]
    if crit == 0:
        reqs.append(T._req('egn_mse_f32', 't', rows=rows, cols=cols, ld_pred=cols, ld_tgt=cols, weight=0.5,
                           accumulate=acc))
    if crit == 1 and not acc:
        reqs.append(T._req('egn_l1_f32', 't', n=rows * cols, weight=0.5))
    for r in reqs:
        out = T.reference(r, x)
        assert abs(float(out['loss'][0]) - 0.75 - float(loss.detach())) < 1e-12
        want = p.grad + (d0 if acc else 0)
        assert float((out['dpred'][0].reshape(rows, cols) - want).abs().max()) < 1e-12


@pytest.mark.parametrize('kind', ['adam', 'adam_l2', 'sgd', 'sgd0'])
def test_optimizer_references_vs_torch_optim_over_five_steps(kind):
    g = torch.Generator().manual_seed(5)
    n = 200
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    grads = [torch.randn(n, generator=g, dtype=torch.float64) for _ in range(5)]
    w = p0.clone().requires_grad_(True)
    if kind.startswith('adam'):
        r = T._req('egn_adam_l2_step_dev_f32', 't', n=n, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2) \
            if kind == 'adam_l2' else T._req('egn_adam_step_dev_f32', 't', n=n, beta1=0.9, beta2=0.999, eps=1e-8)
        s = r['s']
        opt = torch.optim.Adam([w], lr=1e-3, betas=(s['beta1'], s['beta2']), eps=s['eps'],
                               weight_decay=s.get('weight_decay', 0.0))
    else:
        mom = 0.9 if kind == 'sgd' else 0.0
        r = T._req('egn_sgd_step_dev_f32', 't', null=() if mom else ('buf',), n=n, momentum=mom, weight_decay=1e-3)
        opt = torch.optim.SGD([w], lr=1e-3, momentum=r['s']['momentum'], weight_decay=r['s']['weight_decay'])
    lr = torch.tensor([1e-3], dtype=torch.float64)
    x = dict(p=p0, m=torch.zeros(n, dtype=torch.float64), v=torch.zeros(n, dtype=torch.float64),
             buf=torch.zeros(n, dtype=torch.float64), lr_dev=lr, step_dev=torch.tensor([0], dtype=torch.int32))
    if kind == 'sgd0':
        del x['buf']
    for k in range(5):
        w.grad = grads[k].clone()
        opt.step()
        out = T.reference(r, dict(x, g=grads[k]))
        for a in ('p', 'm', 'v', 'buf'):
            if a in out:
                x[a] = out[a][0]
        x['step_dev'] = out['step_dev'][0].to(torch.int32)
        assert int(x['step_dev'][0]) == k + 1
        assert float((x['p'] - w.detach()).abs().max()) < 1e-12, k


def test_fuse_backward_reference_vs_autograd():
    """The interpolate-and-sum form of test_gpu_train_ops.test_fuse_backward_terms."""
    g = torch.Generator().manual_seed(8)
    n, hh, ww, c = 2, 16, 8, 12
    ts = [torch.randn(n, c, hh >> s, ww >> s, generator=g, dtype=torch.float64, requires_grad=True) for s in range(4)]
    y = torch.relu(sum(t if s == 0 else F.interpolate(t, scale_factor=1 << s, mode='nearest')
                       for s, t in enumerate(ts)))
    dy = torch.randn(n, c, hh, ww, generator=g, dtype=torch.float64)
    y.backward(dy)
    x = dict(dy=dy.permute(0, 2, 3, 1).contiguous(), y=y.detach().permute(0, 2, 3, 1).contiguous())
    for s in range(4):
        got = T.reference(T._req('egn_fuse_bwd_f32', 't', N=n, H=hh, W=ww, cs=c, shift=s), x)['g'][0]
        assert float((got.permute(0, 3, 1, 2) - ts[s].grad).abs().max()) < 1e-12


@pytest.fixture(scope='module')
def edge_cases():
    """(request, inputs, reference) of the edge list, computed once."""
    out = []
    for r in T.edge_requests():
        x = T.inputs(r)
        out.append((r, x, T.reference(r, x)))
    return out


def test_fp32_emulations_stay_inside_the_bounds(edge_cases):
    worst = {}
    for r, x, ref in edge_cases:
        for k, v in T.worst_ratios(T.emulate(r, x), ref).items():
            w = worst.setdefault(r['name'], [0.0, ''])
            if v >= w[0]:
                w[0], w[1] = v, '%s (%s)' % (k, r['src'])
    print()
    for name, (v, where) in sorted(worst.items()):
        print('%-30s emulation worst %6.2f  C %5.1f  %s' % (name, v, T.C_BOUND[name], where))
        assert v <= T.C_BOUND[name], (name, v, where)
        assert T.C_BOUND[name] == 0 or v > 0, name       # the emulation is not the reference in disguise
    assert set(worst) == {r['name'] for r, _, _ in edge_cases}


def test_conditioning_of_the_one_pass_variance(edge_cases):
    r, x, ref = next(c for c in edge_cases if c[0]['opt'].get('offsets'))
    cols = r['s']['cols']
    z = x['z'][:, :cols]
    var64 = ref['_rel_var'][0]
    emu = T.emulate(r, x)['_rel_var'][0]
    tv = z.var(0, unbiased=False)                      # torch's fp32 two-pass variance
    rm, rv = torch.zeros(cols), torch.zeros(cols)
    F.batch_norm(z, rm, rv, None, None, True, 1.0, 1e-5)      # momentum 1: running_var = the batch's (unbiased)
    tb = rv.double() * (z.shape[0] - 1) / z.shape[0]
    print()
    for k, off in enumerate((0, 3, 30)):
        sel = slice(k, cols, 3)
        e = float(((emu[sel] - var64[sel]).abs() / var64[sel]).max())
        t = float(((tb[sel] - var64[sel]).abs() / var64[sel]).max())
        print('offset %2d sigma: one-pass emulation %.2e, torch fp32 batch_norm %.2e' % (off, e, t))
        assert e <= T.C_BOUND['egn_bn_stats_f32'] * T.U * (1 + off * off) * 1.2
    assert float(((tv.double() - var64).abs() / var64).max()) < 1e-5


def _mutant_cases(edge_cases, mut):
    pick = {
        'dz_no_row_terms': lambda r: 'bwd_dz' in r['name'],
        'invstd_unbiased': lambda r: r['name'] in ('egn_bn_stats_f32', 'egn_bn_stats_finalize_f32') and r['s']['rows'] > 3,
        'bias_correction_t_minus_1': lambda r: 'adam' in r['name'] and r['opt']['step0'] > 0,
        'weight_decay_after_moments': lambda r: r['name'] == 'egn_adam_l2_step_dev_f32',
        'sgd_first_step_momentum': lambda r: r['name'] == 'egn_sgd_step_dev_f32' and r['opt']['step0'] == 0
        and r['s']['momentum'] > 0,
        'smooth_l1_threshold_half': lambda r: r['name'] == 'egn_elem_loss_f32' and r['s']['crit'] == 2,
        'l1_grad_at_zero': lambda r: r['name'] in ('egn_elem_loss_f32', 'egn_l1_f32') and r['s'].get('crit', 1) == 1
        and 'dpred' not in r['null'],
        'leaky_slope_0.1': lambda r: r['name'].startswith('egn_bn_') and r['s'].get('relu', 0) & 0xf == 2,
        'res_before_activation': lambda r: 'fwd' in r['name'] and r['s']['relu'] & 0x10 and 'res' not in r['null'],
        'no_keep_scale_in_backward': lambda r: 'bwd' in r['name'] and bool(
            r['s'].get('p') or ('keep_scale' in r['s'] and 'mask' not in r['null'])),
    }[mut]
    return [c for c in edge_cases if pick(c[0])]


@pytest.mark.parametrize('mut', T.MUTANTS)
def test_reference_side_mutants_break_the_bounds(edge_cases, mut):
    """A bound that a wrong kernel of these kinds would meet is not a test: each mutant of the reference is further
    from the reference than the bound allows, on every edge case it applies to."""
    cases = _mutant_cases(edge_cases, mut)
    assert cases, mut
    for r, x, ref in cases:
        got = T.reference(r, x, mut=mut)
        w = T.worst_ratios(got, ref)
        assert max(w.values()) > T.C_BOUND[r['name']], (mut, r['name'], r['src'], w)


def test_gate_cap_holds_on_the_edge_list(edge_cases):
    print()
    for r, x, ref in edge_cases:
        share = ref.get('_left_out')
        if share is not None:
            if share:
                print('%s %s: %.4f of the columns left out' % (r['name'], r['src'], share))
            assert share <= T.GATE_CAP, (r['name'], r['src'], share)


def test_dropout_masks_keep_the_binomial_share(edge_cases):
    for r, x, ref in edge_cases:
        p = r['s'].get('p')
        if p and '_kept' in ref:
            n = r['s']['rows'] * r['s']['cols'] if 'rows' in r['s'] else r['s']['n']
            assert abs(ref['_kept'] - (1 - p)) <= 4 * (p * (1 - p) / n) ** 0.5, (r['src'], ref['_kept'])


class _Stub(object):
    """Stands in for the library: the entry points return what they were given."""

    def __init__(self):
        self.calls = []

    def egn_add_f32(self, *a):
        self.calls.append(('egn_add_f32', a))
        return 0

    def egn_bn_act_fwd_f32(self, *a):
        self.calls.append(('egn_bn_act_fwd_f32', a))
        return 7

    def egn_version(self):
        return 42


def test_recorder_notes_a_stubs_calls():
    stub = _Stub()
    prev = _lib._LIB
    with T.Recorder(handle=stub) as rec:
        L = _lib.lib()
        rec.src = 'first'
        assert L.egn_add_f32(C.c_void_p(64), C.c_void_p(128), C.c_void_p(64), 4096, None) == 0
        rec.src = 'second'
        assert L.egn_add_f32(C.c_void_p(640), C.c_void_p(1280), C.c_void_p(640), 4096, C.c_void_p(5)) == 0
        assert L.egn_add_f32(C.c_void_p(64), C.c_void_p(128), C.c_void_p(256), 4096, None) == 0
        assert L.egn_bn_act_fwd_f32(C.c_void_p(8), C.c_void_p(16), C.c_void_p(24), C.c_void_p(32), C.c_void_p(40), None,
                                    1.0, 0x11, None, C.c_void_p(8), 30, 66, 68, None) == 7
        assert L.egn_version() == 42                 # not of train_ops.hip: forwarded, not noted
    assert _lib._LIB is prev
    assert [c[0] for c in stub.calls] == ['egn_add_f32'] * 3 + ['egn_bn_act_fwd_f32']
    assert stub.calls[0][1][3] == 4096               # forwarded unchanged
    m = T.merged(rec.notes)
    assert len(rec.notes) == 4 and len(m) == 3
    assert m[0]['name'] == 'egn_add_f32' and m[0]['s'] == {'n': 4096} and m[0]['alias'] == (('a', 'y'),)
    assert m[0]['srcs'] == ['first', 'second'] and m[0]['null'] == frozenset()
    assert m[1]['alias'] == ()
    assert m[2]['s'] == dict(keep_scale=1.0, relu=0x11, rows=30, cols=66, ld=68)
    assert m[2]['null'] == frozenset(['mask', 'res']) and m[2]['alias'] == (('z', 'y'),)


def test_clamp_follows_the_grid():
    r = T._req('egn_adam_step_dev_f32', 't', n=60000000, beta1=0.9, beta2=0.999, eps=1e-8)
    c = T.clamped(r)
    assert c['s']['n'] == 2 * 4096 * 256 + 77 and c['opt']['clamped_from'] == 60000000
    assert T.clamped(T._req('egn_add_f32', 't', n=4096))['s']['n'] == 4096
    assert T.clamped(T._req('egn_add_f32', 't', n=1 << 26))['s']['n'] % 4 == 0


def test_edge_list_names_entry_points_of_the_library():
    names = {r['name'] for r in T.edge_requests()}
    assert names <= set(_lib.SIGNATURES) and names <= T.train_ops_entries()
    assert set(T.ARGS) <= T.train_ops_entries()
    for name, args in T.ARGS.items():        # the argument table against the ABI: pointers where the ABI has them
        types = _lib.SIGNATURES[name][1]
        assert len(types) == len(args) + 1, name
        for (a, role), t in zip(args, types):
            assert (role is not None) == (t is C.c_void_p), (name, a)
    assert T.product_entries() <= set(T.ARGS), T.product_entries() - set(T.ARGS)
    assert set(T.OPTIMIZERS) <= T.product_entries()
