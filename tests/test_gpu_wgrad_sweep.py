"""Every weight-gradient kernel the dispatch can launch, element by element against float64.

The requests are the product's (tests/wgrad_sweep.py: derived on the host from the torch modules, and proven here to
be what real training steps pass to egn_conv2d_wgrad_f32) plus a supplement for the table rows no product request
selects (tests/test_wgrad_sweep_cpu.py proves that together they reach every row, reduce width, slab order and
shrink branch).  Per request: the workspace is exactly egn_conv2d_wgrad_ws_bytes, filled with 1e30 before each
launch (a slab region the reduce reads but the kernel did not write shows), guard words around the workspace and dw
come back untouched, two launches into differently pre-filled dw agree bit for bit, and EVERY element of dw is within
C_BOUND[form] * 2^-24 * A of ``train_checks.wgrad_ref64`` computed on the device (wgrad_sweep.C_BOUND)."""
import inspect
import os

import pytest
import torch

from egonet_amd import _lib

import wgrad_sweep as S

pytestmark = pytest.mark.gpu

GUARD = 64                    # floats in front of and behind a buffer (256 B: the slabs stay 16 B aligned)
GUARD_VALUE = -2.5e29
SENTINEL = 1e30


def _st():
    return _lib.current_stream()


class _Guarded(object):
    """A device buffer of ``numel`` floats between two guard zones."""

    def __init__(self, numel):
        self.numel = numel
        self.all = torch.empty(numel + 2 * GUARD, device='cuda')
        self.all.fill_(GUARD_VALUE)
        self.body = self.all[GUARD:GUARD + numel]

    def fill(self, v):
        self.body.fill_(v)
        return self

    def guards_intact(self):
        return bool((self.all[:GUARD] == GUARD_VALUE).all()) and bool((self.all[GUARD + self.numel:] == GUARD_VALUE).all())


def _launch(key, x, dy, dw, ws, ws_bytes):
    n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad = key
    _lib.check(_lib.lib().egn_conv2d_wgrad_f32(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw.body), n, h, w, cin, cs_in, cout,
                                               cs_out, kh, kw, stride, pad, _lib.ptr(ws.body), ws_bytes, _st()), 'wgrad')


def _bits(t):
    return t.view(torch.int32)


def _run_private(key, x, dy):
    """The request with a private, sentinel-filled, exactly sized workspace: (dw [Cout,Cin,KH,KW], problems)."""
    n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad = key
    need = S.ws_bytes(key)
    assert need > 0 and need % 4 == 0, (key, need)
    ws = _Guarded(need // 4)
    outs, problems = [], []
    for prefill in (3.0, -7.0e29):
        ws.fill(SENTINEL)
        dw = _Guarded(cout * cin * kh * kw).fill(prefill)
        _launch(key, x, dy, dw, ws, need)
        torch.cuda.synchronize()
        if not (ws.guards_intact() and dw.guards_intact()):
            problems.append('a guard word around the workspace or dw was overwritten')
        outs.append(dw.body.clone().view(cout, cin, kh, kw))
    if not torch.equal(_bits(outs[0]), _bits(outs[1])):
        problems.append('two launches into differently pre-filled dw differ in %d elements'
                        % int((_bits(outs[0]) != _bits(outs[1])).sum()))
    return outs[0], problems


def _sweep(reqs, tag):
    failures, worst_frac, rows = [], {}, set()
    for r in reqs:
        key = r['key']
        p = S.plan(key)
        assert p is not None, r
        gen = torch.Generator().manual_seed(sum((i + 1) * v for i, v in enumerate(key)))
        x, dy = S.inputs(key, gen, 'cuda')
        got, problems = _run_private(key, x, dy)
        want, A = S.reference(key, x, dy)
        ratio, (co, ci, tap) = S.worst(got, want, A, p['form'])       # no element excluded
        C = S.C_BOUND[p['form']]
        rows.add(p['row'])
        kind = 'Winograd' if p['form'] else 'direct'
        worst_frac[kind] = max(worst_frac.get(kind, 0.0), ratio / C)
        if ratio > C:
            problems.append('element (co %d, ci %d, tap %d): |dw - dw64| = %.1f U A, bound %.0f' % (co, ci, tap, ratio, C))
        if problems:
            failures.append(dict(request=key, seen=r['src'], row=p['row'], form=S.FORM_NAMES[p['form']],
                                 plan=S.plan_tuple(p), problems=problems))
    print('wgrad sweep %s: %d requests, table rows %s, worst ratio / bound %s'
          % (tag, len(reqs), sorted(rows), {k: round(v, 3) for k, v in sorted(worst_frac.items())}))
    assert not failures, '\n'.join(str(f) for f in failures)


# (static: collecting this module runs no model)
GROUPS = [name for name, _, _ in S.conv_sweep.INFERENCE_MODELS] + ['lifter', 'supplement']


@pytest.mark.parametrize('group', GROUPS)
def test_every_request_within_the_elementwise_bound(group):
    reqs = S.supplement_requests() if group == 'supplement' else dict(S.corpus())[group]
    _sweep(reqs, group)


def test_launches_sharing_one_workspace_equal_private_workspaces():
    """The tape shares one workspace across all launches of a step (train_hrnet.TapeOwner.wgrad_ws), sized for the
    largest and never cleared: a Winograd pairs request, a direct 3x3 and a 1x1 back to back, each bit-identical to
    its result with a private, sentinel-filled workspace."""
    keys = [(3, 8, 8, 96, 96, 48, 48, 3, 3, 1, 1),         # Winograd, image pairs, odd batch
            (2, 16, 16, 64, 64, 66, 68, 3, 3, 2, 1),       # direct 3x3
            (3, 16, 16, 96, 96, 33, 36, 1, 1, 1, 0)]       # 1x1
    plans = [S.plan(k) for k in keys]
    assert [p['form'] for p in plans] == [2, 0, 0] and plans[1]['row'] != plans[2]['row']
    data, private = [], []
    for key in keys:
        gen = torch.Generator().manual_seed(sum(key))
        x, dy = S.inputs(key, gen, 'cuda')
        data.append((x, dy))
        got, problems = _run_private(key, x, dy)
        assert not problems, (key, problems)
        private.append(got)
    size = max(S.ws_bytes(k) for k in keys)
    ws = _Guarded(size // 4).fill(SENTINEL)
    for order in ((0, 1, 2), (2, 1, 0), (1, 0, 2)):
        for i in order:                                    # (not refilled in between)
            key = keys[i]
            n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad = key
            dw = _Guarded(cout * cin * kh * kw).fill(0.0)
            _launch(key, data[i][0], data[i][1], dw, ws, size)
            torch.cuda.synchronize()
            assert ws.guards_intact() and dw.guards_intact()
            assert torch.equal(_bits(dw.body.view(cout, cin, kh, kw)), _bits(private[i])), (key, order)


# ---------------------------------------------------------------------------------------------------------------
# the corpus is real: what training steps pass to egn_conv2d_wgrad_f32 is what the host derivation says
# ---------------------------------------------------------------------------------------------------------------
class _WgradRecorder(object):
    """Context manager: wraps ``_Tape._wgrad`` and ``LifterCore._wgrad`` the way conv_sweep.TapeRecorder wraps
    the conv launch; records the (n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad) of every call."""

    def __init__(self):
        self.keys = []

    def __enter__(self):
        from egonet_amd import train_hrnet as T, train_lifter as TL
        self._T, self._TL = T, TL
        self._orig = (T._Tape._wgrad, TL.LifterCore._wgrad)
        orig_t, orig_l = self._orig
        me = self

        def named(fn, args, kw):
            call = inspect.signature(fn).bind(*args, **kw)
            call.apply_defaults()
            return call.arguments

        def tape_wgrad(*args, **kw):
            c = named(orig_t, args, kw)
            cout, cin, kh, kw_ = c['weight'].shape
            x = c['x']
            me.keys.append((x.n, x.h, x.w, cin, x.cs, cout, c['cs_out'], kh, kw_, c['stride'], c['pad']))
            return orig_t(*args, **kw)

        def lifter_wgrad(*args, **kw):
            c = named(orig_l, args, kw)
            me.keys.append((c['rows'], 1, 1, c['inf'], c['ld_a'], c['outf'], c['ld_dz'], 1, 1, 1, 0))
            return orig_l(*args, **kw)

        T._Tape._wgrad, TL.LifterCore._wgrad = tape_wgrad, lifter_wgrad
        return self

    def __exit__(self, *exc):
        self._T._Tape._wgrad, self._TL.LifterCore._wgrad = self._orig
        return False


@pytest.fixture
def no_autotune():
    # (only which requests are made matters here, not what the tuner answers: no timing of shapes off the table)
    prev = os.environ.get('EGONET_AMD_AUTOTUNE')
    os.environ['EGONET_AMD_AUTOTUNE'] = '0'
    yield
    if prev is None:
        del os.environ['EGONET_AMD_AUTOTUNE']
    else:
        os.environ['EGONET_AMD_AUTOTUNE'] = prev


@pytest.mark.parametrize('name,n', [('tiny', 3), ('ped', 2)])
def test_a_training_step_makes_the_host_derived_requests(name, n, no_autotune):
    from egonet_amd.model.heatmapModel import hrnet
    from egonet_amd.train_hrnet import HRNetTrainStep
    cfg = S.model_config(name)
    g = torch.Generator().manual_seed(0)
    net = hrnet.get_pose_net(cfg, is_train=False).cuda().train()
    iw, ih = cfg['heatmapModel']['input_size']
    hw, hh = cfg['heatmapModel']['heatmap_size']
    J = cfg['heatmapModel']['num_joints']
    x = torch.randn(n, 3, ih, iw, generator=g).cuda()
    tgt = torch.rand(n, J, hh, hw, generator=g).cuda()
    jxy = (torch.rand(n, J, 2, generator=g) * iw).cuda()
    tr = HRNetTrainStep(net, lr=1e-3, w_coor=0.1)
    with _WgradRecorder() as rec:
        tr.step(x, tgt, jxy, update=False)
    torch.cuda.synchronize()
    want = [r['key'] for r in S.hrnet_requests(name, cfg, (n,))]
    # one launch per trainable Conv2d / Linear, the same shapes with the same channel strides
    assert sorted(rec.keys) == sorted(want), (sorted(set(rec.keys) - set(want)), sorted(set(want) - set(rec.keys)))


def test_a_lifter_step_makes_the_host_derived_requests():
    from egonet_amd.train_lifter import LifterTrainStep
    g = torch.Generator().manual_seed(0)
    tr = LifterTrainStep(S.lifter_model().cuda().train(), lr=1e-3)
    with _WgradRecorder() as rec:
        tr.step(torch.randn(7, 66, generator=g).cuda(), torch.randn(7, 96, generator=g).cuda(), update=False)
    torch.cuda.synchronize()
    want = [r['key'] for r in S.lifter_requests((7,))]
    assert sorted(rec.keys) == sorted(want), (sorted(set(rec.keys) - set(want)), sorted(set(want) - set(rec.keys)))
