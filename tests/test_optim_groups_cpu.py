"""The grouped optimizer step's own parts, without a GPU: the fp32 emulations against torch's float64 optimizers within
the bounds (and the calibration of the constants), the mutants outside them, the work-table builder, the spec from a
torch optimizer with its refusals, the routing between the old entry points and the grouped one (a stand-in library
records the entry-point names), ``prepare_optim``'s new keys, ``_optim_kwargs`` as it was, and the library's refusals
(validated on the host, so they need no device)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import optim_groups_ref as R
from egonet_amd import _lib, optim, train_common, trainer

CASES = R.edge_cases()


@pytest.fixture(scope='module')
def measured():
    """case id -> (inputs, float64 reference, fp32 emulation), computed once."""
    out = {}
    for c in CASES:
        x = R.inputs(c)
        out[R.case_id(c)] = (x, R.reference(c, x), R.emulate(c, x))
    return out


def test_edge_list_holds_what_it_is_there_for():
    ids = [R.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    sizes = {R.layout_of(c)[3] for c in CASES}
    assert {4, 1020, 1028} <= sizes and max(sizes) > 1024 * 256 * 4
    assert {c['step0'] for c in CASES} == {0, 1, 999}
    long_items = R.tables(R.case('adam', 'long', 0))[1]
    assert list(long_items['length'][:3]) == [R.ITEM, R.ITEM, 520]          # two whole items and a partial last one
    alt = R.tables(R.case('adam', 'alt3', 0))
    assert all(e - b == 4 for b, e, _ in alt[2]) and [k for _, _, k in alt[2]][:6] == [0, 1, 2, 0, 1, 2]
    assert {c['grad'] for c in CASES if c['max_norm'] is not None} == {'below', 'above', 'zero', 'inf'}
    assert R.uses(R.case('sgd_plain', 'n4', 0)) == ()                         # momentum 0: no buffer
    gt = R.tables(R.case('adam_amsgrad', 'alt3', 0))[0]
    assert list(gt['flags']) == [0, optim.AMSGRAD, 0] and gt['lr'][2] == 0 and gt['weight_decay'][1] == 0


def test_float64_formula_is_torchs(measured):
    """The header's formula in float64 and torch.optim agree to 1e-12 of A (they are one statement)."""
    for c in CASES:
        x, want, _ = measured[R.case_id(c)]
        f64 = R.emulate(c, x, torch.float64)
        for name in want:
            worst, unequal = R.ratio(f64[name][0], want[name], f64[name][1])
            assert worst * R.U < 1e-12 and not unequal, (R.case_id(c), name, worst * R.U, unequal)


def test_emulations_within_the_bounds_and_the_constants_calibration(measured):
    worst = {}
    for c in CASES:
        x, want, emu = measured[R.case_id(c)]
        got = {k: v[0] for k, v in emu.items()}
        A = {k: v[1] for k, v in emu.items()}
        assert not R.check(c, got, want, A), R.check(c, got, want, A)
        key = c['variant'] + ('_clip' if c['max_norm'] is not None else '')
        for name in want:
            k2 = 'norm' if name == 'total_norm' else key
            w, _ = R.ratio(got[name], want[name], A[name])
            worst[k2] = max(worst.get(k2, 0.0), w)
    for k in sorted(worst):
        print('%-22s worst emulation ratio %.2f' % (k, worst[k]))
    # the rule of the table: C is four times the measured worst, rounded (+ 6 with sqrtf and the two divisions); with
    # clipping the worst grows by no more than C_CLIP / 4
    for v in R.VARIANTS:
        extra = 0.0 if v.startswith('sgd') else 6.0
        assert abs(R.C_BOUND[v] - extra - 4.0 * worst[v]) <= 1.0, (v, worst[v], R.C_BOUND[v])
        if v + '_clip' in worst:
            assert worst[v + '_clip'] <= worst[v] + R.C_CLIP / 4, (v, worst[v + '_clip'])
    assert worst['norm'] <= 0.75 and R.C_BOUND['norm'] == 2.0


def test_bit_equal_below_max_norm(measured):
    """Norm below max_norm: the coefficient is 1 and the result has the bits of the unclipped run."""
    for c in CASES:
        if c['grad'] != 'below':
            continue
        x = measured[R.case_id(c)][0]
        a, b = R.emulate(c, x), R.emulate(dict(c, max_norm=None), x)
        for name in b:
            assert torch.equal(a[name][0], b[name][0]), (R.case_id(c), name)


@pytest.mark.parametrize('mut', R.MUTANTS)
def test_mutants_break_the_bounds(mut, measured):
    broken = []
    for c in CASES:
        x, want, _ = measured[R.case_id(c)]
        emu = R.emulate(c, x, mut=mut)
        if R.check(c, {k: v[0] for k, v in emu.items()}, want, {k: v[1] for k, v in emu.items()}):
            broken.append(R.case_id(c))
    print('%s: outside the bounds on %d of %d cases' % (mut, len(broken), len(CASES)))
    assert broken, mut


# -- the work-table builder -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', sorted(R.LAYOUTS))
def test_work_table_covers_exactly_once_and_respects_boundaries(layout):
    c = R.case('adam', layout, 0)
    offs, nums, grp, total = R.layout_of(c)
    _, items, segs = R.tables(c)
    assert items['begin'][0] == 0 and int(items['begin'][-1]) + int(items['length'][-1]) == total
    assert np.array_equal(items['begin'][1:], (items['begin'] + items['length'])[:-1])
    assert np.all(items['length'] % 4 == 0) and np.all(items['length'] > 0) and np.all(items['length'] <= R.ITEM)
    bounds = {b for b, _, _ in segs} | {total}
    for b, n in zip(items['begin'], items['length']):
        assert not any(b < s < b + n for s in bounds), (b, n)
    # padding with its parameter: every float from a parameter's start to the next parameter's start has its group
    eg = R.element_groups(c, items)
    for i, (o, k) in enumerate(zip(offs, grp)):
        end = offs[i + 1] if i + 1 < len(offs) else total
        assert bool((eg[o:end] == k).all()), (i, o, end)
    assert total % 4 == 0 and all(o % 4 == 0 for o in offs)


def test_a_parameter_in_no_group_is_refused():
    ps = [torch.zeros(5, requires_grad=True), torch.zeros(3, requires_grad=True)]
    sp = optim.spec('adam', [dict(params=[ps[0]])])
    with pytest.raises(ValueError, match='no parameter group'):
        optim.segments(ps, [0, 8], 12, sp)
    with pytest.raises(ValueError, match='more than one group'):
        optim.spec('adam', [dict(params=[ps[0]]), dict(params=[ps[0]])])


# -- the spec ---------------------------------------------------------------------------------------------------------
def _net():
    return nn.Sequential(nn.Linear(3, 5), nn.BatchNorm1d(5), nn.Linear(5, 2))


def test_spec_from_torch_one_and_three_groups():
    net = _net()
    sp = optim.spec_from_torch(torch.optim.Adam(net.parameters(), lr=2e-3, weight_decay=1e-4))
    assert sp.family == 'adam' and len(sp.groups) == 1 and sp.lrs == [2e-3] and len(sp.groups[0]['params']) == 6
    assert optim.plain_kwargs(sp) == dict(lr=2e-3, optim_type='adam', betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    ps = list(net.parameters())
    o = torch.optim.SGD([dict(params=ps[:2], lr=0.1), dict(params=ps[2:4], lr=0.01, weight_decay=0.0),
                         dict(params=ps[4:], momentum=0.5, nesterov=True)], lr=0.05, momentum=0.9, weight_decay=1e-3,
                        foreach=False)
    sp = optim.spec_from_torch(o)
    assert sp.family == 'sgd' and sp.lrs == [0.1, 0.01, 0.05]
    assert [g['weight_decay'] for g in sp.groups] == [1e-3, 0.0, 1e-3]
    assert [g['nesterov'] for g in sp.groups] == [False, False, True] and sp.groups[2]['momentum'] == 0.5
    assert optim.plain_kwargs(sp) is None
    assert optim.spec_from_torch(torch.optim.AdamW(net.parameters(), amsgrad=True)).family == 'adamw'
    # foreach / capturable / differentiable do not change the arithmetic
    assert optim.spec_from_torch(torch.optim.Adam(net.parameters(), foreach=True)).family == 'adam'


@pytest.mark.parametrize('make,word', [
    (lambda ps: torch.optim.Adam(ps, maximize=True), 'maximize'),
    (lambda ps: torch.optim.SGD(ps, lr=0.1, maximize=True), 'maximize'),
    (lambda ps: torch.optim.Adam(ps, lr=torch.tensor(1e-3)), 'tensor lr'),
    (lambda ps: torch.optim.RMSprop(ps), 'RMSprop'),
    (lambda ps: torch.optim.Adagrad(ps), 'Adagrad'),
    (lambda ps: torch.optim.NAdam(ps), 'NAdam'),
])
def test_spec_from_torch_refusals(make, word):
    with pytest.raises(NotImplementedError, match=word):
        optim.spec_from_torch(make(_net().parameters()))


def test_needs_grouped_is_the_routing_rule():
    net = _net()
    ps = list(net.parameters())
    two = lambda **kw: [dict(params=ps[:2], **kw), dict(params=ps[2:])]
    assert not optim.needs_grouped(torch.optim.Adam(ps, weight_decay=1e-4))
    assert not optim.needs_grouped(torch.optim.SGD(ps, lr=0.1, momentum=0.9))
    assert not optim.needs_grouped(torch.optim.Adam(two(), lr=1e-3))              # two groups, nothing differs
    assert optim.needs_grouped(torch.optim.Adam(two(lr=1e-4), lr=1e-3))           # differing lr alone
    assert optim.needs_grouped(torch.optim.Adam(two(weight_decay=0.0), weight_decay=1e-2))
    assert optim.needs_grouped(torch.optim.AdamW(ps))
    assert optim.needs_grouped(torch.optim.Adam(ps, amsgrad=True))
    assert optim.needs_grouped(torch.optim.SGD(ps, lr=0.1, momentum=0.9, nesterov=True))
    assert optim.needs_grouped(torch.optim.SGD(ps, lr=0.1, momentum=0.9, dampening=0.1))
    assert optim.needs_grouped(torch.optim.Adam(ps), max_grad_norm=1.0)


# -- routing: which entry points a step's update reaches ----------------------------------------------------------------
OLD = {'egn_adam_step_dev_f32', 'egn_adam_l2_step_dev_f32', 'egn_sgd_step_dev_f32'}
NEW = {'egn_optim_grouped_step_f32', 'egn_grad_norm_clip_f32'}


class _Stub(object):
    """Stands in for the library: records the names of the launching entry points, answers the two size queries."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name == 'egn_optim_item_floats':
            return lambda: R.ITEM
        if name == 'egn_grad_norm_ws_bytes':
            return lambda: 8192

        def fn(*a):
            self.calls.append(name)
            return 0
        return fn


class _Step(object):
    """What finish_step and optim.attach read of a native step object."""

    def __init__(self, net, optim_spec=None, max_grad_norm=None, **kw):
        self.model, self.grad_sync = net, None
        self.lr, self.betas, self.eps = kw.get('lr', 1e-3), (0.9, 0.999), 1e-8
        self.optim_type, self.momentum, self.weight_decay = kw.get('optim_type', 'adam'), 0.0, 0.0
        self.flat = train_common.FlatParams(net.parameters())
        optim.attach(self, optim_spec, max_grad_norm)

    def set_lrs(self, lrs):                      # as HRNetTrainStep / LifterTrainStep define it
        optim.set_lrs(self, lrs)


def _reached(monkeypatch, **kw):
    stub = _Stub()
    monkeypatch.setattr(_lib, '_LIB', stub)
    net = _net()
    mk = kw.pop('make', None)
    step = _Step(net, optim_spec=None if mk is None else optim.spec_from_torch(mk(list(net.parameters()))), **kw)
    train_common.finish_step(step, None, True, None)
    return step, set(stub.calls)


def test_routing_between_the_old_entry_points_and_the_grouped_one(monkeypatch):
    step, names = _reached(monkeypatch)
    assert step.grouped is None and names == {'egn_adam_step_dev_f32'}
    step, names = _reached(monkeypatch, make=lambda ps: torch.optim.Adam(ps, lr=3e-3, weight_decay=1e-4))
    assert step.grouped is None and names == {'egn_adam_l2_step_dev_f32'} and step.lr == 3e-3 \
        and step.weight_decay == 1e-4
    step, names = _reached(monkeypatch, make=lambda ps: torch.optim.SGD(
        [dict(params=ps[:2]), dict(params=ps[2:])], lr=0.1, momentum=0.9))
    assert step.grouped is None and names == {'egn_sgd_step_dev_f32'} and step.momentum == 0.9 \
        and step.optim_type == 'sgd'
    # differing lr alone
    step, names = _reached(monkeypatch, make=lambda ps: torch.optim.Adam(
        [dict(params=ps[:2], lr=1e-4), dict(params=ps[2:])], lr=1e-3))
    assert step.grouped is not None and names == {'egn_optim_grouped_step_f32'} and not names & OLD
    assert step.grouped.lrs == [R._f32(1e-4), R._f32(1e-3)]
    step, names = _reached(monkeypatch, max_grad_norm=1.0)
    assert names == NEW
    step, names = _reached(monkeypatch, make=lambda ps: torch.optim.AdamW(ps, amsgrad=True))
    assert names == {'egn_optim_grouped_step_f32'} and step.grouped.vmax is not None


def test_set_lrs_refills_only_on_change(monkeypatch):
    step, _ = _reached(monkeypatch, make=lambda ps: torch.optim.Adam(
        [dict(params=ps[:2], lr=1e-4), dict(params=ps[2:])], lr=1e-3))
    g = step.grouped
    assert not g._dirty
    step.set_lrs([1e-4, 1e-3])
    assert not g._dirty
    step.set_lrs([5e-5, 5e-4])
    assert g._dirty and step.lr == 5e-5
    g.push_lrs()
    table = np.frombuffer(g.groups_dev.numpy().tobytes(), dtype=optim.GROUP_DTYPE)
    assert not g._dirty and list(table['lr']) == [np.float32(5e-5), np.float32(5e-4)]
    with pytest.raises(ValueError):
        step.set_lrs([1e-3])


# -- trainer ------------------------------------------------------------------------------------------------------------
def test_prepare_optim_new_keys():
    net = _net()
    o = dict(lr=0.01, weight_decay=1e-2, momentum=0.9, milestones=[2], gamma=0.5)
    opt, _ = trainer.prepare_optim(net, {'optimizer': dict(o, optim_type='adamw', amsgrad=True)})
    assert type(opt) is torch.optim.AdamW and opt.param_groups[0]['amsgrad'] and len(opt.param_groups) == 1
    opt, sche = trainer.prepare_optim(net, {'optimizer': dict(o, optim_type='adamw', no_decay_norm_bias=True)})
    assert [g['weight_decay'] for g in opt.param_groups] == [1e-2, 0.0]
    assert [tuple(p.shape) for p in opt.param_groups[0]['params']] == [(5, 3), (2, 5)]
    assert sorted(tuple(p.shape) for p in opt.param_groups[1]['params']) == [(2,), (5,), (5,), (5,)]
    assert isinstance(sche, torch.optim.lr_scheduler.MultiStepLR) and optim.needs_grouped(opt)
    opt, _ = trainer.prepare_optim(net, {'optimizer': dict(o, optim_type='sgd', nesterov=True)})
    assert opt.param_groups[0]['nesterov'] and opt.param_groups[0]['dampening'] == 0
    opt, _ = trainer.prepare_optim(net, {'optimizer': dict(o, optim_type='sgd', dampening=0.1)})
    assert opt.param_groups[0]['dampening'] == 0.1 and not opt.param_groups[0]['nesterov']
    assert trainer._max_grad_norm({'optimizer': dict(o, max_grad_norm=2.5)}) == 2.5
    assert trainer._max_grad_norm({'optimizer': o}) is None
    # absent keys: what it always made
    opt, _ = trainer.prepare_optim(net, {'optimizer': dict(o, optim_type='adam')})
    assert type(opt) is torch.optim.Adam and len(opt.param_groups) == 1 and not opt.param_groups[0]['amsgrad']
    assert not optim.needs_grouped(opt)
    with pytest.raises(NotImplementedError):
        trainer.prepare_optim(net, {'optimizer': dict(o, optim_type='rmsprop')})


def test_tool_switches_become_config_keys():
    """--optim / --weight-decay / --no-decay-norm-bias / --max-grad-norm of tools/train_IGRs.py and train_lifting.py."""
    import argparse
    ap = argparse.ArgumentParser()
    trainer.add_optim_arguments(ap)
    assert trainer.optim_keys_from_args(ap.parse_args([])) == {'optim_type': 'adam', 'weight_decay': 0.0}
    a = ap.parse_args(['--optim', 'adamw', '--weight-decay', '0.01', '--no-decay-norm-bias', '--max-grad-norm', '2'])
    keys = trainer.optim_keys_from_args(a)
    assert keys == {'optim_type': 'adamw', 'weight_decay': 0.01, 'no_decay_norm_bias': True, 'max_grad_norm': 2.0}
    opt, _ = trainer.prepare_optim(_net(), {'optimizer': dict(keys, lr=1e-3, milestones=[1], gamma=0.5)})
    assert type(opt) is torch.optim.AdamW and [g['weight_decay'] for g in opt.param_groups] == [0.01, 0.0]
    assert trainer.optim_keys_from_args(argparse.Namespace()) == {'optim_type': 'adam', 'weight_decay': 0.0}
    with pytest.raises(SystemExit):
        ap.parse_args(['--optim', 'rmsprop'])


def test_optim_kwargs_unchanged():
    """The answers tests/test_trainer_cpu.py pins, and the refusals: the grouped path is asked before, not inside."""
    net = nn.Linear(3, 2)
    o = dict(lr=0.01, weight_decay=1e-4, momentum=0.9, milestones=[2], gamma=0.5)
    opt, _ = trainer.prepare_optim(net, {'optimizer': dict(o, optim_type='sgd')})
    assert trainer._optim_kwargs(opt, {}) == dict(optim_type='sgd', momentum=0.9, weight_decay=1e-4)
    opt, _ = trainer.prepare_optim(net, {'optimizer': dict(o, optim_type='adam')})
    assert trainer._optim_kwargs(opt, {}) == dict(optim_type='adam', betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    assert trainer._optim_kwargs(None, {'optimizer': dict(o, optim_type='sgd')}) == \
        dict(optim_type='sgd', momentum=0.9, weight_decay=1e-4)
    for bad in (torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9, nesterov=True),
                torch.optim.Adam(net.parameters(), amsgrad=True), torch.optim.AdamW(net.parameters()),
                torch.optim.Adam([dict(params=[net.weight], weight_decay=0.1), dict(params=[net.bias])])):
        with pytest.raises(NotImplementedError):
            trainer._optim_kwargs(bad, {})


# -- the library's refusals: validated on the host before anything is launched ------------------------------------------
def _host_call(c, edit=None, null=(), n=None, family=None):
    """egn_optim_grouped_step_f32 with aligned fake device addresses and the real host tables (edited)."""
    groups, items, _ = R.tables(c)
    groups, items = groups.copy(), items.copy()
    total = R.layout_of(c)[3]
    if edit:
        edit(groups, items)
    a = {k: C.c_void_p(0x10000 * (i + 1)) for i, k in enumerate(
        ('p', 'g', 'm', 'v', 'vmax', 'groups_dev', 'items_dev', 'clip', 'step_dev'))}
    a['clip'] = None
    for k in null:
        a[k] = None
    fam = optim.FAMILIES[R.group_rows(c)[0]] if family is None else family
    return _lib.lib().egn_optim_grouped_step_f32(
        fam, a['p'], a['g'], a['m'], a['v'], a['vmax'], total if n is None else n, groups.ctypes.data,
        a['groups_dev'], len(groups), items.ctypes.data, a['items_dev'], len(items), a['clip'], a['step_dev'], None)


def _set(table, field, row, value):
    def edit(groups, items):
        (groups if table == 'g' else items)[field][row] = value
    return edit


REFUSALS = [
    ('adam', dict(null=('p',))), ('adam', dict(null=('g',))), ('adam', dict(null=('m',))), ('adam', dict(null=('v',))),
    ('adam', dict(null=('step_dev',))), ('adam', dict(null=('groups_dev',))), ('adam', dict(null=('items_dev',))),
    ('adam_amsgrad', dict(null=('vmax',))),                    # AMSGrad without its buffer
    ('sgd', dict(null=('m',))),                                # momentum without buf
    ('adam', dict(n=0)), ('adam', dict(n=2570)), ('adam', dict(family=3)),
    ('adam', dict(edit=_set('i', 'begin', 1, 1028))),          # a gap
    ('adam', dict(edit=_set('i', 'begin', 1, 1020))),          # an overlap
    ('adam', dict(edit=_set('i', 'length', 3, 16))),           # the last row outside the buffer
    ('adam', dict(edit=_set('i', 'length', 3, 8))),            # ... or short of its end
    ('adam', dict(edit=_set('i', 'length', 0, 2048))),         # longer than an item
    ('adam', dict(edit=_set('i', 'group', 2, 2))), ('adam', dict(edit=_set('i', 'group', 2, -1))),
    ('adam', dict(edit=_set('g', 'beta1', 0, 1.0))), ('adam', dict(edit=_set('g', 'beta2', 1, -0.1))),
    ('adam', dict(edit=_set('g', 'eps', 0, 0.0))), ('adam', dict(edit=_set('g', 'lr', 1, -1e-3))),
    ('adam', dict(edit=_set('g', 'weight_decay', 0, -1.0))), ('adam', dict(edit=_set('g', 'lr', 0, float('nan')))),
    ('adam', dict(edit=_set('g', 'flags', 0, optim.NESTEROV))),
    ('sgd', dict(edit=_set('g', 'momentum', 0, -0.5))), ('sgd', dict(edit=_set('g', 'dampening', 1, 1.5))),
    ('sgd', dict(edit=_set('g', 'flags', 1, optim.NESTEROV))),          # Nesterov with dampening 0.1
    ('sgd_plain', dict(edit=_set('g', 'flags', 0, optim.NESTEROV))),    # Nesterov with momentum 0
    ('sgd', dict(edit=_set('g', 'flags', 0, optim.AMSGRAD))),
]


@pytest.mark.parametrize('variant,kw', REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_refusals_are_badarg_before_any_launch(variant, kw):
    before = _lib.lib().egn_launch_count()
    assert _host_call(R.case(variant, 'long', 1), **kw) == -1
    assert _lib.lib().egn_launch_count() == before


def test_norm_refusals():
    L = _lib.lib()
    p = lambda v: C.c_void_p(v)
    before = L.egn_launch_count()
    assert L.egn_grad_norm_ws_bytes() == 8192 and L.egn_optim_item_floats() == R.ITEM
    for args in ((None, 8, 1.0, p(0x1000), p(0x2000)), (p(0x1004), 8, 1.0, p(0x1000), p(0x2000)),
                 (p(0x1000), 0, 1.0, p(0x1000), p(0x2000)), (p(0x1000), 6, 1.0, p(0x1000), p(0x2000)),
                 (p(0x1000), 8, -1.0, p(0x1000), p(0x2000)), (p(0x1000), 8, float('nan'), p(0x1000), p(0x2000)),
                 (p(0x1000), 8, 1.0, None, p(0x2000)), (p(0x1000), 8, 1.0, p(0x1000), None),
                 (p(0x1000), 8, 1.0, p(0x1000), p(0x2004))):
        assert L.egn_grad_norm_clip_f32(*args, None) == -1, args
    assert L.egn_launch_count() == before
