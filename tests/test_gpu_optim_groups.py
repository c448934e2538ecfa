"""The grouped optimizer step on the device (csrc/optim.hip through egonet_amd/optim.py): every edge case of
tests/optim_groups_ref.py against torch's float64 optimizers within the bounds, between guard bands, twice with the same
bits; the refusals; the tiny HRNet and the tiny lifter stepping with parameter groups and clipping, checked
independently of forward and backward; ``trainer.train`` honouring a second group's learning rate through a
``MultiStepLR`` milestone; a grouped, clipped step inside a hipGraph; the plain step untouched."""
import logging

import numpy as np
import pytest
import torch

import optim_groups_ref as R
from sweep_guards import _guarded, _guards_intact
from egonet_amd import _lib, configs, optim, synth, trainer
from egonet_amd.graph import GraphedStep
from egonet_amd.model import FCmodel
from egonet_amd.model.heatmapModel import hrnet
from egonet_amd.train_hrnet import HRNetTrainStep
from egonet_amd.train_lifter import LifterTrainStep

pytestmark = pytest.mark.gpu

CASES = R.edge_cases()
WRITTEN = ('p', 'm', 'v', 'vmax', 'buf')


@pytest.fixture(autouse=True)
def _no_autotune(monkeypatch):
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')


@pytest.fixture(scope='module')
def wanted():
    """case id -> (inputs, float64 reference, A): computed once on the CPU, shared, never changed."""
    out = {}
    for c in CASES:
        x = R.inputs(c)
        out[R.case_id(c)] = (x, R.reference(c, x), {k: v[1] for k, v in R.emulate(c, x).items()})
    return out


def _launch(c, x):
    """One step of the case on the device -> (name -> result on the CPU, guards intact, launches counted)."""
    L = _lib.lib()
    fam, _ = R.group_rows(c)
    groups, items, _ = R.tables(c)
    total = R.layout_of(c)[3]
    dev = {'g': x['g'].cuda()}
    whole = {}
    for a in WRITTEN:
        if a in x:
            whole[a], dev[a] = _guarded(total, torch.float32, None)
            dev[a].copy_(x[a])
    clip = ws = None
    if c['max_norm'] is not None:
        whole['clip'], clip = _guarded(2, torch.float32, -7.0)
        ws = optim.norm_workspace('cuda')
    step_dev = torch.tensor([c['step0']], dtype=torch.int32, device='cuda')
    groups_dev, items_dev = optim._to_device(groups, 'cuda'), optim._to_device(items, 'cuda')
    before = L.egn_launch_count()
    if clip is not None:
        _lib.check(optim.grad_norm_clip(dev['g'], total, c['max_norm'], ws, clip, None), 'norm')
    m = dev.get('buf') if fam == 'sgd' else dev.get('m')
    _lib.check(optim.grouped_step(fam, dev['p'], dev['g'], m, dev.get('v'), dev.get('vmax'), total, groups, groups_dev,
                                  items, items_dev, clip, step_dev, None), 'step')
    torch.cuda.synchronize()
    got = {a: dev[a].cpu() for a in WRITTEN if a in x}
    if clip is not None:
        got['total_norm'] = clip[:1].cpu()
        got['coef'] = clip[1:].cpu()
    assert int(step_dev.item()) == c['step0'] + 1
    assert torch.equal(dev['g'].cpu(), x['g'])                        # the gradient keeps its unclipped values
    return got, all(_guards_intact(w) for w in whole.values()), L.egn_launch_count() - before


def test_item_size_is_the_helpers():
    assert _lib.lib().egn_optim_item_floats() == R.ITEM


@pytest.mark.parametrize('c', CASES, ids=[R.case_id(c) for c in CASES])
def test_edge_case_against_float64_within_bounds_between_guards_twice(c, wanted):
    x, want, A = wanted[R.case_id(c)]
    got, intact, launches = _launch(c, x)
    assert intact, 'a write outside its buffer'
    assert launches == (4 if c['max_norm'] is not None else 2)        # norm + finish, tick + ONE update
    for name in want:
        print('%s %-10s worst ratio %.2f' % (R.case_id(c), name, R.ratio(got[name], want[name], A[name])[0]))
    bad = R.check(c, got, want, A)
    assert not bad, bad
    if c['max_norm'] is not None and c['grad'] in ('below', 'zero') and c['max_norm'] > 0:
        assert float(got['coef']) == 1.0
        plain, _, _ = _launch(dict(c, max_norm=None), x)
        for name in plain:
            assert torch.equal(plain[name], got[name]), name          # coefficient 1: the bits of the unclipped run
    again, intact, _ = _launch(c, x)
    assert intact
    for name in got:
        assert torch.equal(got[name].view(torch.int32), again[name].view(torch.int32)), name


def test_refusals_return_badarg_and_launch_nothing():
    L = _lib.lib()
    c = R.case('adam_amsgrad', 'long', 1)
    groups, items, _ = R.tables(c)
    total = R.layout_of(c)[3]
    t = lambda: torch.zeros(total + 4, device='cuda')
    p, g, m, v, vmax = t(), t(), t(), t(), t()
    step_dev = torch.zeros(1, dtype=torch.int32, device='cuda')
    gd, idev = optim._to_device(groups, 'cuda'), optim._to_device(items, 'cuda')

    def call(fam='adam', p=p, m=m, vmax=vmax, n=total, groups=groups, items=items):
        return optim.grouped_step(fam, p, g, m, v, vmax, n, groups, gd, items, idev, None, step_dev, None)

    def edited(table, field, row, value):
        t2 = table.copy()
        t2[field][row] = value
        return t2

    before = L.egn_launch_count()
    assert call(vmax=None) == -1                                       # AMSGrad without its buffer
    assert call(p=p[1:]) == -1                                         # misaligned
    assert call(m=None) == -1
    assert call(n=total + 2) == -1
    assert call(items=edited(items, 'begin', 1, 1028)) == -1           # a gap
    assert call(items=edited(items, 'length', len(items) - 1, 16)) == -1      # a row outside the buffer
    assert call(items=edited(items, 'group', 0, 2)) == -1              # a group index outside the table
    assert call(groups=edited(groups, 'beta2', 0, 1.0)) == -1
    assert call(groups=edited(groups, 'eps', 1, 0.0)) == -1
    assert call(groups=edited(groups, 'lr', 0, -1.0)) == -1
    sgd = R.tables(R.case('sgd_nesterov', 'long', 1))[0]
    assert call(fam='sgd', groups=sgd, m=None) == -1                   # momentum without buf
    assert call(fam='sgd', groups=edited(sgd, 'dampening', 0, 0.1)) == -1     # Nesterov with dampening
    assert call(fam='sgd', groups=edited(sgd, 'momentum', 0, 0.0)) == -1      # Nesterov without momentum
    assert optim.grad_norm_clip(g[1:], total, 1.0, optim.norm_workspace('cuda'), torch.zeros(2, device='cuda'),
                                None) == -1
    assert optim.grad_norm_clip(g, total, -1.0, optim.norm_workspace('cuda'), torch.zeros(2, device='cuda'), None) == -1
    torch.cuda.synchronize()
    assert L.egn_launch_count() == before and int(step_dev.item()) == 0
    assert call() == 0 and L.egn_launch_count() == before + 2
    torch.cuda.synchronize()


# -- the native steps ---------------------------------------------------------------------------------------------------
def _hrnet(seed=9):
    cfg = configs.tiny_config('coordinates')
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=seed))
    return net.cuda()


def _hrnet_batches(n):
    gen = torch.Generator().manual_seed(2)
    xs = [synth.synth_crops(2, 3, 64, 64, seed=40 + i).cuda() for i in range(n)]
    tg = torch.rand(n, 2, 5, 16, 16, generator=gen).cuda()
    jt = (torch.rand(n, 2, 5, 2, generator=gen) * 64).cuda()
    return [(xs[i], tg[i], jt[i]) for i in range(n)]


def _lifter(seed=3):
    torch.manual_seed(seed)
    cfg = configs.tiny_config()
    cfg['FCModel']['dropout'] = 0.0
    return FCmodel.get_fc_model(1, cfg, 10, 12).cuda()


def _lifter_batches(n):
    gen = torch.Generator().manual_seed(5)
    return [(torch.randn(32, 10, generator=gen).cuda(), torch.randn(32, 12, generator=gen).cuda()) for _ in range(n)]


def _configurations(net):
    """name -> (variant of the constant, family, group dicts with params, max_grad_norm)."""
    ps = [p for p in net.parameters() if p.requires_grad]
    third = len(ps) // 3
    return {
        'adamw-no-decay-clip': ('adamw', 'adamw', optim.no_decay_groups(net, 1e-2, lr=1e-3), 1e-3),
        'sgd-nesterov-three-lrs': ('sgd_nesterov', 'sgd', [
            dict(params=ps[:third], lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-3),
            dict(params=ps[third:2 * third], lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-3),
            dict(params=ps[2 * third:], lr=1e-4, momentum=0.9, nesterov=True, weight_decay=1e-3)], None),
    }


def _check_two_steps(step, batches, variant, family, groups, max_norm):
    """Independent of forward and backward: the state before each update and the gradient the step left (the update
    only reads it) -> torch's float64 optimizer -> the state after."""
    flat, gu = step.flat, step.grouped
    assert gu is not None
    owner = {id(p): k for k, g in enumerate(groups) for p in g['params']}
    params = [(p.numel(), owner[id(p)]) for p in flat.params]
    rows = [{k: v for k, v in g.items() if k != 'params'} for g in groups]
    rows = [dict(optim._DEFAULTS[family], **r) for r in rows]
    names = {'p': flat.flat, 'm': flat.m, 'v': flat.v, 'vmax': gu.vmax, 'buf': flat.m}
    L = _lib.lib()
    for it, batch in enumerate(batches):
        c = R.problem(variant, family, rows, params, it, max_norm)
        x = {a: names[a].detach().cpu().clone() for a in ('p',) + R.uses(c)}
        n0 = L.egn_launch_count()
        step.step(*batch)
        torch.cuda.synchronize()
        x['g'] = flat.grad.detach().cpu().clone()
        assert flat.t == it + 1
        want = R.reference(c, x)
        A = {k: v[1] for k, v in R.emulate(c, x).items()}
        got = {a: names[a].detach().cpu() for a in ('p',) + R.uses(c)}
        if max_norm is not None:
            assert step.last_grad_norm.is_cuda                         # the device scalar: nothing was read back
            got['total_norm'] = step.last_grad_norm.detach().cpu().reshape(1)
            assert 0.0 < float(gu.clip[1]) < 1.0                       # the norm is above max_grad_norm: it clips
        bad = R.check(c, got, want, A)
        assert not bad, bad
        assert L.egn_launch_count() > n0
        if it == 0 and family == 'sgd':
            # group 1's parameters moved by group 1's rate: first Nesterov step, dp = -lr (1 + mu) (g + wd p)
            eg = R.element_groups(c)
            r1 = R._hp(**rows[1])
            sel = (eg == 1) & (x['g'].abs() > 1e-6)
            assert int(sel.sum()) > 10
            dp = (got['p'].double() - x['p'].double())[sel]
            unit = -(1 + r1['momentum']) * (x['g'].double() + r1['weight_decay'] * x['p'].double())[sel]
            rate = float((dp * unit).sum() / (unit * unit).sum())
            assert abs(rate / r1['lr'] - 1) < 2e-2, (rate, r1['lr'])
            assert abs(rate / R._f32(rows[0]['lr']) - 1) > 0.5


@pytest.mark.parametrize('name', ['adamw-no-decay-clip', 'sgd-nesterov-three-lrs'])
def test_tiny_hrnet_steps_with_groups(name):
    net = _hrnet()
    variant, family, groups, max_norm = _configurations(net)[name]
    step = HRNetTrainStep(net, optim_spec=optim.spec(family, groups), max_grad_norm=max_norm)
    _check_two_steps(step, _hrnet_batches(2), variant, family, groups, max_norm)


@pytest.mark.parametrize('name', ['adamw-no-decay-clip', 'sgd-nesterov-three-lrs'])
def test_tiny_lifter_steps_with_groups(name):
    net = _lifter()
    variant, family, groups, max_norm = _configurations(net)[name]
    step = LifterTrainStep(net, optim_spec=optim.spec(family, groups), max_grad_norm=max_norm)
    _check_two_steps(step, _lifter_batches(2), variant, family, groups, max_norm)


def test_a_parameter_in_no_group_is_refused_by_the_step():
    net = _lifter()
    ps = list(net.parameters())
    with pytest.raises(ValueError, match='no parameter group'):
        LifterTrainStep(net, optim_spec=optim.spec('adam', [dict(params=ps[:-1])]))


# -- trainer.train: a second group's learning rate through the schedule ----------------------------------------------------
class _CropSet(torch.utils.data.Dataset):
    def __init__(self, n=8):
        g = torch.Generator().manual_seed(1)
        self.x = synth.synth_crops(n, 3, 64, 64, seed=3)
        self.t = torch.rand(n, 5, 16, 16, generator=g)
        self.j = torch.rand(n, 5, 3, generator=g) * 64

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.t[i], torch.ones(5, 1), {'transformed_joints': self.j[i].numpy()}


def _train_two_epochs(monkeypatch, lr1):
    cfg = configs.clone(configs.tiny_config('coordinates'))
    cfg.update(use_gpu=True, exp_type='test', cascade={'num_stages': 1},
               optimizer={'optim_type': 'adam', 'lr': 4e-3, 'weight_decay': 0.0, 'milestones': [1], 'gamma': 0.5},
               training_settings={'total_epochs': 2, 'batch_size': 4, 'num_threads': 0, 'shuffle': False,
                                  'report_every': 1, 'eval_during': False, 'plot_loss': False})
    net = _hrnet()
    ps = list(net.parameters())
    half = len(ps) // 2
    opt = torch.optim.Adam([dict(params=ps[:half], lr=4e-3), dict(params=ps[half:], lr=lr1)])
    sche = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.5)
    made = []
    real = trainer.make_step
    monkeypatch.setattr(trainer, 'make_step', lambda *a, **k: made.append(real(*a, **k)) or made[-1])
    lg = logging.getLogger('egonet_amd.test_optim_groups')
    lg.handlers = [logging.NullHandler()]
    trainer.train(_CropSet(), net, None, opt, sche, cfg, lg)
    torch.cuda.synchronize()
    return made[-1], [p.detach().cpu().clone() for p in ps], half, opt


def test_trainer_train_honours_the_second_groups_learning_rate(monkeypatch):
    step, ps, half, opt = _train_two_epochs(monkeypatch, 1e-3)
    assert step.grouped is not None
    table = np.frombuffer(step.grouped.groups_dev.cpu().numpy().tobytes(), dtype=optim.GROUP_DTYPE)
    sched = [g['lr'] for g in opt.param_groups]
    assert sched == [2e-3, 5e-4]                                       # the milestone has passed for both groups
    assert list(table['lr']) == [np.float32(v) for v in sched]
    step_b, ps_b, _, _ = _train_two_epochs(monkeypatch, 4e-3)          # group 1 at group 0's rate: the old behaviour
    assert step_b.grouped is None                                      # nothing differs: the old entry points
    assert any(not torch.equal(a, b) for a, b in zip(ps[half:], ps_b[half:]))


# -- hipGraph -------------------------------------------------------------------------------------------------------------
def test_graphed_grouped_clipped_step_equals_eager_steps():
    batches = _hrnet_batches(3)
    lrs = [[1e-3, 1e-4], [5e-4, 5e-5]]
    out = []
    for graphed in (False, True):
        net = _hrnet()
        groups = optim.no_decay_groups(net, 1e-2)
        groups[1]['lr'] = 1e-4
        step = HRNetTrainStep(net, optim_spec=optim.spec('adamw', groups, lr=1e-3, amsgrad=True), max_grad_norm=0.05)
        run = GraphedStep(step, *batches[0], warmup=1) if graphed else step.step
        for it in (1, 2):
            step.set_lrs(lrs[it - 1])                                  # the scheduler between two iterations
            run(*batches[it])
        torch.cuda.synchronize()
        out.append((step.flat.t, [t.detach().cpu().clone() for t in
                                  (step.flat.flat, step.flat.m, step.flat.v, step.grouped.vmax, step.grouped.clip)]))
        if graphed:
            run.close()
    assert out[0][0] == out[1][0] == 2
    for a, b in zip(out[0][1], out[1][1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# -- the plain step ---------------------------------------------------------------------------------------------------------
def test_plain_step_is_untouched_by_the_grouped_path():
    L = _lib.lib()
    batch = _hrnet_batches(1)[0]

    def plain():
        net = _hrnet()
        step = HRNetTrainStep(net)
        assert step.grouped is None
        n0 = L.egn_launch_count()
        step.step(*batch)
        torch.cuda.synchronize()
        return L.egn_launch_count() - n0, step.flat.flat.detach().cpu().clone()

    plain()                                                            # (one-time initialisations are not the subject)
    n_a, p_a = plain()
    c = R.case('adamw_amsgrad', 'alt3', 1, 0.5, 'above')
    _launch(c, R.inputs(c))                                            # the grouped path, elsewhere in the process
    n_b, p_b = plain()
    assert n_a == n_b and torch.equal(p_a, p_b)
    # an expressible spec is the plain step too: the same launches, the same bits
    net = _hrnet()
    step = HRNetTrainStep(net, optim_spec=optim.spec('adam', [dict(params=list(net.parameters()))]))
    assert step.grouped is None
    n0 = L.egn_launch_count()
    step.step(*batch)
    torch.cuda.synchronize()
    assert L.egn_launch_count() - n0 == n_a and torch.equal(step.flat.flat.detach().cpu(), p_a)
