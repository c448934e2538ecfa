"""Save / resume of the native training steps, the parts that need no GPU (egonet_amd/train_state.py and the checkpoint
helpers of egonet_amd/trainer.py): the mapping between the padded flat buffers and ``torch.optim`` state dicts, every
refusal, files that load with ``weights_only=True`` and bring the generators back, the per-rank files under two gloo
ranks, the tools' switches."""
import argparse
import os
import random
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from egonet_amd import _lib, optim, train_common, train_state, trainer

SENTINEL = -777.0


class _Stub(object):
    """Stands in for the library where a GroupedUpdate asks it for its item size; nothing here launches."""

    def __getattr__(self, name):
        if name == 'egn_optim_item_floats':
            return lambda: 1024
        if name == 'egn_grad_norm_ws_bytes':
            return lambda: 8192
        raise AssertionError('the save / resume code called %s' % name)


class _Net(torch.nn.Module):
    """5, 8 and 3 elements: padding after the first and the last (offsets 0, 8, 16 of 20 floats)."""

    def __init__(self, shapes=(('a', (5,)), ('b', (2, 4)), ('c', (3,))), seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        for name, shape in shapes:
            setattr(self, name, torch.nn.Parameter(torch.randn(*shape, generator=g)))


class _Step(object):
    """What train_state reads of a native step object, over CPU tensors."""

    def __init__(self, net, optim_spec=None, max_grad_norm=None, kind='hrnet', **kw):
        self.model, self.grad_sync, self.state_kind = net, None, kind
        self.lr, self.betas, self.eps = kw.get('lr', 1e-3), kw.get('betas', (0.9, 0.999)), 1e-8
        self.optim_type, self.momentum = kw.get('optim_type', 'adam'), kw.get('momentum', 0.0)
        self.weight_decay = kw.get('weight_decay', 0.0)
        self.flat = train_common.FlatParams(net.parameters())
        optim.attach(self, optim_spec, max_grad_norm)
        if kind == 'hrnet':
            self.apply_cr_loss = False
        else:
            self.drop_seed, self._noupdate_forwards = 1234567890123456789, 0

    def set_lrs(self, lrs):
        optim.set_lrs(self, lrs)

    def state_dict(self):
        return train_state.state_dict(self)

    def load_state_dict(self, sd, strict=True):
        train_state.load_state_dict(self, sd, strict)


def _groups(net, family):
    """Two groups that interleave in the flat buffer: torch numbers a = 0, c = 1, b = 2."""
    if family == 'sgd':
        return [dict(params=[net.a, net.c], lr=1e-2, momentum=0.9), dict(params=[net.b], lr=1e-3, momentum=0.8)]
    return [dict(params=[net.a, net.c], lr=1e-3, amsgrad=True), dict(params=[net.b], lr=1e-4, betas=(0.8, 0.99),
                                                                     amsgrad=True)]


CONFIGS = {
    'adam-plain': dict(family='adam', grouped=False, cls=torch.optim.Adam, kw={}),
    'adamw-amsgrad-groups': dict(family='adamw', grouped=True, cls=torch.optim.AdamW, kw=dict(amsgrad=True)),
    'sgd-momentum-plain': dict(family='sgd', grouped=False, cls=torch.optim.SGD, kw=dict(momentum=0.9)),
}


def _make(name, monkeypatch, net=None, kind='hrnet'):
    monkeypatch.setattr(_lib, '_LIB', _Stub())
    c = CONFIGS[name]
    net = net or _Net()
    if c['grouped']:
        step = _Step(net, optim_spec=optim.spec(c['family'], _groups(net, c['family'])), kind=kind)
        assert step.grouped is not None
    else:
        step = _Step(net, optim_type=c['family'], momentum=c['kw'].get('momentum', 0.0), kind=kind)
        assert step.grouped is None
    return step


def _torch_optimizer(name, net):
    c = CONFIGS[name]
    if c['grouped']:
        return c['cls'](_groups(net, c['family']))
    return c['cls'](list(net.parameters()), lr=1e-3, **c['kw'])


def _fill(step, count):
    """Distinct values in every element, the sentinel in the padding, the counter at ``count``."""
    f = step.flat
    own = torch.zeros(f.numel, dtype=torch.bool)
    for i in range(len(f.params)):
        f.cut(own, i).fill_(True)
    assert int((~own).sum()) == 4                                       # 3 floats after a, 1 after c
    bufs = [f.m, f.v] + ([step.grouped.vmax] if step.grouped is not None and step.grouped.vmax is not None else [])
    for k, buf in enumerate(bufs):
        buf.copy_(torch.arange(f.numel, dtype=torch.float32) + 1 + 100 * k)
        buf[~own] = SENTINEL
    f.step_dev.fill_(count)
    return own


def _same(a, b):
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape \
            and torch.equal(a.cpu().reshape(-1).view(torch.uint8), b.cpu().reshape(-1).view(torch.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


# -- 1. export / import mapping ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CONFIGS))
def test_export_holds_each_parameters_own_elements_and_import_inverts_it(name, monkeypatch):
    step = _make(name, monkeypatch)
    own = _fill(step, 7)
    sd = train_state.optimizer_state_dict(step)
    net, f = step.model, step.flat
    order = [net.a, net.c, net.b] if CONFIGS[name]['grouped'] else [net.a, net.b, net.c]
    where = {id(p): i for i, p in enumerate(f.params)}
    assert sorted(sd['state']) == [0, 1, 2]
    keys = {'momentum_buffer': f.m} if CONFIGS[name]['family'] == 'sgd' else {'exp_avg': f.m, 'exp_avg_sq': f.v}
    if name == 'adamw-amsgrad-groups':
        keys['max_exp_avg_sq'] = step.grouped.vmax
    for idx, p in enumerate(order):
        ent = sd['state'][idx]
        assert set(ent) == set(keys) | ({'step'} if 'exp_avg' in keys else set())
        for k, buf in keys.items():
            assert ent[k].shape == p.shape and torch.equal(ent[k], f.cut(buf, where[id(p)]))
            assert ent[k].data_ptr() != f.cut(buf, where[id(p)]).data_ptr()        # a copy
            assert not bool((ent[k] == SENTINEL).any())
        if 'step' in ent:
            assert float(ent['step']) == 7.0
    # into a second object: the flat buffers with zero padding, the counter, the learning rates
    other = _make(name, monkeypatch, net=_Net(seed=1))
    _fill(other, 3)
    train_state.load_optimizer_state_dict(other, sd)
    bufs = [('m', f.m, other.flat.m)] + ([] if CONFIGS[name]['family'] == 'sgd' else [('v', f.v, other.flat.v)])
    if name == 'adamw-amsgrad-groups':
        bufs.append(('vmax', step.grouped.vmax, other.grouped.vmax))
    for label, a, b in bufs:
        assert torch.equal(a[own], b[own]), label
        assert bool((b[~own] == 0).all()), label
    assert other.flat.t == (7 if CONFIGS[name]['family'] != 'sgd' else 1)          # SGD dicts carry no counter
    assert _same(train_state.optimizer_state_dict(other)['state'], sd['state'])


@pytest.mark.parametrize('name', list(CONFIGS))
def test_exported_dict_loads_into_the_installed_torch_optimizer_as_is(name, monkeypatch):
    step = _make(name, monkeypatch)
    _fill(step, 7)
    sd = train_state.optimizer_state_dict(step)
    opt = _torch_optimizer(name, step.model)
    opt.load_state_dict(sd)
    back = opt.state_dict()
    assert _same(back, sd), (back, sd)
    # and torch's own dict comes back in: the same buffers
    other = _make(name, monkeypatch, net=_Net(seed=1))
    train_state.load_optimizer_state_dict(other, back)
    assert _same(train_state.optimizer_state_dict(other)['state'], sd['state'])


def test_a_fresh_optimizer_exports_and_imports_as_empty(monkeypatch):
    step = _make('adamw-amsgrad-groups', monkeypatch)
    assert train_state.optimizer_state_dict(step)['state'] == {}
    _fill(step, 5)
    train_state.load_optimizer_state_dict(step, _torch_optimizer('adamw-amsgrad-groups', step.model).state_dict())
    assert step.flat.t == 0
    for buf in (step.flat.m, step.flat.v, step.grouped.vmax):
        assert bool((buf == 0).all())


def test_step_is_taken_as_int_float_or_tensor(monkeypatch):
    step = _make('adam-plain', monkeypatch)
    _fill(step, 4)
    sd = train_state.optimizer_state_dict(step)
    for make in (int, float, lambda t: torch.tensor(float(t)), lambda t: torch.tensor(int(t))):
        for ent in sd['state'].values():
            ent['step'] = make(4)
        other = _make('adam-plain', monkeypatch, net=_Net(seed=1))
        train_state.load_optimizer_state_dict(other, sd)
        assert other.flat.t == 4


# -- 2. import refusals ----------------------------------------------------------------------------------------------------
def test_import_refusals_name_their_reason(monkeypatch):
    step = _make('adamw-amsgrad-groups', monkeypatch)
    _fill(step, 7)

    def exported():
        return train_state.optimizer_state_dict(step)

    def refuse(sd, match, target=None):
        target = target or _make('adamw-amsgrad-groups', monkeypatch, net=_Net(seed=1))
        before = [t.clone() for t in (target.flat.m, target.flat.v)]
        with pytest.raises(ValueError, match=match):
            train_state.load_optimizer_state_dict(target, sd)
        assert all(torch.equal(a, b) for a, b in zip(before, (target.flat.m, target.flat.v)))     # nothing written

    sd = exported()
    sd['state'][2]['step'] = torch.tensor(8.0)
    refuse(sd, r"one step counter: 'a' is at step 7, 'b' at step 8")
    refuse(exported(), 'family adamw, this step runs adam', target=_make('adam-plain', monkeypatch))
    sd = exported()
    sd['param_groups'][1]['betas'] = (0.8, 0.98)
    refuse(sd, r'group 1: betas is \(0.8, 0.98\) in the dict, this step has \(0.8, 0.99\)')
    sd = exported()
    sd['state'][2]['exp_avg_sq'] = torch.zeros(4, 2)
    refuse(sd, r"'b': exp_avg_sq has shape \(4, 2\) in the dict, the parameter \(2, 4\)")
    sd = exported()
    del sd['state'][1]
    refuse(sd, r"state for 'a' and none for 'c'")


# -- 3. load refusals --------------------------------------------------------------------------------------------------------
def test_load_refusals_name_the_first_difference(monkeypatch):
    step = _make('adamw-amsgrad-groups', monkeypatch)
    _fill(step, 7)
    sd = step.state_dict()

    def target(shapes):
        monkeypatch.setattr(_lib, '_LIB', _Stub())
        net = _Net(shapes)
        ps = dict(net.named_parameters())
        first, second = [ps[k] for k in list(ps) if k != list(ps)[1]], [ps[list(ps)[1]]]
        return _Step(net, optim_spec=optim.spec('adamw', [
            dict(params=first, lr=1e-3, amsgrad=True), dict(params=second, lr=1e-4, betas=(0.8, 0.99), amsgrad=True)]))

    with pytest.raises(ValueError, match=r"saved parameter 'b' where this step has 'renamed'"):
        target((('a', (5,)), ('renamed', (2, 4)), ('c', (3,)))).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"parameter 'b' was saved with shape \(2, 4\), this step has \(4, 2\)"):
        target((('a', (5,)), ('b', (4, 2)), ('c', (3,)))).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"3 parameters saved, this step has 4; this step has 'd' in addition"):
        target((('a', (5,)), ('b', (2, 4)), ('c', (3,)), ('d', (2,)))).load_state_dict(sd)
    same = (('a', (5,)), ('b', (2, 4)), ('c', (3,)))
    with pytest.raises(ValueError, match='format 99'):
        target(same).load_state_dict(dict(sd, format=99))
    with pytest.raises(ValueError, match="saved by a 'lifter' step, this is a 'hrnet' step"):
        target(same).load_state_dict(dict(sd, kind='lifter'))
    with pytest.raises(ValueError, match='saved family adamw, this step runs adam'):
        _make('adam-plain', monkeypatch).load_state_dict(sd)
    # strict: a missing vmax is refused; strict=False zeroes it -- and still refuses another layout
    less = dict(sd, state={k: v for k, v in sd['state'].items() if k != 'vmax'})
    with pytest.raises(ValueError, match="no 'vmax'"):
        target(same).load_state_dict(less)
    t = target(same)
    _fill(t, 2)
    t.load_state_dict(less, strict=False)
    assert bool((t.grouped.vmax == 0).all()) and torch.equal(t.flat.m, step.flat.m) and t.flat.t == 7
    with pytest.raises(ValueError, match='shape'):
        target((('a', (5,)), ('b', (4, 2)), ('c', (3,)))).load_state_dict(less, strict=False)


def test_state_dict_is_a_snapshot_in_plain_containers_and_round_trips(monkeypatch):
    step = _make('adamw-amsgrad-groups', monkeypatch, kind='lifter')
    _fill(step, 7)
    step.set_lrs([5e-4, 5e-5])
    step._noupdate_forwards = 2
    sd = step.state_dict()

    def plain(o):
        if isinstance(o, dict):
            return all(isinstance(k, (str, int)) and plain(v) for k, v in o.items())
        if isinstance(o, list):
            return all(plain(v) for v in o)
        return o is None or isinstance(o, (str, int, float, bool, bytes)) or (torch.is_tensor(o) and not o.is_cuda)
    assert plain(sd)
    assert sd['kind'] == 'lifter' and sd['drop_seed'] == step.drop_seed and sd['_noupdate_forwards'] == 2
    assert sd['layout'] == {'numel': 20, 'params': [{'name': 'a', 'shape': [5], 'offset': 0},
                                                    {'name': 'b', 'shape': [2, 4], 'offset': 8},
                                                    {'name': 'c', 'shape': [3], 'offset': 16}]}
    assert [g['params'] for g in sd['optimizer']['groups']] == [['a', 'c'], ['b']]
    assert [g['lr'] for g in sd['optimizer']['groups']] == [5e-4, 5e-5] and sd['optimizer']['family'] == 'adamw'
    kept = {k: v.clone() for k, v in sd['state'].items() if torch.is_tensor(v)}
    step.flat.m.add_(1.0)                                              # the step goes on: the dict does not follow
    step.grouped.vmax.add_(1.0)
    step.grouped.groups_host['lr'] = 0.0
    assert all(torch.equal(sd['state'][k], v) for k, v in kept.items())
    assert [g['lr'] for g in sd['optimizer']['groups']] == [5e-4, 5e-5]
    other = _make('adamw-amsgrad-groups', monkeypatch, net=_Net(seed=1), kind='lifter')
    other.drop_seed = 5
    ptrs = [t.data_ptr() for t in (other.flat.flat, other.flat.m, other.flat.v, other.flat.step_dev,
                                   other.grouped.vmax, other.grouped.groups_dev, other.grouped.items_dev)]
    other.load_state_dict(sd)
    assert ptrs == [t.data_ptr() for t in (other.flat.flat, other.flat.m, other.flat.v, other.flat.step_dev,
                                           other.grouped.vmax, other.grouped.groups_dev, other.grouped.items_dev)]
    assert _same(other.state_dict(), sd)
    assert other.grouped._dirty and other.grouped.lrs == [float(np.float32(5e-4)), float(np.float32(5e-5))]
    other.grouped.push_lrs()
    other.set_lrs([5e-4, 5e-5])
    assert not other.grouped._dirty                                    # refill only on change


# -- 4. files that load with weights_only=True -----------------------------------------------------------------------------
CFGS = {'exp_type': 'test', 'optimizer': {'optim_type': 'adam', 'lr': 1e-3, 'weight_decay': 0.0}}


def _plain_run(seed=0):
    net = _Net(seed=seed)
    step = _Step(net, kind='lifter')
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    sche = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.5)
    return net, step, opt, sche


def test_checkpoint_files_load_with_weights_only_and_bring_the_generators_back(tmp_path):
    path = str(tmp_path / 'train.ckpt')
    net, step, opt, sche = _plain_run()
    _fill(step, 6)
    sche.step()
    sche.step()
    assert opt.param_groups[0]['lr'] == 5e-4
    step.set_lrs([g['lr'] for g in opt.param_groups])                  # as trainer.train does after sche.step()
    random.seed(3)
    np.random.seed(4)
    torch.manual_seed(5)
    np.random.randn(3)                                                  # a cached Gaussian in numpy's state
    empty = opt.state_dict()
    trainer.save_checkpoint(path, net, step, opt, sche, CFGS, 2, [0, 4], [1.5, 0.5])
    assert _same(opt.state_dict(), empty)                               # the caller's optimizer is not modified
    want = (random.random(), np.random.randn(3), np.random.randint(0, 1 << 30), torch.rand(4))
    assert not os.path.exists(path + '.tmp') and not os.path.exists(path + '.rank0.tmp')
    main = torch.load(path, weights_only=True)
    rank = torch.load(path + '.rank0', weights_only=True)
    assert main['epochs'] == 2 and main['batch_idx'] == [0, 4] and main['loss'] == [1.5, 0.5]
    assert sorted(main['optimizer']['state']) == [0, 1, 2] and float(main['optimizer']['state'][0]['step']) == 6.0
    assert main['fingerprint']['world_size'] == 1 and rank['drop_seed'] == step.drop_seed and rank['rank'] == 0
    assert all(torch.equal(main['model'][k], v) for k, v in net.state_dict().items())
    # a fresh run takes it over
    net2, step2, opt2, sche2 = _plain_run(seed=1)
    step2.drop_seed = 1
    ck = trainer.load_checkpoint(path, net2, step2, opt2, sche2, CFGS, total_epochs=3)
    got = (random.random(), np.random.randn(3), np.random.randint(0, 1 << 30), torch.rand(4))
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2] and torch.equal(got[3], want[3])
    assert ck['epochs'] == 2 and step2.drop_seed == step.drop_seed and step2.flat.t == 6
    assert torch.equal(step2.flat.m, step.flat.m) and torch.equal(step2.flat.flat, step.flat.flat)
    assert all(p.data_ptr() == step2.flat.cut(step2.flat.flat, i).data_ptr() for i, p in enumerate(net2.parameters()))
    assert sche2.last_epoch == 2 and opt2.param_groups[0]['lr'] == 5e-4 and step2.lr == 5e-4
    sche.step()
    sche2.step()
    assert opt2.param_groups[0]['lr'] == opt.param_groups[0]['lr']
    # the refusals
    with pytest.raises(ValueError, match='completed 2 epochs, total_epochs is 2'):
        trainer.load_checkpoint(path, *_plain_run(seed=1), CFGS, total_epochs=2)
    with pytest.raises(ValueError, match="optimizer.optim_type 'adam', this run 'sgd'"):
        trainer.load_checkpoint(path, *_plain_run(seed=1), dict(CFGS, optimizer={'optim_type': 'sgd'}))
    with pytest.raises(ValueError, match="exp_type 'test', this run 'other'"):
        trainer.load_checkpoint(path, *_plain_run(seed=1), dict(CFGS, exp_type='other'))
    os.remove(path + '.rank0')
    with pytest.raises(ValueError, match=r'per-rank file .*\.rank0 is missing'):
        trainer.load_checkpoint(path, *_plain_run(seed=1), CFGS)


# -- 5. two gloo ranks -------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, path, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    out = {}
    torch.manual_seed(10 + rank)
    net, step, opt, sche = _plain_run()
    step.drop_seed = 100 + rank
    _fill(step, 4)
    trainer.save_checkpoint(path, net, step, opt, sche, CFGS, 1)
    # past the barrier: rank 0's file is complete whichever rank looks, and this rank's own is there
    out['after_barrier'] = os.path.isfile(path) and os.path.isfile('%s.rank%d' % (path, rank)) \
        and not os.path.exists(path + '.tmp')
    draw = torch.rand(2)
    net2, step2, opt2, sche2 = _plain_run(seed=1)
    trainer.load_checkpoint(path, net2, step2, opt2, sche2, CFGS, total_epochs=2)
    out['own_seed'] = step2.drop_seed
    out['own_draw'] = bool(torch.equal(torch.rand(2), draw))
    dist.barrier()                                       # (the test's own: both have read before one file goes)
    if rank == 1:
        os.remove('%s.rank1' % path)
    try:
        trainer.load_checkpoint(path, *_plain_run(seed=1), CFGS, total_epochs=2)
        out['missing'] = 'loaded'
    except ValueError as e:
        out['missing'] = str(e)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_per_rank_files_barrier_and_refusals(tmp_path):
    path = str(tmp_path / 'train.ckpt')
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, path, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(os.listdir(str(tmp_path))) == ['train.ckpt', 'train.ckpt.rank0']       # rank 1 removed its own
    for r in (0, 1):
        assert res[r]['after_barrier'] and res[r]['own_draw'] and res[r]['own_seed'] == 100 + r, res[r]
    assert res[0]['missing'] == 'loaded' and 'train.ckpt.rank1 is missing' in res[1]['missing']
    assert torch.load(path, weights_only=True)['fingerprint']['world_size'] == 2
    with pytest.raises(ValueError, match='written by 2 ranks, this run has 1'):
        trainer.load_checkpoint(path, *_plain_run(seed=1), CFGS)


# -- 6. tool switches and defaults ---------------------------------------------------------------------------------------------
def test_tool_switches_become_the_three_keys_and_absent_ones_change_nothing():
    ap = argparse.ArgumentParser()
    trainer.add_checkpoint_arguments(ap)
    assert trainer.checkpoint_keys_from_args(ap.parse_args([])) == {}
    assert trainer.checkpoint_keys_from_args(ap.parse_args(['--checkpoint', 'F', '--resume', 'G'])) == \
        {'checkpoint': 'F', 'checkpoint_every': 1, 'resume': 'G'}
    for off in (None, False, '', 'False', 'None'):                     # the reference's YAML says ``resume: False``
        assert trainer._path_or_none(off) is None
    assert trainer._path_or_none('a/b.ckpt') == 'a/b.ckpt'

    from tools import train_IGRs, train_lifting
    base = dict(tiny=True, lr=1e-3, epochs=1, batch_frames=2, workers=0, report_every=1, eval_every=0)
    plain = train_IGRs.igr_cfgs(argparse.Namespace(**base))
    assert not {'checkpoint', 'checkpoint_every', 'resume'} & set(plain['training_settings'])
    with_keys = train_IGRs.igr_cfgs(argparse.Namespace(checkpoint='F', resume='G', **base))
    ts = with_keys['training_settings']
    assert (ts['checkpoint'], ts['checkpoint_every'], ts['resume']) == ('F', 1, 'G')
    assert {k: v for k, v in ts.items() if k not in ('checkpoint', 'checkpoint_every', 'resume')} == \
        plain['training_settings']
    base = dict(metrics=None, out_rep='R3d', eval_every=0, neurons=64, blocks=1, dropout=0.5, lr=1e-3, epochs=4,
                batch_size=32, report_every=10, eval_start_epoch=0, aug_times=1)
    plain = train_lifting.lifting_cfgs(argparse.Namespace(**base))
    assert not {'checkpoint', 'checkpoint_every', 'resume'} & set(plain['training_settings'])
    ts = train_lifting.lifting_cfgs(argparse.Namespace(resume='G', checkpoint=None, **base))['training_settings']
    assert ts['resume'] == 'G' and 'checkpoint' not in ts
