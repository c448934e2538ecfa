"""Save / resume of the native training steps on the device (egonet_amd/train_state.py, the checkpoints of
egonet_amd/trainer.py): a third step after a round trip through ``state_dict`` has the bits of the uninterrupted one;
the dict is a snapshot and loading keeps every address; the step launches what it launched before; a captured graph
goes on over loaded state; a torch optimizer's state continues natively within the float64 bounds of
tests/optim_groups_ref.py; ``trainer.train`` resumed lands where the uninterrupted run does; the tool's switches."""
import copy
import logging
import os
import random

import numpy as np
import pytest
import torch

import optim_groups_ref as R
from egonet_amd import _lib, configs, optim, synth, train_state, trainer
from egonet_amd.graph import GraphedStep
from egonet_amd.model import FCmodel
from egonet_amd.model.heatmapModel import hrnet
from egonet_amd.train_hrnet import HRNetTrainStep
from egonet_amd.train_lifter import LifterTrainStep

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_autotune(monkeypatch):
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')


# -- the shapes of the optimizer-group tests --------------------------------------------------------------------------------
def _hrnet(seed=9):
    cfg = configs.tiny_config('coordinates')
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=seed))
    return net.cuda()


@pytest.fixture(scope='module')
def hrnet_batches():
    gen = torch.Generator().manual_seed(2)
    xs = [synth.synth_crops(2, 3, 64, 64, seed=40 + i).cuda() for i in range(3)]
    tg = torch.rand(3, 2, 5, 16, 16, generator=gen).cuda()
    jt = (torch.rand(3, 2, 5, 2, generator=gen) * 64).cuda()
    return [(xs[i], tg[i], jt[i]) for i in range(3)]


def _lifter(seed=3, dropout=0.0):
    torch.manual_seed(seed)
    cfg = configs.clone(configs.tiny_config())
    cfg['FCModel']['dropout'] = dropout
    return FCmodel.get_fc_model(1, cfg, 10, 12).cuda()


@pytest.fixture(scope='module')
def lifter_batches():
    gen = torch.Generator().manual_seed(5)
    return [(torch.randn(32, 10, generator=gen).cuda(), torch.randn(32, 12, generator=gen).cuda()) for _ in range(3)]


def _grouped_hrnet_step(net):
    groups = optim.no_decay_groups(net, 1e-2)
    groups[1]['lr'] = 1e-4
    return HRNetTrainStep(net, optim_spec=optim.spec('adamw', groups, lr=1e-3, amsgrad=True), max_grad_norm=0.05)


def _grouped_lifter_step(net):
    return LifterTrainStep(net, optim_spec=optim.spec('adamw', optim.no_decay_groups(net, 1e-2), lr=1e-3, amsgrad=True),
                           max_grad_norm=1e-3)


MAKERS = {
    'hrnet-adam-plain': (_hrnet, lambda net: HRNetTrainStep(net)),
    'hrnet-sgd-momentum-plain': (_hrnet, lambda net: HRNetTrainStep(net, lr=1e-2, optim_type='sgd', momentum=0.9)),
    'hrnet-adamw-groups-amsgrad-clip': (_hrnet, _grouped_hrnet_step),
    'lifter-dropout-in-kernel': (lambda seed=3: _lifter(seed, dropout=0.5), lambda net: LifterTrainStep(net)),
    'lifter-adamw-groups-amsgrad-clip': (_lifter, _grouped_lifter_step),
}


def _device_state(step):
    """Everything a step mutates, as int32 views on the CPU."""
    torch.cuda.synchronize()
    out = {'flat': step.flat.flat, 'm': step.flat.m, 'v': step.flat.v, 'step': step.flat.step_dev}
    if step.grouped is not None:
        out.update({k: t for k, t in (('vmax', step.grouped.vmax), ('clip', step.grouped.clip)) if t is not None})
    for name, b in step.model.named_buffers():
        out['buffer ' + name] = b
    return {k: (t if t.dtype == torch.int64 else t.view(torch.int32)).detach().cpu().clone() for k, t in out.items()}


def _assert_same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _model_state(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}      # (state_dict() itself aliases the flat buffer)


# -- 7. round trip, bit-equal -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(MAKERS))
def test_third_step_after_a_round_trip_has_the_bits_of_the_uninterrupted_one(name, hrnet_batches, lifter_batches):
    make_net, make_step = MAKERS[name]
    batches = hrnet_batches if name.startswith('hrnet') else lifter_batches
    net = make_net()
    step = make_step(net)
    assert (step.grouped is not None) == ('groups' in name)
    step.step(*batches[0])
    step.step(*batches[1])
    sd, msd = step.state_dict(), _model_state(net)
    step.step(*batches[2])
    a = _device_state(step)
    assert int(a['step']) == 3 and sd['state']['step'] == 2

    torch.manual_seed(99)                                              # another dropout seed, other weights
    net_b = make_net(seed=4)
    step_b = make_step(net_b)
    if name.startswith('lifter'):
        assert step_b.drop_seed != step.drop_seed and step_b.p == step.p
        assert step.p == (0.5 if 'dropout' in name else 0.0)
    else:
        step_b.apply_cr_loss = not step.apply_cr_loss
    net_b.load_state_dict(msd)
    step_b.load_state_dict(sd)
    if name.startswith('lifter'):
        assert step_b.drop_seed == step.drop_seed
    else:
        assert step_b.apply_cr_loss == step.apply_cr_loss
    step_b.step(*batches[2])
    _assert_same_state(a, _device_state(step_b))


# -- 8. snapshot and in place ---------------------------------------------------------------------------------------------------
def test_state_dict_is_a_snapshot_and_loading_keeps_every_address(lifter_batches):
    net = _lifter()
    step = _grouped_lifter_step(net)
    step.step(*lifter_batches[0])
    step.set_lrs([5e-4, 5e-5])
    step.step(*lifter_batches[1])
    sd = step.state_dict()
    assert all(not t.is_cuda for t in sd['state'].values() if torch.is_tensor(t))
    kept = copy.deepcopy(sd)
    msd = _model_state(net)
    g = step.grouped
    tensors = lambda: [step.flat.flat, step.flat.grad, step.flat.m, step.flat.v, step.flat.step_dev, step.flat.lr_dev,
                       g.vmax, g.clip, g.groups_dev, g.items_dev] + list(net.parameters()) + list(net.buffers())
    ptrs = [t.data_ptr() for t in tensors()]
    tables = (g.groups_host.ctypes.data, g.items_host.ctypes.data)
    step.set_lrs([1e-4, 1e-5])
    step.step(*lifter_batches[2])                                      # the step goes on: the dict does not follow
    torch.cuda.synchronize()

    def same(x, y):
        if torch.is_tensor(x):
            return torch.equal(x, y)
        if isinstance(x, dict):
            return list(x) == list(y) and all(same(x[k], y[k]) for k in x)
        if isinstance(x, list):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        return x == y
    assert same(sd, kept)
    after = _device_state(step)
    net.load_state_dict(msd)
    step.load_state_dict(sd)
    assert ptrs == [t.data_ptr() for t in tensors()]
    assert tables == (g.groups_host.ctypes.data, g.items_host.ctypes.data)
    back = _device_state(step)
    assert int(back['step']) == 2 and not torch.equal(back['m'], after['m'])
    assert g.lrs == [R._f32(5e-4), R._f32(5e-5)] and g._dirty          # on the set_lrs / push_lrs route
    assert same(step.state_dict(), kept)


# -- 9. no cost to the step -------------------------------------------------------------------------------------------------------
def test_the_step_launches_what_it_launched_before(hrnet_batches):
    L = _lib.lib()

    def count(step, batch):
        torch.cuda.synchronize()
        n0 = L.egn_launch_count()
        step.step(*batch)
        torch.cuda.synchronize()
        return L.egn_launch_count() - n0

    net = _hrnet()
    step = _grouped_hrnet_step(net)
    step.step(*hrnet_batches[0])
    step.step(*hrnet_batches[1])
    before = count(step, hrnet_batches[2])
    n0 = L.egn_launch_count()
    sd, msd = step.state_dict(), _model_state(net)
    assert L.egn_launch_count() == n0                                  # taking the state launches nothing of the library's
    after_save = count(step, hrnet_batches[0])
    net.load_state_dict(msd)
    step.load_state_dict(sd)
    packed = step.packs.table.data_ptr()
    after_load = count(step, hrnet_batches[1])
    again = count(step, hrnet_batches[2])
    # the packed-filter cache kept its table: every filter of the iteration still goes out as one launch
    assert step.packs.table is not None and step.packs.table.data_ptr() == packed
    assert step.packs.ptrs == step.packs._pointers()

    other = _grouped_hrnet_step(_hrnet())                              # never saved, never loaded
    other.step(*hrnet_batches[0])
    other.step(*hrnet_batches[1])
    never = count(other, hrnet_batches[2])
    print('launches per step: before %d, after state_dict %d, after load_state_dict %d / %d, never used %d'
          % (before, after_save, after_load, again, never))
    assert before == after_save == after_load == again == never


# -- 10. under a graph ----------------------------------------------------------------------------------------------------------------
def test_a_graphed_step_goes_on_over_loaded_state(hrnet_batches):
    def graphed():
        net = _hrnet()
        step = _grouped_hrnet_step(net)
        return net, step, GraphedStep(step, *hrnet_batches[0], warmup=1)

    net, step, run = graphed()
    run(*hrnet_batches[1])
    run(*hrnet_batches[2])
    a = _device_state(step)
    run.close()

    net, step, run = graphed()
    run(*hrnet_batches[1])
    torch.cuda.synchronize()
    sd, msd = step.state_dict(), _model_state(net)
    run(*hrnet_batches[2])
    run(*hrnet_batches[0])                                             # further than A went
    torch.cuda.synchronize()
    net.load_state_dict(msd)
    step.load_state_dict(sd)
    run(*hrnet_batches[2])
    b = _device_state(step)
    run.close()
    assert int(a['step']) == 2
    _assert_same_state(a, b)


# -- 11. from torch to native -----------------------------------------------------------------------------------------------------------
def test_a_torch_optimizers_state_continues_natively(lifter_batches):
    net = _lifter()
    net.train()
    groups = optim.no_decay_groups(net, 1e-2, lr=1e-3)
    opt = torch.optim.AdamW(groups, amsgrad=True)
    for x, y in lifter_batches[:2]:                                    # the plain torch module, the torch graph
        opt.zero_grad()
        torch.nn.functional.mse_loss(net.w2(net.get_representation(x)), y).backward()
        opt.step()
    theirs = opt.state_dict()
    step = LifterTrainStep(net, optim_spec=optim.spec_from_torch(opt))
    assert step.grouped is not None and step.flat.t == 0
    train_state.load_optimizer_state_dict(step, theirs)
    assert step.flat.t == 2
    mine = train_state.optimizer_state_dict(step)
    assert mine['param_groups'] == theirs['param_groups']
    assert sorted(mine['state']) == sorted(theirs['state']) and len(mine['state']) == len(step.flat.params)
    for idx, ent in theirs['state'].items():
        assert list(mine['state'][idx]) == list(ent)
        for k, v in ent.items():
            got = mine['state'][idx][k]
            assert got.dtype == v.dtype and got.shape == v.shape
            assert torch.equal(got.view(torch.int32), v.cpu().view(torch.int32)), (idx, k)
    # one native step from there: iteration 2 of tests/test_gpu_optim_groups.py's _check_two_steps, its bounds
    flat, gu = step.flat, step.grouped
    owner = {id(p): k for k, g in enumerate(groups) for p in g['params']}
    params = [(p.numel(), owner[id(p)]) for p in flat.params]
    rows = [{k: g[k] for k in optim._DEFAULTS['adamw']} for g in groups]      # (torch filled its defaults into the dicts)
    assert all(r['amsgrad'] for r in rows) and [r['weight_decay'] for r in rows] == [1e-2, 0.0]
    names = {'p': flat.flat, 'm': flat.m, 'v': flat.v, 'vmax': gu.vmax}
    c = R.problem('adamw_amsgrad', 'adamw', rows, params, 2, None)
    assert R.uses(c) == ('m', 'v', 'vmax')
    x = {a: names[a].detach().cpu().clone() for a in ('p',) + R.uses(c)}
    assert float(x['vmax'].abs().max()) > 0 and float(x['m'].abs().max()) > 0
    step.step(*lifter_batches[2])
    torch.cuda.synchronize()
    x['g'] = flat.grad.detach().cpu().clone()
    assert flat.t == 3
    want = R.reference(c, x)
    A = {k: v[1] for k, v in R.emulate(c, x).items()}
    got = {a: names[a].detach().cpu() for a in ('p',) + R.uses(c)}
    for name in want:
        print('%-6s worst ratio %.2f' % (name, R.ratio(got[name], want[name], A[name])[0]))
    bad = R.check(c, got, want, A)
    assert not bad, bad


# -- 12. trainer.train resumed ------------------------------------------------------------------------------------------------------------
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


def _train(monkeypatch, seed, total_epochs, **keys):
    """Fresh model, optimizer, scheduler and loader; two groups with their own rates, a milestone at epoch 2, a
    shuffling loader (the generators' states matter)."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    cfg = configs.clone(configs.tiny_config('coordinates'))
    cfg.update(use_gpu=True, exp_type='test', cascade={'num_stages': 1},
               optimizer={'optim_type': 'adam', 'lr': 4e-3, 'weight_decay': 0.0, 'milestones': [2], 'gamma': 0.5},
               training_settings=dict({'total_epochs': total_epochs, 'batch_size': 4, 'num_threads': 0, 'shuffle': True,
                                       'report_every': 1, 'eval_during': False, 'plot_loss': False}, **keys))
    net = _hrnet()
    ps = list(net.parameters())
    half = len(ps) // 2
    opt = torch.optim.Adam([dict(params=ps[:half], lr=4e-3), dict(params=ps[half:], lr=1e-3)])
    sche = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.5)
    made = []
    real = trainer.make_step
    monkeypatch.setattr(trainer, 'make_step', lambda *a, **k: made.append(real(*a, **k)) or made[-1])
    lg = logging.getLogger('egonet_amd.test_train_state')
    lg.handlers = [logging.NullHandler()]
    try:
        record = trainer.train(_CropSet(), net, None, opt, sche, cfg, lg)
    finally:
        monkeypatch.setattr(trainer, 'make_step', real)
    step = made[-1]
    assert step.grouped is not None
    return {'state': _device_state(step), 'last_epoch': sche.last_epoch, 'lrs': [g['lr'] for g in opt.param_groups],
            'step_lrs': step.grouped.lrs, 'apply_cr_loss': step.apply_cr_loss, 'batch_idx': record['batch_idx'],
            'loss': record['loss'], 'opt_state': opt.state_dict()['state']}


def test_trainer_train_resumed_lands_where_the_uninterrupted_run_does(monkeypatch, tmp_path):
    path = str(tmp_path / 'run.ckpt')
    a = _train(monkeypatch, 7, 3)
    control = _train(monkeypatch, 7, 3)
    # the premise: within one process, two uninterrupted runs have the same bits
    _assert_same_state(a['state'], control['state'])
    assert a['batch_idx'] == control['batch_idx'] == [0, 1, 2, 3, 4, 5]
    losses_bit_equal = a['loss'] == control['loss']
    print('control run: loss history %s' % ('bit-equal' if losses_bit_equal else 'equal to rounding of the float64 sum'))
    np.testing.assert_allclose(control['loss'], a['loss'], rtol=1e-9, atol=0)

    first = _train(monkeypatch, 7, 1, checkpoint=path)
    assert os.path.isfile(path) and os.path.isfile(path + '.rank0') and first['opt_state'] == {}
    ck = torch.load(path, weights_only=True)
    assert ck['epochs'] == 1 and ck['batch_idx'] == [0, 1] and ck['step']['state']['step'] == 2
    assert len(ck['optimizer']['state']) == len(ck['step']['layout']['params'])
    b = _train(monkeypatch, 1234, 3, checkpoint=path, resume=path)     # other seeds: what counts comes from the files
    _assert_same_state(a['state'], b['state'])
    assert int(b['state']['step']) == 6
    assert b['last_epoch'] == a['last_epoch'] == 3 and b['lrs'] == a['lrs'] == [2e-3, 5e-4]
    assert b['step_lrs'] == a['step_lrs'] and b['apply_cr_loss'] == a['apply_cr_loss']
    assert b['batch_idx'] == a['batch_idx']
    if losses_bit_equal:
        assert b['loss'] == a['loss']
    else:
        np.testing.assert_allclose(b['loss'], a['loss'], rtol=1e-9, atol=0)
    assert torch.load(path, weights_only=True)['epochs'] == 3
    with pytest.raises(ValueError, match='completed 3 epochs, total_epochs is 3'):
        _train(monkeypatch, 7, 3, resume=path)


# -- 13. the tool -------------------------------------------------------------------------------------------------------------------------
def _write_tree(root):
    import pose_annot_cases as pc
    from PIL import Image
    G, _ = pc.load()
    rng = np.random.RandomState(11)
    records = pc.records_of(G, 'tiny')
    for d in ('image_2', 'label_2', 'calib'):
        os.makedirs(os.path.join(root, d))
    for f, rec in enumerate(records):
        stem = '%06d' % f
        w, h = rec['size']
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, 'image_2', stem + '.png'))
        for d, text in (('label_2', rec['labels_text']), ('calib', rec['calib_text'])):
            with open(os.path.join(root, d, stem + '.txt'), 'w') as fh:
                fh.write(text)


def test_tool_checkpoints_and_resumes(tmp_path, caplog):
    from tools import train_IGRs as tool
    root, out_dir = str(tmp_path / 'kitti'), str(tmp_path / 'out')
    first, second = str(tmp_path / 'one.ckpt'), str(tmp_path / 'two.ckpt')
    _write_tree(root)
    common = ['--kitti', root, '--out', out_dir, '--tiny', '--seed', '0', '--batch-frames', '2', '--workers', '0',
              '--report-every', '1', '--no-debug-pictures']
    out = tool.main(common + ['--epochs', '1', '--checkpoint', first])
    assert out['steps'] == 2                                           # three frames, two per batch
    ck = torch.load(first, weights_only=True)
    assert ck['epochs'] == 1 and ck['step']['state']['step'] == 2 and os.path.isfile(first + '.rank0')
    with caplog.at_level(logging.INFO):
        out = tool.main(common + ['--epochs', '2', '--resume', first, '--checkpoint', second])
    assert 'starting at epoch 2' in caplog.text and 'Epoch: [2][0/' in caplog.text
    assert 'Epoch: [1]' not in caplog.text
    assert out['steps'] == 2 and np.isfinite(out['last_loss'])         # this process ran the second epoch alone
    ck = torch.load(second, weights_only=True)
    assert ck['epochs'] == 2 and ck['step']['state']['step'] == 4      # the step count of a two-epoch run
    assert len(ck['loss']) == 4
    state = torch.load(out['out'])
    net = hrnet.get_pose_net(tool.igr_cfgs(tool.argparse.Namespace(
        tiny=True, lr=1e-3, epochs=1, batch_frames=2, workers=0, report_every=1, eval_every=0)), is_train=False)
    net.load_state_dict(state, strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in state.values() if v.is_floating_point())
    assert all(torch.equal(state[k], ck['model'][k]) for k in state)
