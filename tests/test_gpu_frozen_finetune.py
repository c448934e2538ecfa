"""Fine-tuning with frozen layers on the native tape (egonet_amd.frozen_bn, train_hrnet, autograd) on MI355X:
the two new kernels alone, torch's eval-mode BatchNorm semantics inside a model in train mode, gradients against torch
autograd in float64, the pruned backward against the unpruned one bit for bit, the step's loss, and graph capture.

Bounds: the kernels' outputs are one fp32 multiply (bit-equal to numpy) and a double-precision formula rounded once
(one fp32 ulp); the model-level bounds are those of tests/test_gpu_train_hrnet.py (maps atol 2e-4; gradient error
relative to each tensor's largest entry max < 5e-2 and median < 2e-3 -- one ReLU tie resolved the other way moves the
tensors below it by ~1e-2; loss 2e-5 relative)."""
import copy

import numpy as np
import pytest
import torch

import frozen_walk as W
from egonet_amd import _lib, configs, frozen_bn, synth
from egonet_amd.model.heatmapModel import hrnet as hip_hrnet
from egonet_amd.train_hrnet import HRNetTrainStep

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_autotune(monkeypatch):
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')      # cost-model tile choice: keeps the tests short


def _tiny_model(cfg, seed=9):
    net = hip_hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=seed))
    return net.cuda().train()


# ---------------------------------------------------------------------------------------------------------------------
# 1. egn_bn_frozen_bwd_f32 alone
@pytest.mark.parametrize('rows,cols,ld', [(1, 5, 16), (32, 33, 48), (32, 48, 48), (4099, 66, 80), (2 * 64 * 64, 256, 256)])
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('with_dres', [False, True])
def test_frozen_bwd_kernel_is_bit_equal_to_numpy(rows, cols, ld, relu, with_dres):
    L = _lib.lib()
    rng = np.random.RandomState(rows + 7 * cols + relu)
    dy = rng.standard_normal((rows, ld)).astype(np.float32)          # padding columns hold numbers too
    y = rng.standard_normal((rows, ld)).astype(np.float32)
    pick = rng.randint(0, 4, size=y.shape)
    y[pick == 0] = 0.0                                               # exact zeros and negative zeros: gate closed
    y[pick == 1] = -0.0
    scale = np.zeros((cols + 15) // 16 * 16, np.float32)
    scale[:cols] = rng.standard_normal(cols).astype(np.float32)
    dpre = np.where(y > 0, dy, np.float32(0)) if relu else dy.copy()
    dpre[:, cols:] = 0
    want_dz = np.zeros_like(dy)
    want_dz[:, :cols] = dpre[:, :cols] * scale[:cols]                # one fp32 multiply
    t = {k: torch.from_numpy(v).cuda() for k, v in dict(dy=dy, y=y, scale=scale).items()}
    dz = torch.full((rows, ld), float('nan'), device='cuda')
    dres = torch.full((rows, ld), float('nan'), device='cuda') if with_dres else None
    rc = L.egn_bn_frozen_bwd_f32(_lib.ptr(t['dy']), _lib.ptr(t['y']), _lib.ptr(t['scale']), relu, _lib.ptr(dz),
                                 _lib.ptr(dres), rows, cols, ld, _lib.current_stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(dz.cpu().numpy().view(np.uint32), want_dz.view(np.uint32))
    if with_dres:
        assert np.array_equal(dres.cpu().numpy().view(np.uint32), dpre.view(np.uint32))
    assert not dz[:, cols:].any()


def test_frozen_bwd_kernel_refuses_bad_arguments():
    L = _lib.lib()
    a = torch.zeros(64, device='cuda')
    st = _lib.current_stream()
    assert L.egn_bn_frozen_bwd_f32(_lib.ptr(a), None, _lib.ptr(a), 1, _lib.ptr(a), None, 1, 5, 16, st) == -1     # relu, no y
    assert L.egn_bn_frozen_bwd_f32(_lib.ptr(a), _lib.ptr(a), _lib.ptr(a), 2, _lib.ptr(a), None, 1, 5, 16, st) == -1
    assert L.egn_bn_frozen_bwd_f32(_lib.ptr(a), _lib.ptr(a), _lib.ptr(a), 1, _lib.ptr(a), None, 1, 5, 6, st) == -1   # ld % 4
    assert L.egn_bn_frozen_bwd_f32(_lib.ptr(a), _lib.ptr(a), _lib.ptr(a), 1, _lib.ptr(a), None, 1, 20, 16, st) == -1  # ld < cols
    assert L.egn_bn_frozen_bwd_f32(_lib.ptr(a), None, _lib.ptr(a), 0, _lib.ptr(a), None, 1, 5, 16, st) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. egn_bn_fold_batch_f32 alone
def test_fold_kernel_within_one_ulp_of_float64():
    L = _lib.lib()
    dt = np.dtype(frozen_bn.FoldTable._DESC, align=True)
    assert dt.itemsize == L.egn_bn_fold_desc_bytes()
    rng = np.random.RandomState(5)
    eps = 1e-5
    layers, rows = [], []
    for cout, has_bias in ((5, True), (48, False), (66, True)):
        coutp = (cout + 15) // 16 * 16
        h = dict(gamma=rng.uniform(-2, 2, cout), beta=rng.standard_normal(cout), mean=rng.standard_normal(cout) * 3,
                 var=rng.uniform(1e-4, 9, cout), bias=rng.standard_normal(cout))
        d = {k: torch.from_numpy(v.astype(np.float32)).cuda() for k, v in h.items()}
        d['scale'] = torch.full((coutp,), float('nan'), device='cuda')
        d['shift'] = torch.full((coutp,), float('nan'), device='cuda')
        layers.append((cout, has_bias, d))
        rows.append((d['gamma'].data_ptr(), d['beta'].data_ptr(), d['mean'].data_ptr(), d['var'].data_ptr(),
                     d['bias'].data_ptr() if has_bias else 0, d['scale'].data_ptr(), d['shift'].data_ptr(), eps, cout,
                     coutp))
    desc = np.zeros(len(rows), dtype=dt)
    for i, r in enumerate(rows):
        desc[i] = r
    table = torch.from_numpy(desc.view(np.uint8)).cuda()

    def run_and_check():
        assert L.egn_bn_fold_batch_f32(_lib.ptr(table), len(rows), _lib.current_stream()) == 0
        torch.cuda.synchronize()
        for cout, has_bias, d in layers:
            g, b, m, v, cb = (d[k].cpu().numpy().astype(np.float64) for k in ('gamma', 'beta', 'mean', 'var', 'bias'))
            sc = g / np.sqrt(v + eps)
            sh = b + ((cb if has_bias else 0.0) - m) * sc
            for got, want in ((d['scale'].cpu().numpy(), sc), (d['shift'].cpu().numpy(), sh)):
                ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
                assert np.all(np.abs(got[:cout].astype(np.float64) - want) <= ulp), np.abs(got[:cout] - want).max()
                assert got[cout:].size == (-cout) % 16 and not got[cout:].any()      # padding: zeros, not the NaN fill
    run_and_check()
    before = layers[1][2]['scale'].clone()
    layers[1][2]['gamma'].mul_(-1.75)                    # in place: the table's pointers still hold
    run_and_check()
    assert not torch.equal(before, layers[1][2]['scale'])
    assert L.egn_bn_fold_batch_f32(None, 3, _lib.current_stream()) == -1
    assert L.egn_bn_fold_batch_f32(_lib.ptr(table), 0, _lib.current_stream()) == -1


def test_fold_kernel_gamma_null_gives_inverse_sigma_and_skips_shift():
    L = _lib.lib()
    var = torch.rand(20, device='cuda') + 0.1
    mean = torch.randn(20, device='cuda')
    scale = torch.full((32,), float('nan'), device='cuda')
    desc = np.zeros(1, dtype=np.dtype(frozen_bn.FoldTable._DESC, align=True))
    desc[0] = (0, 0, mean.data_ptr(), var.data_ptr(), 0, scale.data_ptr(), 0, 1e-5, 20, 32)
    table = torch.from_numpy(desc.view(np.uint8)).cuda()
    assert L.egn_bn_fold_batch_f32(_lib.ptr(table), 1, _lib.current_stream()) == 0
    want = 1.0 / np.sqrt(var.cpu().numpy().astype(np.float64) + 1e-5)
    got = scale.cpu().numpy()
    assert np.all(np.abs(got[:20] - want) <= np.spacing(want.astype(np.float32))) and not got[20:].any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. semantics: eval-mode layers keep their statistics and counters
def _bn_state(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()
            if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}


def _check_eval_layers_untouched(net, before):
    after = _bn_state(net)
    frozen = [k for k in before if k.startswith(('layer1.', 'bn1.'))]
    assert len(frozen) >= 3 * 13
    for k in frozen:
        assert torch.equal(after[k], before[k]), k
    for name in ('bn2', 'stage2.0.branches.0.0.bn1', 'head2.0.bn1'):        # train-mode layers still track
        assert not torch.equal(after[name + '.running_mean'], before[name + '.running_mean']), name
        assert not torch.equal(after[name + '.running_var'], before[name + '.running_var']), name
        assert int(after[name + '.num_batches_tracked']) == int(before[name + '.num_batches_tracked']) + 1, name


def _inputs(n=2, seed=4):
    gen = torch.Generator().manual_seed(3)
    x = synth.synth_crops(n, 3, 64, 64, seed=seed).cuda()
    return x, torch.rand(n, 5, 16, 16, generator=gen).cuda(), torch.rand(n, 5, 2, generator=gen) * 64


@pytest.mark.parametrize('affine_trains', [False, True], ids=['fused', 'affine'])
def test_eval_mode_batchnorm_keeps_statistics_in_the_native_step(affine_trains):
    net = _tiny_model(configs.tiny_config('coordinates'))
    W.freeze(net, W.STEM_FREEZE, bn_eval=True, affine_trains=affine_trains)
    assert not net.layer1[0].bn1.training and not net.bn1.training and net.bn2.training and net.training
    before = _bn_state(net)
    x, tg, jt = _inputs()
    tr = HRNetTrainStep(net, lr=1e-3)
    loss = tr.step(x, tg, jt)
    assert np.isfinite(float(loss.item()))
    _check_eval_layers_untouched(net, before)


def test_eval_mode_batchnorm_keeps_statistics_under_the_bridge():
    net = _tiny_model(configs.tiny_config('coordinates'))
    net.layer1.eval()
    net.bn1.eval()                               # torch's own interface: parameters stay trainable (the affine form)
    before = _bn_state(net)
    x, _, _ = _inputs()
    L = _lib.lib()
    c0 = L.egn_direct_conv_count()
    maps, coords = net(x)
    (maps.sum() + coords.sum()).backward()
    assert L.egn_direct_conv_count() > c0        # the native tape ran, not the torch graph
    torch.cuda.synchronize()
    _check_eval_layers_untouched(net, before)
    assert net.layer1[0].bn1.weight.grad is not None and float(net.layer1[0].bn1.weight.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. gradients against torch autograd in float64
def _rel_err(got, want):
    return float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-12)


def _bridge_vs_float64(net, x, seed=11):
    """Outputs and parameter gradients of the bridge against the same modules (same modes) on the CPU in float64;
    loss = sum of outputs x a fixed random tensor."""
    ref = copy.deepcopy(net).cpu().double()
    assert [m.training for m in ref.modules()] == [m.training for m in net.modules()]
    L = _lib.lib()
    c0 = L.egn_direct_conv_count()
    outs = net(x)
    outs = outs if isinstance(outs, tuple) else (outs,)
    gen = torch.Generator().manual_seed(seed)
    rnd = [torch.randn(o.shape, generator=gen, dtype=torch.float64) for o in outs]
    sum((o * r.float().cuda()).sum() for o, r in zip(outs, rnd)).backward()
    assert L.egn_direct_conv_count() > c0
    routs = ref(x.cpu().double())
    routs = routs if isinstance(routs, tuple) else (routs,)
    sum((o * r).sum() for o, r in zip(routs, rnd)).backward()
    for o, r in zip(outs, routs):
        np.testing.assert_allclose(o.detach().cpu().numpy(), r.detach().numpy(), rtol=0, atol=2e-4)
    named, rnamed = dict(net.named_parameters()), dict(ref.named_parameters())
    # A bias in front of a train-mode BatchNorm has the gradient ZERO identically (the batch mean removes a constant):
    # the float64 reference holds ~1e-16 of the other gradients there and "relative to the tensor's largest entry" has
    # no meaning.  Ours is a cancelling fp32 column sum of <= 512 rows of dz: rounding leaves at most rows * 2^-24 =
    # 3e-5 of one term, and a term (an entry of dz) is taken to be no larger than ``top``, the largest entry of any
    # parameter gradient -- so such tensors are bounded by 1e-4 * top instead.
    top = max(float(q.grad.abs().max()) for q in rnamed.values() if q.grad is not None)
    errs, zeros = {}, {}
    for k, p in named.items():
        if not p.requires_grad:
            assert p.grad is None and rnamed[k].grad is None, k
            continue
        assert p.grad is not None, k
        want = rnamed[k].grad.numpy()
        if float(np.abs(want).max()) < 1e-9 * top:
            zeros[k] = float(p.grad.abs().max()) / top
        else:
            errs[k] = _rel_err(p.grad.cpu().numpy().astype(np.float64), want)
    assert errs
    vals = list(errs.values())
    print('gradient errors: max %.3g median %.3g over %d tensors; identically-zero gradients: %s'
          % (max(vals), np.median(vals), len(vals), {k: '%.2g' % v for k, v in zeros.items()}))
    assert max(vals) < 5e-2 and np.median(vals) < 2e-3, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    assert all(v < 1e-4 for v in zeros.values()), zeros


def _case_model(case):
    if case == 'shuffle':
        cfg = configs.clone(configs.tiny_config('heatmap'))
        cfg['heatmapModel']['pixel_shuffle'] = True
        cfg['heatmapModel']['heatmap_size'] = [32, 32]
        return _tiny_model(cfg)
    return _tiny_model(configs.tiny_config('coordinates'))


def _apply_case(net, case):
    if case == 'fused':                  # (a) statistics and affine frozen
        W.freeze(net, W.STEM_FREEZE, bn_eval=True)
    elif case == 'affine':               # (b) statistics frozen, gamma / beta trainable
        W.freeze(net, W.STEM_FREEZE, bn_eval=True, affine_trains=True)
    elif case == 'shuffle':              # (c) the biased 1x1 conv's BatchNorm of the pixel-shuffle head in eval mode
        bn = net.upsample_layer[1].eval()
        bn.weight.requires_grad = bn.bias.requires_grad = False


@pytest.mark.parametrize('case', ['fused', 'affine', 'shuffle'])
@pytest.mark.parametrize('frozen', [False, True], ids=['all_train', 'frozen'])
def test_bridge_gradients_vs_torch_float64(case, frozen):
    """``all_train``: the same model and seeds with every layer in train mode pass the same comparison, so a failure of
    ``frozen`` is the feature's and not a ReLU tie of the seed."""
    net = _case_model(case)
    if frozen:
        _apply_case(net, case)
    _bridge_vs_float64(net, synth.synth_crops(2, 3, 64, 64, seed=4).cuda())


@pytest.mark.parametrize('wino', ['1', '43'])
@pytest.mark.parametrize('frozen', [False, True], ids=['all_train', 'frozen'])
def test_fused_epilogue_with_residual_on_both_winograd_families(wino, frozen, monkeypatch):
    """(d) 48-channel blocks: the 3x3 convs with residual of stages 2 and 3, their BatchNorm in eval mode with gamma /
    beta frozen and the filters trainable -- forward epilogue (scale, shift, residual, ReLU), frozen backward, weight and
    data gradients on F(2x2,3x3) and F(4x4,3x3).  Weights seed 21 and 4 crops of seed 30 (those of
    test_first_step_gradients_vs_reference): of seven (weights, crops, count) combinations measured on an MI355X the
    all-train model passed on both families with these (max 0.034, one ReLU tie; median 1e-5); with a tie high in the
    net the median itself reaches 2e-3 .. 1.7e-2 (e.g. weights 9 / crops 4 / 2 crops: 9.4e-3)."""
    monkeypatch.setenv('EGONET_AMD_WINO', wino)
    net = _tiny_model(configs.hrnet_config(48, (64, 64), 5, 'heatmap', modules=(1, 1, 1), num_blocks=1), seed=21)
    if frozen:
        for name, m in net.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d) and name.startswith(('stage2', 'stage3')):
                m.eval()
                m.weight.requires_grad = m.bias.requires_grad = False
    _bridge_vs_float64(net, synth.synth_crops(4, 3, 64, 64, seed=30).cuda())


# ---------------------------------------------------------------------------------------------------------------------
# 5. pruning is exact
def _pruned_and_unpruned(prefixes, monkeypatch):
    """One step with pruning and one without from identical state -> {'1': ..., '0': ...}."""
    L = _lib.lib()
    x, tg, jt = _inputs()
    runs = {}
    for prune in ('1', '0'):
        monkeypatch.setenv('EGONET_AMD_PRUNE_BACKWARD', prune)
        net = W.freeze(_tiny_model(configs.tiny_config('coordinates')), prefixes)
        tr = HRNetTrainStep(net, lr=1e-3)
        assert tr.prune_backward == (prune == '1')
        c0 = L.egn_direct_conv_count()
        loss = tr.step(x, tg, jt)
        torch.cuda.synchronize()
        runs[prune] = dict(net=net, loss=loss.clone(), convs=L.egn_direct_conv_count() - c0,
                           counts=tr.last_backward_launches,
                           grads={k: p.grad.clone() for k, p in net.named_parameters() if p.requires_grad})
    return runs


@pytest.mark.parametrize('prefixes', [W.STEM_FREEZE, W.PED_FREEZE], ids=['stem', 'pedestrian'])
def test_pruned_backward_is_bit_identical_to_the_unpruned_one(prefixes, monkeypatch):
    runs = _pruned_and_unpruned(prefixes, monkeypatch)
    on, off = runs['1'], runs['0']
    assert on['grads'] and list(on['grads']) == list(off['grads'])
    for k in on['grads']:
        assert torch.equal(on['grads'][k], off['grads'][k]), k
    for (k, a), (_, b) in zip(on['net'].state_dict().items(), off['net'].state_dict().items()):
        assert torch.equal(a, b), k
    want = W.expected_launches(on['net'])
    print('backward launches: pruned %s, unpruned %s' % (on['counts'], off['counts']))
    assert on['counts'] == want
    assert on['counts'] == frozen_bn.planned_backward_launches(on['net'], 64, 64, prune=True)
    assert off['counts'] == frozen_bn.planned_backward_launches(off['net'], 64, 64, prune=False)
    assert off['counts']['wgrad'] == on['counts']['wgrad']
    pruned_dgrads = off['counts']['dgrad'] - on['counts']['dgrad']
    assert pruned_dgrads > 0 and off['counts']['bn_bwd'] > on['counts']['bn_bwd']
    assert off['convs'] - on['convs'] == pruned_dgrads


@pytest.mark.parametrize('prefixes', [W.STEM_FREEZE, W.PED_FREEZE], ids=['stem', 'pedestrian'])
def test_pruned_step_loss_is_bit_identical_to_the_unpruned_one(prefixes, monkeypatch):
    """The loss scalar of the two steps, ``torch.equal`` as the feature's specification asks.

    KNOWN TO FAIL, run to run: the loss is computed in the forward, which pruning does not touch, but the loss kernels
    add per-wavefront partial sums into one float64 word with atomics (csrc/train_ops.hip, elem_loss_kernel), so the
    last bit depends on the order the waves arrive in.  Measured on an MI355X: four IDENTICAL pruned steps of the
    stem-frozen model gave 1.3648372148919672, 1.3648372148919672, 1.364837214891967, 1.364837214891967; the pruned /
    unpruned pair gave (…672, …67) for the stem freeze and (…67, …672) for the Pedestrian list in one run.  Every
    gradient and every updated parameter of the same steps is bit-equal (the test above).  tests/test_gpu_train_hrnet.py
    compares such losses with rtol=1e-12 for the same reason; the bound here is left as specified."""
    runs = _pruned_and_unpruned(prefixes, monkeypatch)
    on, off = runs['1'], runs['0']
    print('losses: pruned %r, unpruned %r' % (float(on['loss']), float(off['loss'])))
    assert torch.equal(on['loss'], off['loss']), (float(on['loss']), float(off['loss']))


def test_all_trainable_model_counts_every_layer():
    net = _tiny_model(configs.tiny_config('coordinates'))
    tr = HRNetTrainStep(net, lr=1e-3)
    tr.step(*_inputs())
    convs = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert tr.last_backward_launches == {'dgrad': len(convs) - 1, 'wgrad': len(convs), 'bn_bwd': 2 * len(bns)}
    assert not tr.folds.entries                      # nothing to fold: no launch was added to this model's step


# ---------------------------------------------------------------------------------------------------------------------
# 6. the frozen-BN step's loss against the bridge + the same loss written in torch
def test_frozen_bn_step_loss_equals_bridge_loss():
    x, tg, jt = _inputs()
    net = W.freeze(_tiny_model(configs.tiny_config('coordinates')), W.STEM_FREEZE, bn_eval=True)
    loss = float(HRNetTrainStep(net, lr=1e-3).step(x, tg, jt, update=False).item())
    net2 = W.freeze(_tiny_model(configs.tiny_config('coordinates')), W.STEM_FREEZE, bn_eval=True)
    maps, coords = net2(x)
    gt = (jt / 64.0).cuda()
    ref = 0.5 * torch.nn.functional.mse_loss(maps, tg) + 0.1 * torch.nn.functional.l1_loss(coords, gt)
    print('step loss %.9g, bridge + torch loss %.9g' % (loss, float(ref.detach())))
    ref = float(ref.detach())
    assert abs(loss - ref) < 2e-5 * abs(ref)


# ---------------------------------------------------------------------------------------------------------------------
# 7. graph capture
def test_graphed_frozen_bn_step_equals_eager_steps():
    from egonet_amd.graph import GraphedStep
    gen = torch.Generator().manual_seed(2)
    xs = [synth.synth_crops(2, 3, 64, 64, seed=40 + i).cuda() for i in range(4)]
    tg = torch.rand(4, 2, 5, 16, 16, generator=gen).cuda()
    jt = (torch.rand(4, 2, 5, 2, generator=gen) * 64).cuda()
    out = []
    for graphed in (False, True):
        net = W.freeze(_tiny_model(configs.tiny_config('coordinates')), W.STEM_FREEZE, bn_eval=True)
        tr = HRNetTrainStep(net, lr=1e-3)
        if graphed:
            before = {k: v.clone() for k, v in net.state_dict().items()}
            g = GraphedStep(tr, xs[0], tg[0], jt[0], warmup=1)       # the warm-up iteration is undone
            for k, v in net.state_dict().items():
                assert torch.equal(v, before[k]), k
            losses = [float(g(xs[i], tg[i], jt[i]).item()) for i in range(1, 4)]
        else:
            losses = [float(tr.step(xs[i], tg[i], jt[i]).item()) for i in range(1, 4)]
        out.append((net, losses, tr.flat.t))
    assert out[0][2] == out[1][2] == 3
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=1e-12)       # the loss sum uses atomics: order varies
    for (k, a), (_, b) in zip(out[0][0].state_dict().items(), out[1][0].state_dict().items()):
        assert torch.equal(a, b), k
