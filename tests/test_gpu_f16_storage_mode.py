"""activations = 'f16' end to end on the device: f16 storage between f16-operand convolutions must not move a bit.

Every returned tensor of ``forward`` and of ``EgoNet.infer_crops`` under activations = 'f16' must ``torch.equal`` the one
under activations = 'f32' -- the reader of a tensor rounds it to f16 while staging it; the producer applies the same
rounding and stores f16 instead.  No tolerance, no timing.  Models and inputs: tests/f16_mode_case.py
(W48 widths), tests/f16x_mode_case.py (W32 widths, 192 x 256); one case each for the full W48 and W32 at 2 crops."""
import numpy as np
import pytest
import torch

import f16_mode_case as case48
import f16x_mode_case as case32
from egonet_amd import _lib, configs, engine, synth
from egonet_amd.model.heatmapModel import hrnet

pytestmark = pytest.mark.gpu
# (case module, the precisions that lower something on its model)
TINY = {'w48': (case48, ('f16', 'f16s2', 'f16x')), 'w32': (case32, ('f16x',))}


@pytest.fixture(autouse=True, params=['all-classes', 'shipped'])
def _deterministic_tile_choice(request, monkeypatch):
    """As in tests/test_gpu_f16_mode.py: the fp32 layers run on the shipped table or the cost model, never on an in-process
    timing.  Every test runs with every qualifying tensor in f16 (engine.F16_STORAGE_FP32_CLASSES emptied: the rule itself)
    and with the shipped exceptions."""
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    if request.param == 'all-classes':
        monkeypatch.setattr(engine, 'F16_STORAGE_FP32_CLASSES', ())


def _flat(o):
    return o if isinstance(o, tuple) else (o,)


def _same(a, b):
    a, b = _flat(a), _flat(b)
    return len(a) == len(b) and all(p.dtype == q.dtype and torch.equal(p, q) for p, q in zip(a, b))


def _forward(net, x, activations):
    """(outputs, launches of the forward, tags of the lowered layers) under the switch."""
    L = _lib.lib()
    net.activations = activations
    n0 = L.egn_launch_count()
    with torch.no_grad():
        out = net(x)
    torch.cuda.synchronize()
    return out, L.egn_launch_count() - n0, list(net._hip_engine().last_f16_ops)


def _check_model(net, x, precisions):
    eng = net._hip_engine()
    for prec in precisions:
        net.precision = prec
        before = len(eng.programs)
        off, launches_off, tags_off = _forward(net, x, 'f32')
        on, launches_on, tags_on = _forward(net, x, 'f16')
        assert len(eng.programs) == before + 2                      # the two switches key separate programs
        key_on = [k for k in eng.programs if 'af16' in k and prec in k]
        key_off = [k for k in eng.programs if 'af16' not in k and prec in k]
        assert len(key_on) == 1 and len(key_off) == 1 and key_on[0][:len(key_off[0])] == key_off[0]
        p_on, p_off = eng.programs[key_on[0]], eng.programs[key_off[0]]
        # the switch does something: fewer bytes, a smaller or equal arena -- and not a bit of difference
        assert sum(m['bytes'] for m in p_on.meta) < sum(m['bytes'] for m in p_off.meta), prec
        assert p_on.arena_bytes <= p_off.arena_bytes
        assert [m['klass'] for m in p_on.meta] == [m['klass'] for m in p_off.meta]
        assert _same(on, off), prec
        assert launches_on == launches_off > 0 and tags_on == tags_off and len(tags_on) > 0
        for o in _flat(on):
            assert torch.isfinite(o).all()
        again, _, _ = _forward(net, x, 'f16')
        back, launches_back, _ = _forward(net, x, 'f32')             # switching back: the first program, its bits
        assert len(eng.programs) == before + 2
        assert _same(again, on) and _same(back, off) and launches_back == launches_off
    del net.activations


@pytest.mark.parametrize('head', ('heatmap', 'coordinates'))
@pytest.mark.parametrize('which', sorted(TINY))
def test_forward_keeps_every_bit(which, head):
    case, precisions = TINY[which]
    net = case.model(head).cuda()
    _check_model(net, case.crops('forward').cuda(), precisions)
    # precision = 'f32': nothing is lowered, nothing qualifies -- the same launches, the same bits
    net.precision = 'f32'
    x = case.crops('forward').cuda()
    off, launches_off, tags_off = _forward(net, x, 'f32')
    on, launches_on, tags_on = _forward(net, x, 'f16')
    assert _same(on, off) and launches_on == launches_off and tags_on == tags_off == []


@pytest.mark.parametrize('head', ('heatmap', 'coordinates'))
@pytest.mark.parametrize('which', sorted(TINY))
def test_infer_crops_keeps_every_bit(which, head):
    from egonet_amd.model.egonet import EgoNet
    case, precisions = TINY[which]
    cfg = case.config(head)
    J = cfg['heatmapModel']['num_joints']
    x = case.crops('infer_crops').cuda()
    n = x.shape[0]
    boxes = synth.synth_boxes(n, seed=3)
    centers = np.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2], axis=1)
    scales = np.stack([(boxes[:, 2] - boxes[:, 0]) / 200.0] * 2, axis=1)
    for prec in precisions:
        outs = {}
        for act in ('f32', 'f16'):
            ego = EgoNet(cfg, precision=prec, activations=act)
            ego.HC.load_state_dict(case.model(head).state_dict())
            ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=5))
            ego.LS = synth.synth_lifter_stats(2 * J, 3 * (J - 1))
            ego = ego.cuda().eval()
            assert ego.HC.precision == prec and ego.HC.activations == act
            L = _lib.lib()
            n0 = L.egn_launch_count()
            out = ego.infer_crops(x, centers, scales, to_host=False)
            torch.cuda.synchronize()
            outs[act] = (out, L.egn_launch_count() - n0, list(ego.HC._hip_engine().last_f16_ops),
                         [k for k in ego.HC._hip_engine().programs])
        (a, la, ta, ka), (b, lb, tb, kb) = outs['f32'], outs['f16']
        assert sorted(a) == sorted(b) and la == lb > 0 and ta == tb and len(ta) > 0
        assert all('af16' in k for k in kb) and not any('af16' in k for k in ka) and len(ka) == len(kb) == 1
        compared = 0
        for k in a:
            if torch.is_tensor(a[k]):
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (prec, k)
                compared += 1
            elif isinstance(a[k], np.ndarray):
                assert np.array_equal(a[k], b[k]), (prec, k)
                compared += 1
        assert compared > 0


@pytest.mark.parametrize('which', ('w48', 'w32'))
def test_full_model_keeps_every_bit(which):
    """The full HRNet-W48 (256 x 256) and HRNet-W32 (192 x 256) at 2 crops under 'f16x': 106 and 116 tensors in f16."""
    cfg = configs.w48_config('coordinates') if which == 'w48' else configs.ped_config('coordinates')
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=11))
    net = net.eval().cuda()
    iw, ih = cfg['heatmapModel']['input_size']
    x = synth.synth_crops(2, 3, ih, iw, seed=2).cuda()
    net.precision = 'f16x'
    off, launches_off, tags_off = _forward(net, x, 'f32')
    on, launches_on, tags_on = _forward(net, x, 'f16')
    assert _same(on, off) and launches_on == launches_off > 0 and tags_on == tags_off
    for o in _flat(on):
        assert torch.isfinite(o).all()
    eng = net._hip_engine()
    assert len(eng.programs) == 2 and sum(1 for k in eng.programs if 'af16' in k) == 1
    p_on = [p for k, p in eng.programs.items() if 'af16' in k][0]
    p_off = [p for k, p in eng.programs.items() if 'af16' not in k][0]
    assert sum(m['bytes'] for m in p_on.meta) < sum(m['bytes'] for m in p_off.meta)
    if not engine.F16_STORAGE_FP32_CLASSES:
        # every qualifying tensor saves 2 bytes an element on each side
        with torch.no_grad():
            rec, _, _ = eng._record(2, 3, ih, iw, None)
        f16 = engine.f16_storage(rec)
        assert len(f16) == (106 if which == 'w48' else 116)
