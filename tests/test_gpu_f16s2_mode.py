"""precision = 'f16s2' end to end on the device ('f16' plus the 3x3 stride-2 layers on csrc/conv_h.hip with S = 2, under the
recorded program) against the fp32 CPU forward.

The rule and the quantities of tests/test_gpu_f16_mode.py: the allowed error is not taken from the code under test.  E
comes from the CPU emulation of the mode (tests/golden/make_f16s2_bounds.py -> tests/golden/f16s2_mode_bounds.json;
model, inputs and quantities in tests/f16_mode_case.py), and the device result must stay within 2 E of the fp32 CPU
forward.  'f16' must compute in the same process, after 'f16s2' was visited, the bits it computed before.  The reference
runs these layers as fp32 torch calls (libs/model/heatmapModel/hrnet.py, the transition and fuse layers)."""
import json

import numpy as np
import pytest
import torch
import torch.nn as nn

import f16s2_mode_case as case
from egonet_amd import engine, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _deterministic_tile_choice(monkeypatch):
    """As in tests/test_gpu_f16_mode.py: the fp32 layers around the f16 ones run on the shipped table or the cost model,
    never on an in-process timing -- the test must compute the same bits every time."""
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')


@pytest.fixture(scope='module')
def bounds():
    with open(case.BOUNDS_PATH) as f:
        return json.load(f)


_REF = {}


def _reference(head, which):
    """The fp32 CPU forward's quantities, computed once per (head, batch)."""
    if (head, which) not in _REF:
        _REF[(head, which)] = case.cpu_f32(case.model(head), case.crops(which))
    return _REF[(head, which)]


def _check(q, head, which, bounds, label):
    ref, E = _reference(head, which), bounds[head][which]
    dev = case.deviations(q, ref)
    for k in sorted(dev):
        print('%s %s %s: |device - fp32 CPU| = %.3e, E = %.3e (allowed 2 E = %.3e)' % (label, head, k, dev[k], E[k], 2 * E[k]))
    for k in sorted(dev):
        assert dev[k] <= 2 * E[k], (label, head, k, dev[k], E[k])


def _flat(o):
    return o if isinstance(o, tuple) else (o,)


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(_flat(a), _flat(b)))


@pytest.mark.parametrize('head', case.HEADS)
def test_f16s2_mode_against_the_fp32_cpu_forward(head, bounds):
    x = case.crops('forward')
    net = case.model(head).cuda()
    with torch.no_grad():
        net.precision = 'f16'
        f16_before = net(x.cuda())
        tags16 = list(net._hip_engine().last_f16_ops)
        net.precision = 'f16s2'
        fast = net(x.cuda())
        tags = list(net._hip_engine().last_f16_ops)
        again = net(x.cuda())
        net.precision = 'f16'
        f16_after = net(x.cuda())
    assert _same(fast, again)                           # repeatable bit for bit
    assert not _same(fast, f16_before)                  # the wider switch does something
    assert _same(f16_before, f16_after)                 # 'f16' keeps its bits after 'f16s2' was visited
    # the lowered layers: the sets the CPU test derives from the two rules (tests/test_f16s2_mode_cpu.py)
    assert len(tags16) == 18 and len(tags) == bounds[head]['forward']['f16_convs']
    s1 = {name for name, m in net.named_modules() if isinstance(m, nn.Conv2d) and name.startswith('stage')
          and m.kernel_size == (3, 3) and m.stride == (1, 1)}
    s2 = {name[:-2] for name, m in net.named_modules() if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3)
          and m.stride == (2, 2) and name.startswith(('transition2', 'transition3', 'stage'))
          and (m.in_channels, m.out_channels) not in engine.F16S2_FP32_CLASSES}
    assert set(tags16) == s1 and set(tags) == s1 | s2 and len(s2) == bounds[head]['forward']['f16s2_convs'] > 0
    assert {k[-1] for k in net._hip_engine().programs} == {'f16', 'f16s2'}
    _check(case.quantities(fast), head, 'forward', bounds, "'f16s2'")


def test_infer_crops_in_f16s2_mode(bounds):
    """EgoNet.infer_crops(precision = 'f16s2') on 4 crops: finite results, key points within 2 E of the fp32 CPU forward."""
    from egonet_amd.model.egonet import EgoNet
    head, which = 'coordinates', 'infer_crops'
    cfg = case.config(head)
    ego = EgoNet(cfg, precision='f16s2')
    ego.HC.load_state_dict(case.model(head).state_dict())
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=5))
    J = cfg['heatmapModel']['num_joints']
    ego.LS = synth.synth_lifter_stats(2 * J, 3 * (J - 1))
    ego = ego.cuda().eval()
    assert ego.HC.precision == 'f16s2' and engine.PRECISIONS[-1] == 'f16s2'
    x = case.crops(which)
    n = x.shape[0]
    boxes = synth.synth_boxes(n, seed=3)
    centers = np.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2], axis=1)
    scales = np.stack([(boxes[:, 2] - boxes[:, 0]) / 200.0] * 2, axis=1)
    out = ego.infer_crops(x.cuda(), centers, scales, to_host=False)
    assert len(ego.HC._hip_engine().last_f16_ops) == bounds[head][which]['f16_convs'] > 18
    for k, v in out.items():
        if torch.is_tensor(v) and v.is_floating_point():
            assert torch.isfinite(v).all(), k
    ref = _reference(head, which)
    got = out['local'].detach().cpu().double() * case.SIZE
    dev, E = float((got - ref['coords_px']).abs().max()), bounds[head][which]['coords_px']
    print('infer_crops key points: |device - fp32 CPU| = %.3e px, E = %.3e (allowed 2 E = %.3e)' % (dev, E, 2 * E))
    assert dev <= 2 * E, (dev, E)
