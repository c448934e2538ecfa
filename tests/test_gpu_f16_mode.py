"""precision = 'f16' end to end on the device (csrc/conv_h.hip under the recorded program) against the fp32 CPU forward.

The allowed error is not taken from the code under test: E comes from the CPU emulation of the mode
(tests/golden/make_f16_bounds.py -> tests/golden/f16_mode_bounds.json; model, inputs and quantities in
tests/f16_mode_case.py), and the device result must stay within 2 E of the fp32 CPU forward:
|gpu - f32| <= |gpu - emulation| + E, where the first term is made of the same f16 rounding decisions flipped by
fp32-level differences, so it is of the size of E and not larger.  Arg-max agreement with fp32 is printed, not asserted.
The reference runs these layers as fp32 torch calls (libs/model/heatmapModel/hrnet.py:63-92)."""
import json

import numpy as np
import pytest
import torch

import f16_mode_case as case
from egonet_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _deterministic_tile_choice(monkeypatch):
    """The fp32 layers around the f16 ones run on the shipped table or the cost model, never on an in-process timing:
    which configuration wins a timing can change from run to run, fp32-level differences in front of an f16 rounding
    flip it, and E for the coordinates is a few units in the last place -- the test must compute the same bits every time."""
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


def _check(q, head, which, bounds, label, enforce=True):
    ref, E = _reference(head, which), bounds[head][which]
    dev = case.deviations(q, ref)
    for k in sorted(dev):
        print('%s %s %s: |device - fp32 CPU| = %.3e, E = %.3e (allowed 2 E = %.3e)' % (label, head, k, dev[k], E[k], 2 * E[k]))
    same = (q['heatmap'].flatten(2).argmax(2) == ref['heatmap'].flatten(2).argmax(2)).double().mean()
    print('%s %s: heat-map arg-max agrees with fp32 on %.1f %% of the maps' % (label, head, 100.0 * float(same)))
    for k in sorted(dev):
        assert not enforce or dev[k] <= 2 * E[k], (label, head, k, dev[k], E[k])
    return dev


@pytest.mark.parametrize('head', case.HEADS)
def test_f16_mode_against_the_fp32_cpu_forward(head, bounds):
    x = case.crops('forward')
    net = case.model(head).cuda()
    with torch.no_grad():
        never_set = net(x.cuda())                       # the attribute never set: the default program
        assert net._hip_engine().last_f16_ops == []
        net.precision = 'f32'
        explicit = net(x.cuda())
        net.precision = 'f16'
        fast = net(x.cuda())
        tags = list(net._hip_engine().last_f16_ops)
        again = net(x.cuda())
    flat = (lambda o: o if isinstance(o, tuple) else (o,))
    assert all(torch.equal(a, b) for a, b in zip(flat(never_set), flat(explicit)))       # 'f32' is the default, bit for bit
    assert all(torch.equal(a, b) for a, b in zip(flat(fast), flat(again)))
    assert not all(torch.equal(a, b) for a, b in zip(flat(fast), flat(never_set)))       # the switch does something
    # the lowered layers: the set the CPU test derives from engine.f16_eligible (tests/test_f16_mode_cpu.py)
    assert len(tags) == bounds[head]['forward']['f16_convs'] == 18
    import torch.nn as nn
    want = {name for name, m in net.named_modules() if isinstance(m, nn.Conv2d) and name.startswith('stage')
            and m.kernel_size == (3, 3) and m.stride == (1, 1)}
    assert set(tags) == want
    assert {k[-1] for k in net._hip_engine().programs if k[-1] == 'f16'} == {'f16'} and len(net._hip_engine().programs) == 2
    _check(case.quantities(never_set), head, 'forward', bounds, "'f32'", enforce=False)      # (printed: the fp32 program's own distance)
    _check(case.quantities(fast), head, 'forward', bounds, "'f16'")


def test_infer_crops_in_f16_mode(bounds):
    """EgoNet.infer_crops(precision = 'f16') on 4 crops: finite results, key points within 2 E of the fp32 CPU forward."""
    from egonet_amd.model.egonet import EgoNet
    head, which = 'coordinates', 'infer_crops'
    cfg = case.config(head)
    ego = EgoNet(cfg, precision='f16')
    ego.HC.load_state_dict(case.model(head).state_dict())
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=5))
    J = cfg['heatmapModel']['num_joints']
    ego.LS = synth.synth_lifter_stats(2 * J, 3 * (J - 1))
    ego = ego.cuda().eval()
    assert ego.HC.precision == 'f16'
    x = case.crops(which)
    n = x.shape[0]
    boxes = synth.synth_boxes(n, seed=3)
    centers = np.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2], axis=1)
    scales = np.stack([(boxes[:, 2] - boxes[:, 0]) / 200.0] * 2, axis=1)
    out = ego.infer_crops(x.cuda(), centers, scales, to_host=False)
    assert len(ego.HC._hip_engine().last_f16_ops) == 18
    for k, v in out.items():
        if torch.is_tensor(v) and v.is_floating_point():
            assert torch.isfinite(v).all(), k
    ref = _reference(head, which)
    got = out['local'].detach().cpu().double() * case.SIZE
    dev, E = float((got - ref['coords_px']).abs().max()), bounds[head][which]['coords_px']
    print('infer_crops key points: |device - fp32 CPU| = %.3e px, E = %.3e (allowed 2 E = %.3e)' % (dev, E, 2 * E))
    assert dev <= 2 * E, (dev, E)
