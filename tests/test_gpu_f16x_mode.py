"""precision = 'f16x' end to end on the device (what 'f16s2' lowers plus the 3x3 layers of the 32-multiple widths on
csrc/conv_h.hip with CK = 32, under the recorded program) against the fp32 CPU forward.

The rule of tests/test_gpu_f16_mode.py and tests/test_gpu_f16s2_mode.py: the allowed error is not taken from the code
under test.  E comes from the CPU emulation of the mode (tests/golden/make_f16x_bounds.py ->
tests/golden/f16x_mode_bounds.json; model, inputs and quantities in tests/f16x_mode_case.py: HRNet with the W32 widths on
the 192 x 256 Pedestrian input), and the device result must stay within 2 E of the fp32 CPU forward.  'f16' and 'f16s2'
must compute in the same process, after 'f16x' was visited, the bits they computed before.  The reference runs these
layers as fp32 torch calls (libs/model/heatmapModel/hrnet.py)."""
import json

import numpy as np
import pytest
import torch

import f16x_mode_case as case
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
def test_f16x_mode_against_the_fp32_cpu_forward(head, bounds):
    x = case.crops('forward')
    net = case.model(head).cuda()
    with torch.no_grad():
        net.precision = 'f32'
        plain = net(x.cuda())
        net.precision = 'f16s2'
        s2 = net(x.cuda())
        tags2 = list(net._hip_engine().last_f16_ops)
        net.precision = 'f16x'
        fast = net(x.cuda())
        tags = list(net._hip_engine().last_f16_ops)
        again = net(x.cuda())
    assert _same(fast, again)                           # repeatable bit for bit
    assert tags2 == [] and _same(s2, plain)             # a W32 model: 'f16s2' lowers nothing and computes the fp32 bits
    assert not _same(fast, s2)                          # the new switch does something
    assert len(tags) == len(set(tags)) == bounds[head]['forward']['f16_convs'] > 0
    progs = net._hip_engine().programs                  # the precision is part of the program key
    assert len(progs) == 3 and {k[-1] for k in progs if k[-1] in engine.ALL_PRECISIONS} == {'f16s2', 'f16x'}
    _check(case.quantities(fast), head, 'forward', bounds, "'f16x'")


def test_the_old_modes_keep_their_bits_after_f16x_was_visited():
    """On the model with the W48 widths (tests/f16_mode_case.py): 'f16' and 'f16s2' compute the same bits before and after
    'f16x' ran in the same process, and 'f16x' -- which adds layer1, the stem's second convolution and transition1 there --
    does not compute theirs."""
    import f16_mode_case as w48
    x = w48.crops('forward').cuda()
    net = w48.model('coordinates').cuda()
    out, tags = {}, {}
    with torch.no_grad():
        for prec in ('f16', 'f16s2', 'f16x', 'f16', 'f16s2'):
            net.precision = prec
            out.setdefault(prec, []).append(net(x))
            if len(out[prec]) == 1:            # (the first visit records the mode's program; the second finds it)
                tags[prec] = set(net._hip_engine().last_f16_ops)
    tags2, tagsx = tags['f16s2'], tags['f16x']
    assert _same(out['f16'][0], out['f16'][1]) and _same(out['f16s2'][0], out['f16s2'][1])
    extra = tagsx - tags2
    assert tags2 <= tagsx and all(t == 'conv2' or t.startswith(('layer1.', 'transition1.')) for t in extra)
    if not engine.F16X_FP32_CLASSES:
        assert {'conv2', 'layer1.0.conv2', 'transition1.0', 'transition1.1.0'} <= extra
    assert _same(out['f16x'][0], out['f16s2'][0]) == (not extra)       # (every added class measured not to win: the same program)
    for o in _flat(out['f16x'][0]):
        assert torch.isfinite(o).all()


def test_infer_crops_in_f16x_mode(bounds):
    """EgoNet.infer_crops(precision = 'f16x') on 3 crops: finite results, key points within 2 E of the fp32 CPU forward."""
    from egonet_amd.model.egonet import EgoNet
    head, which = 'coordinates', 'infer_crops'
    cfg = case.config(head)
    ego = EgoNet(cfg, precision='f16x')
    ego.HC.load_state_dict(case.model(head).state_dict())
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=5))
    J = cfg['heatmapModel']['num_joints']
    ego.LS = synth.synth_lifter_stats(2 * J, 3 * (J - 1))
    ego = ego.cuda().eval()
    assert ego.HC.precision == 'f16x'
    x = case.crops(which)
    n = x.shape[0]
    boxes = synth.synth_boxes(n, seed=3)
    centers = np.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2], axis=1)
    scales = np.stack([(boxes[:, 2] - boxes[:, 0]) / 200.0] * 2, axis=1)
    out = ego.infer_crops(x.cuda(), centers, scales, to_host=False)
    assert len(ego.HC._hip_engine().last_f16_ops) == bounds[head][which]['f16_convs'] > 0
    for k, v in out.items():
        if torch.is_tensor(v) and v.is_floating_point():
            assert torch.isfinite(v).all(), k
    ref = _reference(head, which)
    got = out['local'].detach().cpu().double() * torch.tensor([case.WIDTH, case.HEIGHT], dtype=torch.float64)
    dev, E = float((got - ref['coords_px']).abs().max()), bounds[head][which]['coords_px']
    print('infer_crops key points: |device - fp32 CPU| = %.3e px, E = %.3e (allowed 2 E = %.3e)' % (dev, E, 2 * E))
    assert dev <= 2 * E, (dev, E)
