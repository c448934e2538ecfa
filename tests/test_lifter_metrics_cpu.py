"""The lifter's 3-D metrics without a GPU: the host path of RError3D / RTError3D / JointDistance3D / RotationError3D /
Evaluator (egonet_amd/metric/criterions.py) on the reference-generated fixture, the refused styles, the Evaluator
that ``trainer.train`` builds from ``eval_metrics``, and the ABI names of the device path."""
import json
import logging
import re

import numpy as np
import pytest
import torch

from conftest import golden
from egonet_amd import _lib, trainer
from egonet_amd.metric import criterions as cr

CASES = {'RError3D': lambda c: cr.RError3D(c, 33), 'RTError3D': lambda c: cr.RTError3D(c, 33),
         'JointDistance3D': lambda c: cr.JointDistance3D(c), 'RotationError3D': lambda c: cr.RotationError3D(c),
         'Evaluator': lambda c: cr.Evaluator(['RError3D'], c, 33)}
_NUM = re.compile(r'[-+]?(?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?')


def _skeleton(line):
    """The text around the numbers: numpy pads an array's columns to its widest element and wraps its rows at 75
    characters, which is formatting."""
    line = re.sub(r'[ \n]+', ' ', _NUM.sub('#', line))
    return line.replace('[ ', '[').replace(' ]', ']')


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _logger(name='egonet_amd.test_lifter_metrics'):
    lg = logging.getLogger(name)
    lg.setLevel(logging.INFO)
    lg.propagate = False
    h = _Lines()
    lg.handlers = [h]
    return lg, h


def _cfgs(g):
    return json.loads(str(g['cfgs']))


def _attr_names(g, name):
    return [k.split('/')[1] for k in g.files
            if k.startswith(name + '/') and k.split('/')[1].split('_')[0] in ('count', 'mean', 'max', 'min')]


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('unnormalised', [False, True])
def test_host_path_against_the_reference_attributes(name, unnormalised):
    """The host path is float64, the reference float32 in distances, H and SVD: the bound per attribute is ten times
    the gap the generator measured between its float64 restatement and the reference (stored under gap/)."""
    g = golden('lifter_metrics.npz')
    layout = str(g[name + '/layout'])
    pred, gt = g[layout + '/pred'], g[layout + '/gt']
    stats = {'mean_out': g[layout + '/mean_out'], 'std_out': g[layout + '/std_out']}
    obj = CASES[name](_cfgs(g))
    b0 = 0
    for b in g['batches']:
        p, t = pred[b0:b0 + b], gt[b0:b0 + b]
        if unnormalised:                            # what trainer.evaluate hands over for a host evaluator
            obj.update(p * stats['std_out'] + stats['mean_out'], ground_truth=t * stats['std_out'] + stats['mean_out'])
        else:
            obj.update(p, ground_truth=t, statistics=stats)
        b0 += int(b)
    metric = obj.metrics[0] if name == 'Evaluator' else obj
    names = _attr_names(g, name)
    assert names
    worst = 10.0 * max(float(g['gap/%s/%s' % (name, a)]) for a in names)
    for a in names:
        want, got = g['%s/%s' % (name, a)], getattr(metric, a)
        bound = 10.0 * float(g['gap/%s/%s' % (name, a)])
        if a.startswith('count'):
            assert int(got) == int(want) == 300
            continue
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape
        err = float(np.max(np.abs(got - want)))
        print('%s.%s: max |host - reference| %.3e, bound %.3e' % (name, a, err, bound))
        assert err <= bound
    # report(): the reference's text, character for character around the numbers; the numbers are the attributes
    # above printed with 8 significant digits: the largest attribute bound of the class plus that rounding
    lg, h = _logger()
    obj.report(lg)
    want_lines = json.loads(str(g[name + '/report']))
    assert len(h.lines) == len(want_lines) == 1
    for got_line, want_line in zip(h.lines, want_lines):
        assert _skeleton(got_line) == _skeleton(want_line)
        a = np.array([float(x) for x in _NUM.findall(got_line)])
        b = np.array([float(x) for x in _NUM.findall(want_line)])
        np.testing.assert_allclose(a, b, rtol=1e-7, atol=worst)


def test_evaluator_name_table():
    g = golden('lifter_metrics.npz')
    cfgs = _cfgs(g)
    cfgs['FCModel'] = {'output_size': 96}
    ev = cr.Evaluator(['RError3D', 'RTError3D', 'JointDistance3D', 'RotationError3D'], cfgs, 33)
    assert [type(m).__name__ for m in ev.metrics] == ['RError3D', 'RTError3D', 'JointDistance3D', 'RotationError3D']
    assert ev.device_update is True
    assert ev.metrics[0].num_joints == 32 and ev.metrics[0].name == 'RError3D'
    assert ev.metrics[0].count_rT == 0 and np.array_equal(ev.metrics[0].max_R, -np.ones(3))
    assert np.array_equal(ev.metrics[1].min_T_xyz, np.ones(3) * 1e16) and ev.metrics[1].mean_T.shape == (1,)
    with pytest.raises(NotImplementedError, match='NoSuchMetric'):
        cr.Evaluator(['RError3D', 'NoSuchMetric'], cfgs, 33)
    with pytest.raises(NotImplementedError):
        cr.Evaluator(['__import__("os").getcwd() or RError3D'], cfgs, 33)      # a table, not eval()
    with pytest.raises(AttributeError):
        ev.metrics[0].no_such_attribute


def test_out_of_scope_styles_are_refused():
    g = golden('lifter_metrics.npz')
    for path, value, make in (
            (('metrics', 'R3D', 'T_style'), 'procrustes', lambda c: cr.RError3D(c, 33)),
            (('metrics', 'RTError3D', 'T_style'), 'procrustes', lambda c: cr.RTError3D(c, 33)),
            (('metrics', 'JD3D', 'style'), 'procrustes', lambda c: cr.JointDistance3D(c)),
            (('metrics', 'R3D', 'R_style'), 'quaternion', lambda c: cr.RError3D(c, 33)),
            (('metrics', 'R3D', 'style'), 'quaternion', lambda c: cr.RotationError3D(c)),
            (('dataset', '3d_kpt_sample_style'), 'bbox27', lambda c: cr.RError3D(c, 33)),
            (('dataset', '3d_kpt_sample_style'), 'bbox27', lambda c: cr.RTError3D(c, 33))):
        cfgs = _cfgs(g)
        cfgs[path[0]] = dict(cfgs[path[0]])
        if len(path) == 3:
            cfgs[path[0]][path[1]] = dict(cfgs[path[0]][path[1]], **{path[2]: value})
        else:
            cfgs[path[0]][path[1]] = value
        with pytest.raises(NotImplementedError, match=r'criterions\.py:\d+'):
            make(cfgs)


def test_train_builds_the_evaluator_from_eval_metrics(monkeypatch):
    """trainer.py:151-156: eval_during + eval_metrics and nothing passed in -> Evaluator(eval_metrics, cfgs,
    train_dataset.num_joints), handed to evaluate().  The native step is stubbed: no GPU here."""
    g = golden('lifter_metrics.npz')
    cfgs = _cfgs(g)
    cfgs['training_settings'] = {'total_epochs': 1, 'report_every': 1, 'batch_size': 4, 'num_threads': 0,
                                 'shuffle': False, 'eval_during': True, 'eval_every': 1, 'eval_start_epoch': 0,
                                 'eval_metrics': ['RError3D']}
    seen = []

    class _Step(object):
        dev, lr = torch.device('cpu'), 0.0

        def step(self, data, target):
            return torch.zeros(())

    class _Set(torch.utils.data.Dataset):
        num_joints = 33

        def __len__(self):
            return 12

        def __getitem__(self, i):
            return torch.zeros(66), torch.zeros(96), torch.ones(1), {}

    def fake_evaluate(ds, model, loss_func, cfgs_, logger, evaluator, **kw):
        seen.append(evaluator)

    monkeypatch.setattr(trainer, 'make_step', lambda *a, **k: _Step())
    monkeypatch.setattr(trainer, 'evaluate', fake_evaluate)
    lg, h = _logger()
    trainer.train(_Set(), torch.nn.Linear(66, 96), None, None, None, cfgs, lg, valid_dataset=_Set())
    assert len(seen) == 2 and seen[0] is seen[1]                     # batches 1 and 2; one object for the run
    assert isinstance(seen[0], cr.Evaluator) and type(seen[0].metrics[0]) is cr.RError3D
    assert seen[0].metrics[0].num_joints == 32
    assert not any('no validation during training' in l for l in h.lines)
    # without eval_metrics the warning stays
    del cfgs['training_settings']['eval_metrics']
    del seen[:]
    lg, h = _logger()
    trainer.train(_Set(), torch.nn.Linear(66, 96), None, None, None, cfgs, lg, valid_dataset=_Set())
    assert not seen and any('no validation during training' in l for l in h.lines)


def test_abi_names_in_header_and_ctypes_table():
    src = open(_lib.HEADER_PATH).read()
    for name in ('egn_lifter_metrics_ws_bytes', 'egn_lifter_metrics_reset', 'egn_lifter_metrics_update_f32'):
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['egn_lifter_metrics_update_f32'][1]) == 13
    assert int(re.search(r'#define EGN_LIFTER_METRICS_ACC_DOUBLES (\d+)', src).group(1)) == cr._ACC_DOUBLES
