"""Inference plans on the GPU (egonet_amd/plan.py, csrc/plan_run.hip): a plan replays the launches of the engine that
wrote it with the same arguments, so on every output ``Plan.infer_crops`` returns the BYTES of ``EgoNet.infer_crops`` on
the exporting model -- in the same process, and from tools/_build/egonet_run in a fresh one without Python."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from egonet_amd import _lib, build, configs, plan, synth
from egonet_amd.common.img_proc import modify_bbox
from egonet_amd.model.egonet import EgoNet

pytestmark = pytest.mark.gpu
K = np.array([[707.0493, 0., 604.0814], [0., 707.0493, 180.5066], [0., 0., 1.]])
KEYS = ('local', 'kpts_2d', 'kpts_3d', 'euler', 'alpha', 'translation')


@pytest.fixture(scope='module', autouse=True)
def _table_or_cost_model():
    # the tiny shapes are in no shipped table: without this every recording would time its candidates (seconds per
    # program, and a choice that depends on the noise of the moment)
    mp = pytest.MonkeyPatch()
    mp.setenv('EGONET_AMD_AUTOTUNE', '0')
    yield
    mp.undo()


def make_ego(cfg, precision=None, J=33):
    ego = EgoNet(cfg, pre_trained=False, precision=precision)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=6))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=7))
    ego.LS = synth.synth_lifter_stats(2 * J, (J - 1) * 3, seed=1)
    return ego.eval().cuda()


def case(ego, n, seed=8):
    w, h = ego.resolution
    crops = synth.synth_crops(n, 3, h, w, seed=seed)
    rets = [modify_bbox(b, h / w) for b in synth.synth_boxes(n, seed=2)]
    return crops, np.stack([r['c'] for r in rets]), np.stack([r['s'] for r in rets])


def same_bytes(got, want, what):
    assert list(got.keys()) == list(want.keys()), (what, list(got), list(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k, float(np.abs(got[k] - want[k]).max()))


def check(ego, P, n, decode='auto', what=''):
    crops, c, s = case(ego, n)
    want = ego.infer_crops(crops.cuda(), c, s, K=K, decode=decode)
    got = P.infer_crops(crops.cuda(), c, s, K=K)
    assert tuple(want.keys()) == KEYS
    same_bytes(got, want, '%s n=%d' % (what, n))
    return got


@pytest.fixture(scope='module')
def tiny(tmp_path_factory, _table_or_cost_model):
    ego = make_ego(configs.tiny_config('coordinates', num_joints=33))
    path = str(tmp_path_factory.mktemp('plan') / 'tiny.egnplan')
    plan.export_plan(ego, path, batch_sizes=(1, 4))
    return ego, path, plan.Plan(path).load('cuda:0')


@pytest.mark.parametrize('n', [1, 4, 5, 3])
def test_same_process(tiny, n):
    """5 = 4 + 1 and 3 = 1 + 1 + 1 run as chunks of the exported sizes."""
    ego, _, P = tiny
    before = _lib.lib().egn_launch_count()
    check(ego, P, n, what='tiny')
    assert _lib.lib().egn_launch_count() > before
    crops, c, s = case(ego, n)
    dev = P.infer_crops(crops.cuda(), c, s, K=None, alpha_mode='trans', to_host=False)
    want = ego.infer_crops(crops.cuda(), c, s, K=None, alpha_mode='trans', to_host=False)
    assert all(v.is_cuda for v in dev.values())
    same_bytes({k: v.cpu().numpy() for k, v in dev.items()}, {k: v.cpu().numpy() for k, v in want.items()}, 'no K')


def test_uncomposable_batch_is_refused_before_any_launch(tmp_path):
    ego = make_ego(configs.tiny_config('coordinates', num_joints=33))
    path = str(tmp_path / 't.egnplan')
    plan.export_plan(ego, path, batch_sizes=(2, 4))
    P = plan.Plan(path).load('cuda:0')
    crops, c, s = case(ego, 3)
    torch.cuda.synchronize()
    before = _lib.lib().egn_launch_count()
    with pytest.raises(ValueError):
        P.infer_crops(crops.cuda(), c, s, K=K)
    assert _lib.lib().egn_launch_count() == before
    check(ego, P, 6, what='4 + 2')
    P.close()


@pytest.mark.parametrize('decode', ['soft', 'hard'])
def test_heatmap_head(tmp_path, decode):
    ego = make_ego(configs.tiny_config('heatmap', num_joints=33))
    path = str(tmp_path / 'hm.egnplan')
    plan.export_plan(ego, path, batch_sizes=(1, 4), decode=decode)
    P = plan.Plan(path).load('cuda:0')
    assert P.info['decode'] == decode and P.info['head_type'] == 'heatmap'
    assert 6 in P.program_info(0)['kinds']            # the decode op
    for n in (4, 2):
        check(ego, P, n, decode=decode, what=decode)
    P.close()


def test_non_square_input(tmp_path):
    """With the heat-map head: the tiny coordinate head has no 64 x 96 form (its last layer wants a square map)."""
    ego = make_ego(configs.tiny_config('heatmap', input_size=(64, 96), num_joints=33))
    path = str(tmp_path / 'ns.egnplan')
    plan.export_plan(ego, path, batch_sizes=(1, 2))
    P = plan.Plan(path).load('cuda:0')
    assert (P.info['W'], P.info['H']) == (64, 96)
    for n in (2, 3):
        check(ego, P, n, what='64 x 96')
    P.close()


def test_f16x_precision(tmp_path):
    ego = make_ego(configs.tiny_config('coordinates', num_joints=33), precision='f16x')
    path = str(tmp_path / 'hx.egnplan')
    plan.export_plan(ego, path, batch_sizes=(2,))
    P = plan.Plan(path).load('cuda:0')
    assert P.info['precision'] == 'f16x'
    assert 14 in P.program_info(0)['kinds'], 'no f16-operand op (kind 14) in the f16x plan'
    check(ego, P, 2, what='f16x')
    P.close()


def test_lanes_and_dependencies_at_16(tmp_path):
    ego = make_ego(configs.tiny_config('coordinates', num_joints=33))
    path = str(tmp_path / 'n16.egnplan')
    plan.export_plan(ego, path, batch_sizes=(16,))
    P = plan.Plan(path).load('cuda:0')
    info = P.program_info(0)
    assert info['ops_with_waits'] > 0 and 7 in info['kinds'], info
    check(ego, P, 16, what='16 crops')
    P.close()


def test_w48_two_crops(tmp_path):
    """The fused layer1 pairs, the stem, the F(4x4,3x3) families and the K-split ops that own ticket words."""
    ego = make_ego(configs.w48_config('coordinates'))
    path = str(tmp_path / 'w48.egnplan')
    plan.export_plan(ego, path, batch_sizes=(2,))
    P = plan.Plan(path).load('cuda:0')
    kinds = P.program_info(0)['kinds']
    assert 10 in kinds and len(kinds) > 250
    check(ego, P, 2, what='W48')
    crops, _, _ = case(ego, 2)
    L = _lib.lib()
    native = ego.HC._hip_engine().program(crops.cuda(), None)
    assert L.egn_program_ticket_ops(P.native_program(0)) == L.egn_program_ticket_ops(native.handle)
    assert L.egn_program_num_ops(P.native_program(0)) == L.egn_program_num_ops(native.handle)
    P.close()


def test_fresh_process_without_python(tiny, tmp_path):
    ego, path, P = tiny
    spec = importlib.util.spec_from_file_location('export_plan_tool', os.path.join(ROOT, 'tools', 'export_plan.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    n = 5
    crops, c, s = case(ego, n)
    want = P.infer_crops(crops.cuda(), c, s, K=K)
    same_bytes(want, ego.infer_crops(crops.cuda(), c, s, K=K), 'plan vs model')
    case_path = tool.write_case(str(tmp_path / 'five.case'), crops.numpy(), c, s, K)
    exe = build.RUN_OUT if os.path.isfile(build.RUN_OUT) else build.build_run(verbose=False)     # (build() makes it)
    out_dir = tmp_path / 'out'
    out_dir.mkdir()
    r = subprocess.run([exe, path, case_path, str(out_dir)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    got = tool.read_outputs(str(out_dir), n, 33, 96)
    same_bytes(got, want, 'egonet_run')
    # the plan holds its own weights: the exporting model's are overwritten, the plan's answer does not move
    params = list(ego.HC.parameters()) + list(ego.L.parameters())
    with torch.no_grad():
        for p in params:
            p.mul_(0.5)
    try:
        moved = ego.infer_crops(crops.cuda(), c, s, K=K)
        assert moved['kpts_3d'].tobytes() != want['kpts_3d'].tobytes()
        same_bytes(P.infer_crops(crops.cuda(), c, s, K=K), want, 'after the model changed')
    finally:
        with torch.no_grad():          # (the fixture is shared: a power of two, so the weights come back exactly)
            for p in params:
                p.mul_(2.0)
