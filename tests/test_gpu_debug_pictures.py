"""The training debug pictures on the GPU (csrc/debug_pictures.hip): the kernels give the bytes of their host twins on
the smallest shapes at which they take another path, leave padding bytes and refused buffers alone, run on a side
stream, and carry ``trainer.train(save_debug=True)`` end to end without changing the step."""
import logging
import os

import numpy as np
import pytest
import torch

import debug_pictures_ref as ref
from egonet_amd import _lib, configs, synth, trainer
from egonet_amd.model.heatmapModel import hrnet
from egonet_amd.visualization import debug as dbg

pytestmark = pytest.mark.gpu
PAD = 0xA5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _range_device(x, c_used=3, offset=0):
    """egn_debug_range_f32 on x [n, c, hw] -> (code, lohi read back); ``offset``: floats the device copy is shifted
    by inside its allocation (1: no 16-byte alignment)."""
    L = _lib.lib()
    n, c, hw = x.shape
    hold = torch.zeros(x.size + offset, dtype=torch.float32, device='cuda')
    d = hold[offset:]
    d.copy_(torch.from_numpy(x.reshape(-1)))
    ws_bytes = L.egn_debug_range_ws_bytes(n, c_used, hw)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device='cuda')
    lohi = torch.full((2,), 77.0, dtype=torch.float32, device='cuda')
    code = L.egn_debug_range_f32(_lib.ptr(d), n, c, c_used, hw, _lib.ptr(ws), ws_bytes, _lib.ptr(lohi),
                                 _lib.current_stream())
    torch.cuda.synchronize()
    return code, lohi.cpu().numpy()


def _host_range(x, c_used=3):
    n, c, hw = x.shape
    lohi = np.full(2, 77.0, dtype=np.float32)
    code = _lib.lib().egn_debug_range_host_f32(x.ctypes.data, n, c, c_used, hw, lohi.ctypes.data)
    return code, lohi


def _compose_both(x, m, lohi, nrow, extra):
    """Grid and mosaic of one case by the device entries and by the host twins, into buffers whose rows carry
    ``extra`` padding bytes -> [(name, device buffer read back, host buffer, bytes of a row that belong to the
    picture)]."""
    L, lut = _lib.lib(), dbg.jet_lut()
    N, C, H, W = x.shape
    n, J, h, w = m.shape
    _, _, gh, gw = dbg.grid_layout(N, H, W, nrow, 2)
    d_x, d_m, d_lohi, d_lut = _dev(x), _dev(m), _dev(lohi), _dev(lut)
    out = []
    g_dev = torch.full((gh, 3 * gw + extra), PAD, dtype=torch.uint8, device='cuda')
    g_host = np.full((gh, 3 * gw + extra), PAD, dtype=np.uint8)
    assert L.egn_debug_grid_u8(_lib.ptr(d_x), N, C, H, W, nrow, 2, _lib.ptr(d_lohi), _lib.ptr(g_dev), g_dev.stride(0),
                               _lib.current_stream()) == 0
    assert L.egn_debug_grid_host_u8(x.ctypes.data, N, C, H, W, nrow, 2, lohi.ctypes.data, g_host.ctypes.data,
                                    g_host.strides[0]) == 0
    out.append(('grid', g_dev, g_host, 3 * gw))
    mw = 3 * (J + 1) * w
    m_dev = torch.full((n * h, mw + extra), PAD, dtype=torch.uint8, device='cuda')
    m_host = np.full((n * h, mw + extra), PAD, dtype=np.uint8)
    assert L.egn_debug_mosaic_u8(_lib.ptr(d_x), C, H, W, _lib.ptr(d_m), n, J, h, w, _lib.ptr(d_lohi), _lib.ptr(d_lut),
                                 _lib.ptr(m_dev), m_dev.stride(0), _lib.current_stream()) == 0
    assert L.egn_debug_mosaic_host_u8(x.ctypes.data, C, H, W, m.ctypes.data, n, J, h, w, lohi.ctypes.data,
                                      lut.ctypes.data, m_host.ctypes.data, m_host.strides[0]) == 0
    out.append(('mosaic', m_dev, m_host, mw))
    torch.cuda.current_stream().synchronize()
    return [(name, d.cpu().numpy(), hst, width) for name, d, hst, width in out]


@pytest.mark.parametrize('case', ref.CASES, ids=[c[0] for c in ref.CASES])
def test_device_bytes_equal_the_host_twin(case):
    name, N, C, H, W, nrow, n, J, h, w, kind = case
    x, m = ref.build_case(N, C, H, W, n, J, h, w, seed=len(name), kind=kind)
    code, lohi = _range_device(x.reshape(N, C, H * W))
    assert code == 0 and np.array_equal(lohi, _host_range(x.reshape(N, C, H * W))[1])
    assert np.array_equal(lohi, ref.image_range(x))
    launches = _lib.lib().egn_launch_count()
    for extra in (0, 5):                                             # 5: rows that start on no dword boundary
        for what, got, want, width in _compose_both(x, m, lohi, nrow, extra):
            assert np.array_equal(got[:, :width], want[:, :width]), (what, extra, int((got != want).sum()))
            assert (got[:, width:] == PAD).all(), (what, extra)      # the padding bytes are untouched
            assert (want[:, :width] != PAD).any()
    assert _lib.lib().egn_launch_count() - launches == 4             # one launch per picture


def test_side_stream_beside_a_busy_default_stream():
    name, N, C, H, W, nrow, n, J, h, w, kind = ref.CASES[1]
    x, m = ref.build_case(N, C, H, W, n, J, h, w, seed=3)
    lohi = ref.image_range(x)
    a = torch.empty(16 << 20, device='cuda').normal_()
    b = torch.empty_like(a)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(4):
        b.copy_(a)
    with torch.cuda.stream(side):
        res = _compose_both(x, m, lohi, nrow, 3)
        code, got_lohi = _range_device(x.reshape(N, C, H * W))
    torch.cuda.synchronize()
    assert code == 0 and np.array_equal(got_lohi, lohi)
    for what, got, want, width in res:
        assert np.array_equal(got, want), what


@pytest.mark.parametrize('hw', [1, 63, 64, 8200, 64 * 1000 + 7])
def test_range_equals_numpys_nan_ignoring_min_max_exactly(hw):
    rs = np.random.RandomState(hw)
    x = rs.randn(2, 5, hw).astype(np.float32)
    x[:, 3], x[:, 4] = 1e6, -1e6                                     # planes 3 and 4 do not count
    nan = rs.rand(2, 5, hw) < 0.1
    x[nan] = np.nan
    want = np.zeros(2, dtype=np.float32) if np.isnan(x[:, :3]).all() else \
        np.array([np.nanmin(x[:, :3]), np.nanmax(x[:, :3])], dtype=np.float32)
    for offset in (0, 1):                                            # 1: hw % 4 == 0 without the alignment
        code, lohi = _range_device(x, offset=offset)
        assert code == 0 and np.array_equal(lohi, want), (hw, offset)
    assert np.array_equal(_host_range(x)[1], want)
    # a chunk, and a whole picture, of NaNs: its partial folds as "nothing seen"
    x[0, 0, :min(hw, 4096)] = np.nan
    want = np.array([np.nanmin(x[:, :3]), np.nanmax(x[:, :3])], dtype=np.float32) if hw > 1 else want
    code, lohi = _range_device(x)
    assert code == 0 and np.array_equal(lohi, _host_range(x)[1]) and (hw == 1 or np.array_equal(lohi, want))
    code, lohi = _range_device(np.full((1, 3, hw), np.nan, dtype=np.float32))
    assert code == 0 and tuple(lohi) == (0.0, 0.0)


def test_bad_arguments_leave_the_buffer_alone_and_zero_counts_are_no_ops():
    L = _lib.lib()
    x, m = ref.build_case(2, 3, 4, 4, 2, 2, 2, 2, seed=1)
    d_x, d_m, d_lohi, d_lut = _dev(x), _dev(m), _dev(ref.image_range(x)), _dev(dbg.jet_lut())
    buf = torch.full((4096,), PAD, dtype=torch.uint8, device='cuda')
    st = _lib.current_stream()
    launches = L.egn_launch_count()

    def untouched():
        torch.cuda.synchronize()
        return bool((buf == PAD).all())
    a = (_lib.ptr(d_x), 2, 3, 4, 4, 8, 2, _lib.ptr(d_lohi), _lib.ptr(buf), 3 * 14, st)
    for i, v in ((1, -1), (2, 2), (3, -4), (5, 0), (6, -1), (9, 3 * 14 - 1), (0, None), (7, None), (8, None),
                 (3, 0x7fffffff)):
        b = list(a)
        b[i] = v
        assert L.egn_debug_grid_u8(*b) == -1 and untouched(), (i, v)
    for i in (1, 3, 4):
        b = list(a)
        b[i] = 0
        assert L.egn_debug_grid_u8(*b) == 0 and untouched()
    a = (_lib.ptr(d_x), 3, 4, 4, _lib.ptr(d_m), 2, 2, 2, 2, _lib.ptr(d_lohi), _lib.ptr(d_lut), _lib.ptr(buf), 18, st)
    for i, v in ((1, 2), (2, 0), (5, -1), (6, -1), (7, -2), (12, 17), (0, None), (4, None), (9, None), (10, None),
                 (11, None), (8, 0x7fffffff)):
        b = list(a)
        b[i] = v
        assert L.egn_debug_mosaic_u8(*b) == -1 and untouched(), (i, v)
    for i in (5, 7, 8):
        b = list(a)
        b[i] = 0
        assert L.egn_debug_mosaic_u8(*b) == 0 and untouched()
    lohi = torch.full((2,), 77.0, dtype=torch.float32, device='cuda')
    ws = torch.empty(64, dtype=torch.uint8, device='cuda')
    r = (_lib.ptr(d_x), 2, 3, 3, 16, _lib.ptr(ws), 64, _lib.ptr(lohi), st)
    for i, v in ((1, -1), (3, 4), (4, -1), (0, None), (5, None), (7, None), (6, 47)):      # 2 x 3 partials need 48 bytes
        b = list(r)
        b[i] = v
        assert L.egn_debug_range_f32(*b) == -1, (i, v)
    for i in (1, 3, 4):
        b = list(r)
        b[i] = 0
        assert L.egn_debug_range_f32(*b) == 0
    torch.cuda.synchronize()
    assert lohi.tolist() == [77.0, 77.0]
    assert L.egn_launch_count() == launches                          # nothing of all this was launched
    assert L.egn_debug_range_f32(*r) == 0 and L.egn_launch_count() - launches == 2
    torch.cuda.synchronize()
    assert np.array_equal(lohi.cpu().numpy(), ref.image_range(x))


def test_python_entries_on_cuda_tensors_equal_the_host_path(monkeypatch, tmp_path):
    """``save_batch_image_with_joints`` / ``save_batch_heatmaps`` with CUDA tensors (a channel slice read in place)
    hand the encoder the arrays the same calls with numpy arrays hand it."""
    x, m = ref.build_case(9, 5, 16, 24, 7, 3, 4, 6, seed=4)          # nine crops: two grid rows
    rs = np.random.RandomState(0)
    pred, gt = rs.uniform(-3, 27, (9, 3, 2)).astype(np.float32), rs.uniform(0, 24, (7, 3, 3))
    handed = []
    monkeypatch.setattr(dbg, '_encode_jpeg', lambda path, a, q=95: handed.append(a.copy()))
    d_x = _dev(x)
    launches = _lib.lib().egn_launch_count()
    dbg.save_batch_image_with_joints(d_x[:, :3], {'pred': (_dev(pred), None), 'gt': (gt, None)}, 'a.jpg')
    assert _lib.lib().egn_launch_count() - launches == 4             # range (2), grid, overlay
    dbg.save_batch_heatmaps(d_x[:, :3], _dev(m), 'b.jpg')
    dbg.save_batch_image_with_joints(x[:, :3], {'pred': (pred, None), 'gt': (gt, None)}, 'a.jpg')
    dbg.save_batch_heatmaps(x[:, :3], m, 'b.jpg')
    assert handed[0].shape == (2 * 18 + 2, 8 * 26 + 2, 3) and handed[1].shape == (7 * 4, 4 * 6, 3)
    assert np.array_equal(handed[0], handed[2]) and np.array_equal(handed[1], handed[3])
    assert (handed[0] == (0, 255, 255)).all(-1).any() and (handed[1] == (255, 0, 0)).all(-1).any()


class _CropSet(torch.utils.data.Dataset):
    def __init__(self, n=4):
        g = torch.Generator().manual_seed(1)
        self.x = synth.synth_crops(n, 3, 64, 64, seed=3)
        self.t = torch.rand(n, 5, 16, 16, generator=g)
        self.j = torch.rand(n, 5, 3, generator=g) * 64

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.t[i], torch.ones(5, 1), {'transformed_joints': self.j[i].numpy()}


def _run(head, out_dir, save_debug, monkeypatch):
    """Two native steps of the tiny HRNet (report_every = 1) -> (losses, launches of the run, launches inside
    save_debug_images, [(the call's tensors on the host)], {file name: array handed to the encoder}); ``losses`` is
    the pair (reported losses, the weights and buffers after the two steps)."""
    L = _lib.lib()
    cfg = configs.clone(configs.tiny_config(head))
    cfg.update(use_gpu=True, exp_type='instanceto2d', dirs={'output': str(out_dir)},
               optimizer={'optim_type': 'adam', 'lr': 1e-3, 'weight_decay': 0.0, 'momentum': 0.9, 'milestones': [3],
                          'gamma': 0.5},
               training_settings={'total_epochs': 1, 'batch_size': 2, 'num_threads': 0, 'shuffle': False,
                                  'report_every': 1, 'eval_during': False, 'plot_loss': False,
                                  'debug': {'save': True, 'save_images_kpts': True, 'save_hms_gt': True,
                                            'save_hms_pred': True}})
    net = hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=9))
    net = net.cuda()
    optim, sche = trainer.prepare_optim(net, cfg)
    calls, handed, inside = [], {}, [0]
    real_save, real_encode = dbg.save_debug_images, dbg._encode_jpeg

    def save(epoch, batch, cfgs, data, meta, target, others, output, split, writer=None):
        torch.cuda.synchronize()
        host_out = tuple(o.detach().cpu().clone() for o in output) if type(output) is tuple else output.detach().cpu().clone()
        calls.append((epoch, batch, data.cpu().clone(), meta, target.cpu().clone(), host_out, split))
        c0 = L.egn_launch_count()
        real_save(epoch, batch, cfgs, data, meta, target, others, output, split, writer=writer)
        inside[0] += L.egn_launch_count() - c0

    def encode(path, a, q=95):
        handed[os.path.basename(path)] = a.copy()
        real_encode(path, a, q)
    monkeypatch.setattr(trainer.debug_pictures, 'save_debug_images', save)
    monkeypatch.setattr(dbg, '_encode_jpeg', encode)
    lg = logging.getLogger('egonet_amd.test_gpu_debug_pictures')
    lg.handlers = [logging.NullHandler()]
    lg.propagate = False
    torch.cuda.synchronize()
    c0, d0 = L.egn_launch_count(), L.egn_direct_conv_count()
    rec = trainer.train(_CropSet(), net, None, optim, sche, cfg, lg, save_debug=save_debug)
    torch.cuda.synchronize()
    monkeypatch.setattr(trainer.debug_pictures, 'save_debug_images', real_save)
    state = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    return (rec['loss'], state), (L.egn_launch_count() - c0, L.egn_direct_conv_count() - d0), inside[0], calls, handed, cfg


@pytest.mark.parametrize('head', ['coordinates', 'heatmap'])
def test_train_with_save_debug_writes_the_pictures_and_leaves_the_step_alone(head, tmp_path, monkeypatch):
    Image = pytest.importorskip('PIL.Image')
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    (loss_on, state_on), (launch_on, conv_on), inside, calls, handed, cfg = _run(head, tmp_path / 'on', True, monkeypatch)
    folder = tmp_path / 'on' / 'intermediate_results' / 'train'
    names = sorted('1_%d_%s.jpg' % (b, k) for b in (0, 1) for k in ('keypoints', 'hm_gt', 'hm_pred'))
    assert sorted(os.listdir(str(folder))) == names and sorted(handed) == names      # after close(): all six, no .tmp
    assert Image.open(str(folder / '1_1_keypoints.jpg')).size == (2 * 66 + 2, 66 + 2)
    assert Image.open(str(folder / '1_0_hm_pred.jpg')).size == (6 * 16, 2 * 16)
    assert [(c[0], c[1], c[6]) for c in calls] == [(1, 0, 'train'), (1, 1, 'train')]
    # the device route hands the encoder what the host twin makes of the same tensors
    device_arrays = dict(handed)
    for epoch, batch, data, meta, target, output, split in calls:
        handed.clear()
        dbg.save_debug_images(epoch, batch, cfg, data, meta, target, None, output, split)
        assert len(handed) == 3
        for name, want in handed.items():
            assert np.array_equal(device_arrays[name], want), (name, int((device_arrays[name] != want).sum()))
            assert len(np.unique(want)) > 20
    assert (device_arrays['1_0_keypoints.jpg'] == (0, 255, 255)).all(-1).any()
    # pictures off: the same losses, and the same launches apart from those issued inside save_debug_images
    (loss_off, state_off), (launch_off, conv_off), inside_off, calls_off, handed_off, _ = _run(head, tmp_path / 'off',
                                                                                              False, monkeypatch)
    # the step itself: every weight and buffer after the two steps is bit-identical.  The reported loss is a float64
    # sum the step's kernels build with one atomicAdd per wavefront (csrc/train_ops.hip mse_kernel), so its last bits
    # depend on the order the waves arrive in, run by run, pictures or not: two orderings of K non-negative terms
    # differ by at most 2 (K - 1) 2^-53 of the sum; K <= one wave per 64 map elements plus the coordinate term's
    print('losses on %r off %r' % (loss_on, loss_off))
    assert list(state_on) == list(state_off) and all(torch.equal(state_on[k], state_off[k]) for k in state_on)
    waves = 2 * 5 * 16 * 16 // 64 + 8
    assert len(loss_on) == len(loss_off) == 2
    assert all(abs(a - b) <= 2 * waves * 2.0 ** -53 * abs(b) for a, b in zip(loss_on, loss_off))
    assert calls_off == [] and handed_off == {} and not (tmp_path / 'off').exists()
    print('launches on %d (of which pictures %d), off %d' % (launch_on, inside, launch_off))
    assert inside >= 2 * (2 + 3 + 1) and launch_on - inside == launch_off and conv_on == conv_off
