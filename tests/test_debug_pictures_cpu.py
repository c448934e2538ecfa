"""The training debug pictures without a GPU: the host twins of csrc/debug_pictures.hip against the numpy restatement
of the definition (byte for byte), the colour table, the grid layout, the seven-segment digits, ``save_debug_images``
on CPU tensors and the trainer's wiring with a stub step."""
import logging
import os

import numpy as np
import pytest
import torch

import debug_pictures_ref as ref
from egonet_amd import _lib, trainer
from egonet_amd.train_hrnet import HRNetTrainStep
from egonet_amd.visualization import OverlayRenderer
from egonet_amd.visualization import debug as dbg


def _host_range(x, c_used=3):
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, c = x.shape[:2]
    lohi = np.full(2, 77.0, dtype=np.float32)
    code = _lib.lib().egn_debug_range_host_f32(x.ctypes.data, n, c, c_used, int(np.prod(x.shape[2:])), lohi.ctypes.data)
    return code, lohi


def _host_grid(x, lohi, nrow, pad=2, extra=0):
    N, C, H, W = x.shape
    _, _, gh, gw = dbg.grid_layout(N, H, W, nrow, pad)
    buf = np.full((gh, 3 * gw + extra), 0xA5, dtype=np.uint8)
    code = _lib.lib().egn_debug_grid_host_u8(x.ctypes.data, N, C, H, W, nrow, pad, lohi.ctypes.data, buf.ctypes.data,
                                             buf.strides[0])
    return code, buf


def _host_mosaic(x, m, lohi, lut, extra=0):
    n, J, h, w = m.shape
    buf = np.full((n * h, 3 * (J + 1) * w + extra), 0xA5, dtype=np.uint8)
    code = _lib.lib().egn_debug_mosaic_host_u8(x.ctypes.data, x.shape[1], x.shape[2], x.shape[3], m.ctypes.data, n, J, h,
                                               w, lohi.ctypes.data, lut.ctypes.data, buf.ctypes.data, buf.strides[0])
    return code, buf


@pytest.mark.parametrize('case', ref.CASES, ids=[c[0] for c in ref.CASES])
def test_host_twins_equal_the_numpy_restatement_byte_for_byte(case):
    name, N, C, H, W, nrow, n, J, h, w, kind = case
    x, m = ref.build_case(N, C, H, W, n, J, h, w, seed=len(name), kind=kind)
    lut = dbg.jet_lut()
    code, lohi = _host_range(x)
    want_lohi = ref.image_range(x)
    assert code == 0 and np.array_equal(lohi, want_lohi)
    for extra in (0, 7):
        code, buf = _host_grid(x, lohi, nrow, extra=extra)
        gw = buf.shape[1] - extra
        assert code == 0 and np.array_equal(buf[:, :gw].reshape(buf.shape[0], -1, 3), ref.grid(x, lohi, nrow))
        assert (buf[:, gw:] == 0xA5).all()
        code, buf = _host_mosaic(x, m, lohi, lut, extra=extra)
        mw = buf.shape[1] - extra
        assert code == 0 and np.array_equal(buf[:, :mw].reshape(n * h, -1, 3), ref.mosaic(x, m, lohi, lut))
        assert (buf[:, mw:] == 0xA5).all()
    if kind == 'normal':
        assert len(np.unique(ref.grid(x, lohi, nrow))) >= min(30, x[:, :3].size // 2)     # the grey levels are spread


def test_range_ignores_nans_and_folds_signed_zeros():
    for vals, want in (([np.nan, 2.0, -3.0, np.nan], (-3.0, 2.0)), ([np.nan] * 4, (0.0, 0.0)), ([-0.0] * 4, (0.0, 0.0)),
                       ([np.inf, 1.0, -np.inf, 0.0], (-np.inf, np.inf))):
        x = np.zeros((1, 4, 1, 4), dtype=np.float32)
        x[0, :3] = np.asarray(vals, dtype=np.float32)
        x[0, 3] = 1e9                                               # the fourth plane is not the picture's
        code, lohi = _host_range(x)
        assert code == 0 and tuple(lohi) == want and not np.signbit(lohi[lohi == 0]).any(), vals
    code, lohi = _host_range(np.zeros((0, 3, 2, 2), dtype=np.float32))
    assert code == 0 and tuple(lohi) == (77.0, 77.0)                # nothing to fold: lohi is left alone
    assert _lib.lib().egn_debug_range_host_f32(None, 1, 2, 3, 4, lohi.ctypes.data) == -1      # c_used > c
    assert _lib.lib().egn_debug_range_host_f32(None, -1, 3, 3, 4, lohi.ctypes.data) == -1
    assert _lib.lib().egn_debug_range_ws_bytes(24, 3, 256 * 256) == 24 * 3 * 16 * 8
    assert _lib.lib().egn_debug_range_ws_bytes(-1, 3, 4) == -1


def test_quantiser_and_thumbnail_by_hand():
    # lo = 0, hi = 1: v = x / 1.00001; 0.5 -> trunc(127.49...) = 127, 1 -> trunc(254.997) = 254, above -> 255
    x = np.zeros((1, 3, 4, 4), dtype=np.float32)
    x[0, :, 1:3, 1:3] = np.array([[0.5, 1.0], [0.0, 1.0]], dtype=np.float32)
    lohi = np.array([0.0, 1.0], dtype=np.float32)
    code, g = _host_grid(x, lohi, 8)
    assert code == 0 and g.shape == (8, 24)
    centre = g.reshape(8, 8, 3)[3:5, 3:5, 0]
    assert centre.tolist() == [[127, 254], [0, 254]]
    # 4:1 thumbnail = the mean of the 2 x 2 centre pixels, rounded half up: (127 + 254 + 0 + 254) / 4 = 158.75 -> 159
    m = np.zeros((1, 1, 1, 1), dtype=np.float32)
    code, mo = _host_mosaic(x, m, lohi, dbg.jet_lut())
    assert code == 0 and mo.reshape(1, 2, 3)[0, 0].tolist() == [159, 159, 159]
    assert mo.reshape(1, 2, 3)[0, 1].tolist() == [(3 * 159) // 10, (3 * 159) // 10, (7 * 128 + 3 * 159) // 10]


def test_bad_arguments_leave_the_buffer_alone_and_zero_counts_are_no_ops():
    x, m = ref.build_case(2, 3, 4, 4, 2, 2, 2, 2, seed=1)
    lohi, lut, L = ref.image_range(x), dbg.jet_lut(), _lib.lib()
    buf = np.full(4096, 0xA5, dtype=np.uint8)
    a = (x.ctypes.data, 2, 3, 4, 4, 8, 2, lohi.ctypes.data, buf.ctypes.data, 3 * 14)
    for i, v in ((1, -1), (2, 2), (3, -4), (5, 0), (6, -1), (9, 3 * 14 - 1), (0, None), (7, None), (8, None),
                 (3, 0x7fffffff)):
        b = list(a)
        b[i] = v
        assert L.egn_debug_grid_host_u8(*b) == -1 and (buf == 0xA5).all(), (i, v)
    for i in (1, 3, 4):
        b = list(a)
        b[i] = 0
        assert L.egn_debug_grid_host_u8(*b) == 0 and (buf == 0xA5).all()
    a = (x.ctypes.data, 3, 4, 4, m.ctypes.data, 2, 2, 2, 2, lohi.ctypes.data, lut.ctypes.data, buf.ctypes.data, 18)
    for i, v in ((1, 2), (2, 0), (5, -1), (6, -1), (7, -2), (12, 17), (0, None), (4, None), (9, None), (10, None),
                 (11, None), (8, 0x7fffffff)):
        b = list(a)
        b[i] = v
        assert L.egn_debug_mosaic_host_u8(*b) == -1 and (buf == 0xA5).all(), (i, v)
    for i in (5, 7, 8):
        b = list(a)
        b[i] = 0
        assert L.egn_debug_mosaic_host_u8(*b) == 0 and (buf == 0xA5).all()


def test_jet_lut_end_points_and_piecewise_monotone_channels():
    lut = dbg.jet_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8 and np.array_equal(lut, ref.jet_lut())
    assert tuple(lut[0]) == (0, 0, 128) and tuple(lut[255]) == (128, 0, 0)
    for ch in range(3):
        d = np.diff(lut[:, ch].astype(int))
        peak = int(np.argmax(lut[:, ch]))
        last_peak = 255 - int(np.argmax(lut[::-1, ch]))
        assert (d[:peak] >= 0).all() and (d[last_peak:] <= 0).all() and lut[:, ch].max() == 255      # up, flat, down
    assert int(np.argmax(lut[:, 2])) < int(np.argmax(lut[:, 1])) < int(np.argmax(lut[:, 0]))           # blue, green, red


@pytest.mark.parametrize('n,want', [(1, (1, 1, 20, 28)), (3, (3, 1, 20, 80)), (8, (8, 1, 20, 210)),
                                    (9, (8, 2, 38, 210))])
def test_grid_layout_numbers(n, want):
    assert dbg.grid_layout(n, 16, 24) == want
    x = np.zeros((n, 3, 16, 24), dtype=np.float32)
    code, buf = _host_grid(x, np.zeros(2, dtype=np.float32), 8)
    assert code == 0 and buf.shape == (want[2], 3 * want[3])


def test_digits_1_to_33_have_the_seven_segment_counts():
    counts = {0: 6, 1: 2, 2: 5, 3: 5, 4: 4, 5: 5, 6: 6, 7: 3, 8: 7, 9: 6}
    assert {d: len(s) for d, s in dbg.DIGIT_SEGMENTS.items()} == counts
    for number in range(1, 34):
        prims, cols = dbg.build_digit_primitives(number, 10.0, 40.0, 8.0, (0, 255, 255))
        digits = [int(c) for c in str(number)]
        assert len(prims) == sum(counts[d] for d in digits) == len(cols)
        assert prims.dtype == np.float32 and (cols == (255 << 8 | 255 << 16)).all()
        at = 0
        for i, d in enumerate(digits):                               # each digit inside its own cell
            p = prims[at:at + counts[d]]
            at += counts[d]
            assert p[:, [0, 2]].min() >= 10.0 + 6.0 * i and p[:, [0, 2]].max() <= 10.0 + 6.0 * i + 4.0
            assert p[:, [1, 3]].min() >= 32.0 and p[:, [1, 3]].max() <= 40.0
            assert (p[:, 4] == 0.5).all() and (p[:, 5] == 1.0).all()
    one, _ = dbg.build_digit_primitives(1, 0.0, 8.0, 8.0, 'r')       # the right-hand side, top to bottom
    assert one.tolist() == [[4.0, 0.0, 4.0, 4.0, 0.5, 1.0], [4.0, 4.0, 4.0, 8.0, 0.5, 1.0]]


def _cfgs(out, head='coordinates', **debug):
    d = dict(save=True, save_images_kpts=True, save_hms_gt=True, save_hms_pred=True)
    d.update(debug)
    return {'dirs': {'output': str(out)}, 'heatmapModel': {'input_size': [24, 16], 'head_type': head},
            'training_settings': {'debug': d}}


def _batch(N=3, n=2, J=4, seed=0):
    rs = np.random.RandomState(seed)
    data = torch.from_numpy(rs.randn(N, 3, 16, 24).astype(np.float32))
    target = torch.from_numpy(rs.uniform(0, 1, (n, J, 4, 6)).astype(np.float32))
    maps = torch.from_numpy(rs.uniform(-0.1, 1, (N, J, 4, 6)).astype(np.float32))
    coords = torch.from_numpy(rs.uniform(0.1, 0.9, (N, J, 2)).astype(np.float32))
    meta = {'transformed_joints': rs.uniform(2, 14, (n, J, 3)), 'joints_vis': np.ones((n, J))}
    return data, target, maps, coords, meta


NAMES = ['5_30_hm_gt.jpg', '5_30_hm_pred.jpg', '5_30_keypoints.jpg']


def test_save_debug_images_writes_the_reference_files_with_the_defined_sizes(tmp_path, monkeypatch):
    Image = pytest.importorskip('PIL.Image')
    data, target, maps, coords, meta = _batch()
    handed = {}
    encode = dbg._encode_jpeg
    monkeypatch.setattr(dbg, '_encode_jpeg', lambda path, a, q=95: (handed.__setitem__(os.path.basename(path), a.copy()),
                                                                   encode(path, a, q)))
    dbg.save_debug_images(5, 30, _cfgs(tmp_path), data, meta, target, None, (maps, coords), 'train')
    folder = tmp_path / 'intermediate_results' / 'train'
    assert sorted(os.listdir(str(folder))) == NAMES
    sizes = {n: Image.open(str(folder / n)).size for n in NAMES}
    # the mixed batch: N = 3 crops in the grid and the predicted mosaic, n = 2 rows in the target mosaic
    assert sizes == {'5_30_keypoints.jpg': (3 * 26 + 2, 18 + 2), '5_30_hm_gt.jpg': (5 * 6, 2 * 4),
                     '5_30_hm_pred.jpg': (5 * 6, 3 * 4)}
    assert all(Image.open(str(folder / n)).mode == 'RGB' for n in NAMES)
    # what was handed to the encoder: the definition's composition, then the markers by the host overlay twin
    x = data.numpy()
    lohi, lut, host = ref.image_range(x), ref.jet_lut(), OverlayRenderer('cpu')
    for name, m in (('5_30_hm_gt.jpg', target.numpy()), ('5_30_hm_pred.jpg', maps.numpy())):
        plain = ref.mosaic(x, m, lohi, lut)
        p, c = dbg.build_mosaic_markers(dbg.max_preds_host(m), 4, 6)
        assert len(p) == 2 * m.shape[0] * 4
        want = host.draw([plain], p, c, [(0, len(p))])[0]
        assert np.array_equal(handed[name], want) and (want != plain).any()
    plain = ref.grid(x, lohi)
    pred = coords.numpy() * np.array([24.0, 16.0], dtype=np.float32)
    parts = [dbg.build_grid_markers(pred, 3, 16, 24, colour=dbg.RED),
             dbg.build_grid_markers(meta['transformed_joints'], 3, 16, 24, colour=dbg.CYAN)]
    assert len(parts[0][0]) == 3 * (4 + 16) and len(parts[1][0]) == 2 * (4 + 16)      # digits 1..4: 2 + 5 + 5 + 4
    p, c = np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
    want = host.draw([plain], p, c, [(0, len(p))])[0]
    assert np.array_equal(handed['5_30_keypoints.jpg'], want)
    third = want[:, 2 + 2 * 26:2 + 2 * 26 + 24]                     # the unlabelled crop's cell: no cyan centre
    cyan, red = (want == (0, 255, 255)).all(-1), (want == (255, 0, 0)).all(-1)
    assert cyan[:, :2 + 2 * 26].any() and red.any() and not (third == (0, 255, 255)).all(-1)[4:, :12].any()
    # the first ground-truth disc sits at the truncated position
    gx, gy = int(2 + meta['transformed_joints'][0, 0, 0]), int(2 + meta['transformed_joints'][0, 0, 1])
    assert p[len(parts[0][0])].tolist() == [gx, gy, gx, gy, 3.0, 1.0]


@pytest.mark.parametrize('head', ['coordinates', 'heatmap'])
def test_others_none_and_others_with_joints_for_both_heads(tmp_path, monkeypatch, head):
    pytest.importorskip('PIL.Image')
    data, target, maps, coords, meta = _batch(N=2, n=2)
    output = (maps, coords) if head == 'coordinates' else maps
    handed = []
    monkeypatch.setattr(dbg, '_encode_jpeg', lambda path, a, q=95: handed.append((os.path.basename(path), a.copy())))
    cfgs = _cfgs(tmp_path, head, save_hms_gt=False, save_hms_pred=False)
    dbg.save_debug_images(1, 0, cfgs, data, meta, target, None, output, 'train')
    if head == 'coordinates':
        joints = coords.numpy() * np.array([24.0, 16.0], dtype=np.float32)
    else:
        joints = dbg.max_preds_host(maps.numpy()) * np.array([4.0, 4.0], dtype=np.float32)
    assert np.array_equal(dbg.decode_joints_pred(output, [24, 16]), joints)
    dbg.save_debug_images(1, 0, cfgs, data, meta, target, {'joints_pred': joints}, output, 'train')
    dbg.save_debug_images(1, 0, cfgs, data, meta, target, {'src_coord': None}, output, 'train')
    assert [n for n, _ in handed] == ['1_0_keypoints.jpg'] * 3
    assert np.array_equal(handed[0][1], handed[1][1]) and np.array_equal(handed[0][1], handed[2][1])
    assert (handed[0][1] == (255, 0, 0)).all(-1).any()


def test_each_key_gates_its_file(tmp_path):
    pytest.importorskip('PIL.Image')
    data, target, maps, coords, meta = _batch()
    for k, key in enumerate(('save_hms_gt', 'save_hms_pred', 'save_images_kpts')):
        out = tmp_path / key
        dbg.save_debug_images(5, 30, _cfgs(out, **{key: False}), data, meta, target, None, (maps, coords), 'validation')
        assert sorted(os.listdir(str(out / 'intermediate_results' / 'validation'))) == NAMES[:k] + NAMES[k + 1:]
    dbg.save_debug_images(5, 30, _cfgs(tmp_path / 'off', save=False), data, meta, target, None, (maps, coords), 'train')
    assert not (tmp_path / 'off').exists()


def test_writer_keeps_one_report_in_flight_and_raises_what_the_encoder_raised(tmp_path, monkeypatch):
    import threading
    gate, order = threading.Event(), []

    def slow(path, a, q=95):
        gate.wait(10)
        order.append(os.path.basename(path))
        if 'bad' in path:
            raise OSError('disk full')
    monkeypatch.setattr(dbg, '_encode_jpeg', slow)
    w = dbg.DebugPictureWriter()
    pic = np.zeros((2, 2, 3), dtype=np.uint8)
    w.write_host([('a1', pic), ('a2', pic)])                          # returns at once: the worker waits at the gate
    assert order == []
    t = threading.Timer(0.05, gate.set)
    t.start()
    w.write_host([('b1', pic)])                                       # waits for the first report, drops nothing
    assert order[:2] == ['a1', 'a2']
    w.flush()
    assert order == ['a1', 'a2', 'b1'] and w.reports == 2
    w.write_host([('bad', pic)])
    with pytest.raises(OSError):
        w.flush()
    w.close()
    w.close()
    with pytest.raises(RuntimeError):
        w.write_host([('c', pic)])


class _StubStep(HRNetTrainStep):
    """What trainer.train reads of a key-point step, without a GPU."""

    def __init__(self, fail_at=None):
        self.dev, self.angle_crit, self.w_coor, self.use_target_weight = torch.device('cpu'), None, 0.0, False
        self.lr, self.apply_cr_loss, self.calls, self.fail_at = 1e-3, False, 0, fail_at
        self.last_maps = self.last_coords = None

    def step(self, data, target, joints=None, target_weight=None):
        if self.calls == self.fail_at:
            raise FloatingPointError('stub')
        self.calls += 1
        self.last_maps = torch.zeros(len(data), 2, 4, 4)
        return torch.tensor([0.5])


class _Set(torch.utils.data.Dataset):
    num_joints = 2

    def __len__(self):
        return 14

    def __getitem__(self, i):
        return torch.zeros(3, 8, 8), torch.zeros(2, 4, 4), torch.ones(2, 1), {'transformed_joints': np.zeros((2, 3))}


class _Writer(object):
    made = []

    def __init__(self):
        self.closed = 0
        _Writer.made.append(self)

    def close(self):
        self.closed += 1


def _train(monkeypatch, save_debug, fail_at=None):
    calls = []
    _Writer.made = []
    step = _StubStep(fail_at)
    monkeypatch.setattr(trainer, 'make_step', lambda *a, **k: step)
    monkeypatch.setattr(trainer.debug_pictures, 'DebugPictureWriter', _Writer)
    monkeypatch.setattr(trainer.debug_pictures, 'save_debug_images',
                        lambda epoch, batch, cfgs, data, meta, target, others, output, split, writer=None:
                        calls.append((epoch, batch, tuple(data.shape), tuple(target.shape), others, output is step.last_maps,
                                      split, writer)))
    cfgs = {'training_settings': {'total_epochs': 2, 'report_every': 3, 'batch_size': 2, 'num_threads': 0,
                                  'shuffle': False}}
    lg = logging.getLogger('egonet_amd.test_debug_pictures')
    lg.handlers = [logging.NullHandler()]
    lg.propagate = False
    model = torch.nn.Linear(1, 1)
    trainer.train(_Set(), model, None, None, None, cfgs, lg, save_debug=save_debug)
    return calls


def test_trainer_calls_the_writer_on_report_batches_only_and_closes_it(monkeypatch):
    calls = _train(monkeypatch, True)
    w, = _Writer.made
    assert w.closed == 1
    assert [(c[0], c[1]) for c in calls] == [(e, b) for e in (1, 2) for b in (0, 3, 6)]       # 7 batches, report every 3
    assert all(c[2:] == ((2, 3, 8, 8), (2, 2, 4, 4), None, True, 'train', w) for c in calls)


def test_trainer_closes_the_writer_on_an_exception(monkeypatch):
    with pytest.raises(FloatingPointError):
        _train(monkeypatch, True, fail_at=4)
    w, = _Writer.made
    assert w.closed == 1


def test_trainer_never_constructs_a_writer_with_save_debug_off(monkeypatch):
    assert _train(monkeypatch, False) == [] and _Writer.made == []


class _EvalModel(torch.nn.Module):
    def forward(self, data):
        return torch.zeros(len(data), 2, 4, 4), torch.full((len(data), 2, 2), 0.5)


def _evaluate(monkeypatch, exp_type, save_debug):
    calls = []
    _Writer.made = []
    monkeypatch.setattr(trainer.debug_pictures, 'DebugPictureWriter', _Writer)
    monkeypatch.setattr(trainer.debug_pictures, 'save_debug_images',
                        lambda epoch, batch, cfgs, data, meta, target, others, output, split, writer=None:
                        calls.append((epoch, batch, len(data), others, type(output) is tuple, split, writer)))
    cfgs = {'use_gpu': False, 'exp_type': exp_type,
            'testing_settings': {'batch_size': 4, 'num_threads': 0, 'shuffle': False, 'save_debug': save_debug}}
    lg = logging.getLogger('egonet_amd.test_debug_pictures')
    lg.handlers = [logging.NullHandler()]
    lg.propagate = False
    trainer.evaluate(_Set(), _EvalModel(), None, cfgs, lg, None)
    return calls


def test_evaluate_honours_testing_settings_save_debug_for_the_key_point_model(monkeypatch):
    calls = _evaluate(monkeypatch, 'instanceto2d', True)
    w, = _Writer.made
    assert w.closed == 1                                             # 14 samples in batches of 4: epoch 0, 'validation'
    assert calls == [(0, b, n, None, True, 'validation', w) for b, n in enumerate((4, 4, 4, 2))]
    assert _evaluate(monkeypatch, 'baselinealpha', True) == [] and _Writer.made == []
    assert _evaluate(monkeypatch, 'instanceto2d', False) == [] and _Writer.made == []
