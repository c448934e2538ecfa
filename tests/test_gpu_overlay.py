"""The overlay rasteriser on the GPU (csrc/overlay.hip): the kernel gives the bytes of the host twin -- with and without
its tile binning --, keeps painter's order across the chunks of its LDS list, draws in place on a side stream, and
carries ``EgoNet.post_process(visualize=True)`` and ``tools/inference_kitti.py --draw``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))

import overlay_ref as orf                                            # noqa: E402
from egonet_amd import _lib, configs, synth                          # noqa: E402
from egonet_amd.model.egonet import EgoNet                           # noqa: E402
from egonet_amd.visualization import OverlayRenderer, build_bev_primitives, build_primitives   # noqa: E402

pytestmark = pytest.mark.gpu


def _device(buf, tab, prims, colors, antialias=1, cull=1, n_frames=None, n_prims=None, max_hw=None, base=True):
    """egn_overlay_draw_u8 on a device copy of ``buf`` -> (return code, the buffer read back)."""
    d_buf = torch.from_numpy(np.array(buf, dtype=np.uint8, copy=True)).cuda()
    d_tab = torch.from_numpy(np.ascontiguousarray(tab, dtype=np.int64)).cuda()
    d_pr = torch.from_numpy(np.ascontiguousarray(prims, dtype=np.float32)).cuda()
    d_col = torch.from_numpy(np.ascontiguousarray(colors, dtype=np.uint32).view(np.int32)).cuda()
    mh, mw = (int(tab[:, 1].max()), int(tab[:, 2].max())) if max_hw is None else max_hw
    code = _lib.lib().egn_overlay_draw_u8(
        _lib.ptr(d_buf) if base else None, _lib.ptr(d_tab), len(tab) if n_frames is None else n_frames, mh, mw,
        _lib.ptr(d_pr), _lib.ptr(d_col), len(colors) if n_prims is None else n_prims, antialias, cull,
        _lib.current_stream())
    torch.cuda.synchronize()
    return code, d_buf.cpu().numpy()


@pytest.mark.parametrize('antialias', [1, 0])
@pytest.mark.parametrize('name,sizes,seed,strides,empty', orf.CASES, ids=[c[0] for c in orf.CASES])
def test_device_equals_host_twin_with_and_without_culling(name, sizes, seed, strides, empty, antialias):
    frames, buf, tab, prims, colors = orf.build_case(sizes, seed, strides, empty)
    code, want = orf.host_twin(buf, tab, prims, colors, antialias)
    assert code == 0 and (want != buf).any()
    for cull in (1, 0):
        code, got = _device(buf, tab, prims, colors, antialias, cull)
        assert code == 0
        assert np.array_equal(got, want), (name, cull, int((got != want).sum()))
    got_frames, pad = orf.unpack(got, tab)
    assert (pad == 0xA5).all()                                       # padding bytes of wide strides are untouched
    for i in empty:
        assert np.array_equal(got_frames[i], frames[i])              # an empty primitive range: bit-identical


@pytest.mark.parametrize('cull', [1, 0])
def test_painters_order_holds_across_chunks_of_the_tile_list(cull):
    cap = _lib.lib().egn_overlay_tile_capacity()
    n = cap + 3
    frame = orf.noise(40, 70, 9)
    prims = np.tile(np.array([[37., 35., 37., 35., 0.5, 1.0]], dtype=np.float32), (n, 1))    # all on pixel (35, 37)
    colors = (np.arange(n, dtype=np.uint32) * 2654435761 % (1 << 24)).astype(np.uint32)
    assert len(set(colors.tolist())) == n
    tab, _ = orf.table([(40, 70)], [210], [n])
    code, got = _device(frame.reshape(-1), tab, prims, colors, 1, cull)
    assert code == 0
    got = got.reshape(40, 70, 3)
    last = int(colors[-1])
    assert tuple(got[35, 37]) == (last & 255, (last >> 8) & 255, (last >> 16) & 255)
    want = frame.copy()
    want[35, 37] = got[35, 37]
    assert np.array_equal(got, want)
    assert np.array_equal(orf.host_twin(frame.reshape(-1), tab, prims, colors)[1].reshape(40, 70, 3), want)


def test_bad_arguments_and_no_ops():
    frames, buf, tab, prims, colors = orf.build_case([(9, 13)], 1)
    for kw in (dict(n_frames=-1), dict(n_prims=-1), dict(max_hw=(-1, 13)), dict(max_hw=(9, -1)), dict(base=False)):
        code, got = _device(buf, tab, prims, colors, **kw)
        assert code == -1 and np.array_equal(got, buf), kw
    for kw in (dict(n_frames=0), dict(n_prims=0)):
        code, got = _device(buf, tab, prims, colors, **kw)
        assert code == 0 and np.array_equal(got, buf), kw
    # a table row the host entry refuses (stride below 3 W; a range past n_prims): the kernel draws nothing there
    for col, val in ((3, 38), (5, len(prims) + 1)):
        t = tab.copy()
        t[0, col] = val
        assert orf.host_twin(buf, t, prims, colors)[0] == -1
        code, got = _device(buf, t, prims, colors)
        assert code == 0 and np.array_equal(got, buf)


def test_renderer_draws_in_place_on_a_side_stream_beside_a_busy_default_stream():
    sizes = [(33, 45), (8, 70), (40, 17)]
    frames, buf, tab, prims, colors = orf.build_case(sizes, 3)
    want, _ = orf.unpack(orf.host_twin(buf, tab, prims, colors)[1], tab)
    ranges = [(int(r[4]), int(r[5])) for r in tab]
    # frame 0 lives inside a wider buffer: rows of 135 bytes at a stride of 150
    wide = torch.full((33, 150), 0xA5, dtype=torch.uint8).cuda()
    wide[:, :135] = torch.from_numpy(frames[0].reshape(33, 135)).cuda()
    d_frames = [wide[:, :135].view(33, 45, 3), torch.from_numpy(frames[1]).cuda(), torch.from_numpy(frames[2]).cuda()]
    assert d_frames[0].stride() == (150, 3, 1)
    a = torch.empty(32 << 20, device='cuda').normal_()
    b = torch.empty_like(a)
    r = OverlayRenderer()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    launches = _lib.lib().egn_launch_count()
    for _ in range(8):
        b.copy_(a)                                                   # 128 MB each on the default stream
    with torch.cuda.stream(side):
        out = r.draw(d_frames, prims, colors, ranges)
    busy = not torch.cuda.default_stream().query()
    side.synchronize()
    assert _lib.lib().egn_launch_count() - launches == 1             # three frames, one launch
    torch.cuda.synchronize()
    print('default stream still busy when the draw was issued:', busy)
    assert all(o is f for o, f in zip(out, d_frames))
    for o, w in zip(out, want):
        assert np.array_equal(o.cpu().numpy(), w)
    assert (wide[:, 135:] == 0xA5).all()
    # host frames through a GPU renderer: uploaded, drawn, read back; the inputs stay
    out = r.draw(frames, prims, colors, ranges)
    assert all(isinstance(o, np.ndarray) and np.array_equal(o, w) for o, w in zip(out, want))


def _tiny_ego():
    cfg = configs.hrnet_config(8, (64, 64), 33, 'coordinates', modules=(1, 1, 1), num_blocks=1, lifter_neurons=128)
    ego = EgoNet(cfg, pre_trained=False)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=6))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=7))
    ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    return ego.eval().cuda()


def test_post_process_visualize_on_the_cuda_model_equals_the_host_twin(monkeypatch):
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    ego = _tiny_ego()
    paths = ['000001.png', '000002.png']
    images = {paths[0]: orf.noise(96, 128, 1), paths[1]: torch.from_numpy(orf.noise(100, 131, 2)).cuda()}
    boxes = [np.array([[20., 30., 70., 60.], [60., 20., 110., 70.], [5., 5., 40., 40.]]),
             np.array([[30., 10., 90., 80.], [10., 40., 50., 90.], [70., 50., 120., 90.]])]
    row = {'class': 'Car', 'truncation': 0., 'occlusion': 0., 'alpha': 0., 'bbox': [0., 0., 1., 1.],
           'dimensions': [3.9, 1.5, 1.6], 'locations': [2., 1.5, 15.], 'rot_y': 0.2}
    annot = {'path': paths, 'boxes': boxes, 'K': [np.eye(3)] * 2,
             'raw_txt_format': [[dict(row, locations=[2. + 3 * i, 1.5, 15. + 5 * i]) for i in range(3)]] * 2}
    keep = {p: (f.cpu().numpy() if torch.is_tensor(f) else f).copy() for p, f in images.items()}
    rec = ego(annot, images=images)
    out = ego.post_process(rec, visualize=True, images=images)
    host = OverlayRenderer('cpu')
    for p in paths:
        assert np.array_equal(images[p].cpu().numpy() if torch.is_tensor(images[p]) else images[p], keep[p])
        prims, cols = build_primitives(out[p])
        assert len(prims) == 3 * (4 + 12 + 33)
        want = host.draw([keep[p]], prims, cols, [(0, len(prims))])[0]
        assert (want != keep[p]).any() and np.array_equal(out[p]['plots']['image'], want)
        bp, bc, (h, w), n = build_bev_primitives(out[p])
        assert n == 3
        white = np.full((h, w, 3), 255, dtype=np.uint8)
        assert np.array_equal(out[p]['plots']['bev'], host.draw([white], bp, bc, [(0, len(bp))])[0])


def _label(cls, alpha, box, z=20.0):
    return '%s 0.00 0 %.4f %.2f %.2f %.2f %.2f 1.50 1.60 3.90 1.00 1.50 %.2f %.4f' % ((cls, alpha) + box + (z, alpha + 0.05))


def test_inference_tool_draws_and_leaves_its_result_files_alone(tmp_path, monkeypatch):
    from PIL import Image
    import inference_kitti
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    img_dir, lab_dir, gt_dir = tmp_path / 'image_2', tmp_path / 'boxes', tmp_path / 'label_2'
    for d in (img_dir, lab_dir, gt_dir):
        d.mkdir()
    labels = {0: [_label('Car', 0.3, (30.0, 40.0, 120.0, 100.0)), _label('Car', -1.2, (200.0, 50.0, 290.0, 110.0))],
              1: [_label('Pedestrian', 0.5, (100.0, 30.0, 130.0, 100.0))],
              2: [_label('Car', 2.0, (250.0, 20.0, 380.0, 110.0))]}
    for idx, lines in labels.items():
        Image.fromarray(orf.noise(120, 400, idx)).save(str(img_dir / ('%06d.png' % idx)))
        (lab_dir / ('%06d.txt' % idx)).write_text('\n'.join(lines) + '\n')
        # the labels stand 10 m behind the input boxes, or the magenta layer would cover the black one exactly
        (gt_dir / ('%06d.txt' % idx)).write_text('\n'.join(l.replace(' 20.00 ', ' 30.00 ') for l in lines) + '\n')
    common = ['--images', str(img_dir), '--boxes', str(lab_dir), '--synthetic', '--tiny', '--frames-per-step', '2']
    plain = inference_kitti.main(common + ['--out', str(tmp_path / 'plain')])
    drawn = inference_kitti.main(common + ['--out', str(tmp_path / 'drawn'), '--draw', str(tmp_path / 'vis'),
                                           '--draw-gt', '--gt', str(gt_dir)])
    assert 'drawn' not in plain and drawn['drawn'] == 4              # two frames with cars: a picture and a top view each
    for name in ('000000.txt', '000001.txt', '000002.txt'):
        assert (tmp_path / 'plain' / 'data' / name).read_bytes() == (tmp_path / 'drawn' / 'data' / name).read_bytes()
    assert sorted(os.listdir(str(tmp_path / 'vis'))) == ['000000.png', '000000_bev.png', '000002.png', '000002_bev.png']
    for idx in (0, 2):
        src = np.array(Image.open(str(img_dir / ('%06d.png' % idx))))
        pic = np.array(Image.open(str(tmp_path / 'vis' / ('%06d.png' % idx))))
        changed = (pic != src).any(-1)
        assert pic.shape == src.shape and changed.any() and (pic[changed] == (255, 0, 0)).all(-1).any()
        bev = np.array(Image.open(str(tmp_path / 'vis' / ('%06d_bev.png' % idx))))
        assert bev.shape == (600, 500, 3) and (bev == (0, 0, 0)).all(-1).any()      # the label boxes, in black
        assert (bev == (255, 0, 255)).all(-1).any() and (bev == (255, 0, 0)).all(-1).any()
