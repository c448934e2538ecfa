"""The overlay rasteriser without a GPU: the host twin (egn_overlay_draw_host_u8, csrc/overlay_math.h) against the
numpy restatement of the definition (tests/overlay_ref.py) and against closed forms, the primitive builders, and
``EgoNet.post_process(visualize=True)`` on a CPU model."""
import math
import os

import numpy as np
import pytest
import torch

import overlay_ref as orf
from egonet_amd import _lib, configs, synth
from egonet_amd.model.egonet import EgoNet
from egonet_amd.visualization import (CUBOID_EDGES, OverlayRenderer, build_bev_primitives, build_primitives,
                                      parse_color)


def _one(frame, prims, colors, antialias=1):
    """The host twin on one tightly packed frame."""
    h, w = frame.shape[:2]
    tab, _ = orf.table([(h, w)], [3 * w], [len(prims)])
    code, out = orf.host_twin(frame.reshape(-1), tab, np.asarray(prims, dtype=np.float32).reshape(-1, 6), colors,
                              antialias)
    assert code == 0
    return out.reshape(h, w, 3)


@pytest.mark.parametrize('antialias', [1, 0])
@pytest.mark.parametrize('name,sizes,seed,strides,empty', orf.CASES, ids=[c[0] for c in orf.CASES])
def test_host_twin_against_the_restatement(name, sizes, seed, strides, empty, antialias):
    """Both compute the same real number in float64; another association can flip one floor(v + 0.5): |diff| <= 1.
    Outside every primitive's reach the bytes are the input's."""
    frames, buf, tab, prims, colors = orf.build_case(sizes, seed, strides, empty)
    code, out = orf.host_twin(buf, tab, prims, colors, antialias)
    assert code == 0
    got, pad = orf.unpack(out, tab)
    assert (pad == 0xA5).all()
    for f, g, row in zip(frames, got, tab):
        want, reach = orf.draw(f, prims[row[4]:row[5]], colors[row[4]:row[5]], antialias)
        diff = np.abs(g.astype(np.int64) - want.astype(np.int64)).max() if g.size else 0
        print(name, f.shape, 'max |diff| =', diff, 'pixels changed', int((g != f).any(-1).sum()))
        assert diff <= 1
        assert np.array_equal(g[~reach], f[~reach])
        if row[4] == row[5]:
            assert np.array_equal(g, f)
        elif f.shape[0] > 8:
            assert (g != f).any()


def test_closed_forms():
    frame = np.full((20, 30, 3), 10, dtype=np.uint8)
    cap = [(5, 10, 20, 10, 1, 1)]
    white = np.array([orf.rgb(255, 255, 255)], dtype=np.uint32)
    want = frame.copy()
    want[10, 5:21] = 255
    want[9, 5:21] = want[11, 5:21] = 133            # floor(10 + 245 * 0.5 + 0.5)
    # the round caps: (4, 10) and (21, 10) lie at distance 1 from an end point, coverage 0.5 as well
    want[10, 4] = want[10, 21] = 133
    got = _one(frame, cap, white, 1)
    assert np.array_equal(got[8], frame[8]) and np.array_equal(got[12], frame[12])
    # the diagonal neighbours of the end points: distance sqrt(2), coverage 1.5 - sqrt(2), 10 + 245 * 0.0857.. = 31.0
    for y, x in ((9, 4), (11, 4), (9, 21), (11, 21)):
        want[y, x] = math.floor(10 + 245 * (1.5 - math.sqrt(2.0)) + 0.5)
    assert np.array_equal(got, want)
    hard = frame.copy()
    hard[9:12, 5:21] = 255
    hard[10, 4] = hard[10, 21] = 255                # distance exactly 1 <= r
    assert np.array_equal(_one(frame, cap, white, 0), hard)
    # a disc of radius 0 on a pixel centre touches that one pixel: its 4-neighbours have coverage 0.5 - 1 < 0.  By the
    # definition the pixel itself has coverage min(1, 0 + 0.5 - 0) = 0.5 (an ideal point covers no area), so it holds
    # the half-way blend, floor(10 + (col - 10) 0.5 + 0.5) per channel; at full opacity that is all a radius 0 gives
    dot = frame.copy()
    dot[7, 9] = (133, 5, 69)
    assert np.array_equal(_one(frame, [(9, 7, 9, 7, 0, 1)], np.array([orf.rgb(255, 0, 128)], dtype=np.uint32)), dot)
    # ... and a disc of radius 0.5 is the smallest that gives its pixel the full colour, still without neighbours
    dot[7, 9] = (255, 0, 128)
    assert np.array_equal(_one(frame, [(9, 7, 9, 7, 0.5, 1)], np.array([orf.rgb(255, 0, 128)], dtype=np.uint32)), dot)
    # opacity 0 changes nothing
    assert np.array_equal(_one(frame, [(5, 10, 20, 10, 3, 0)], white), frame)
    # two opaque primitives over one pixel: the later colour wins
    two = _one(frame, [(9, 7, 9, 7, 0.5, 1), (9, 7, 9, 7, 0.5, 1)],
               np.array([orf.rgb(1, 2, 3), orf.rgb(200, 100, 50)], dtype=np.uint32))
    assert tuple(two[7, 9]) == (200, 100, 50) and (two != frame).any(-1).sum() == 1


@pytest.mark.parametrize('antialias', [1, 0])
def test_dropped_primitives_leave_no_trace(antialias):
    frame = orf.noise(24, 31, 5)
    prims, colors = orf.varied_prims(24, 31, 6)
    bad, bad_col = orf.dropped_prims()
    base = _one(frame, prims, colors, antialias)
    mixed_p = np.concatenate([bad[:2], prims[:5], bad[2:4], prims[5:], bad[4:]])
    mixed_c = np.concatenate([bad_col[:2], colors[:5], bad_col[2:4], colors[5:], bad_col[4:]])
    assert np.array_equal(_one(frame, mixed_p, mixed_c, antialias), base)
    assert np.array_equal(_one(frame, bad, bad_col, antialias), frame)


def test_bad_arguments_and_no_ops():
    L = _lib.lib()
    frame = orf.noise(6, 7, 1)
    prims, colors = orf.varied_prims(6, 7, 1)
    tab, _ = orf.table([(6, 7)], [21], [len(prims)])
    for col, val in ((3, 20), (1, -1), (2, -1), (0, -8), (4, -1), (5, len(prims) + 1), (4, len(prims) + 1)):
        t = tab.copy()
        t[0, col] = val
        code, out = orf.host_twin(frame.reshape(-1), t, prims, colors)
        assert code == -1 and np.array_equal(out.reshape(6, 7, 3), frame), (col, val)
    buf = frame.copy()
    assert L.egn_overlay_draw_host_u8(buf.ctypes.data, tab.ctypes.data, -1, prims.ctypes.data, colors.ctypes.data,
                                      len(prims), 1) == -1
    assert L.egn_overlay_draw_host_u8(buf.ctypes.data, tab.ctypes.data, 1, prims.ctypes.data, colors.ctypes.data,
                                      -1, 1) == -1
    assert L.egn_overlay_draw_host_u8(None, tab.ctypes.data, 1, prims.ctypes.data, colors.ctypes.data,
                                      len(prims), 1) == -1
    assert L.egn_overlay_draw_host_u8(None, None, 0, prims.ctypes.data, colors.ctypes.data, len(prims), 1) == 0
    t0 = tab.copy()
    t0[0, 4:] = 0
    assert L.egn_overlay_draw_host_u8(buf.ctypes.data, t0.ctypes.data, 1, None, None, 0, 1) == 0
    assert np.array_equal(buf, frame)
    assert L.egn_overlay_tile_capacity() >= 64


def test_renderer_on_the_host_keeps_kinds_and_inputs():
    frames = [orf.noise(9, 11, 1), orf.noise(5, 20, 2)]
    lists = [orf.varied_prims(9, 11, 1), orf.varied_prims(5, 20, 2)]
    prims = np.concatenate([p for p, _ in lists])
    colors = np.concatenate([c for _, c in lists])
    n0 = len(lists[0][0])
    ranges = [(0, n0), (n0, len(prims))]
    r = OverlayRenderer('cpu')
    keep = [f.copy() for f in frames]
    out = r.draw(frames, prims, colors, ranges)
    assert all(isinstance(o, np.ndarray) for o in out)
    for f, k, o, (p, c) in zip(frames, keep, out, lists):
        assert np.array_equal(f, k)
        assert np.array_equal(o, _one(k, p, c))
    out_t = r.draw([torch.from_numpy(f) for f in frames], prims, colors, ranges)
    assert all(torch.is_tensor(o) and np.array_equal(o.numpy(), w) for o, w in zip(out_t, out))
    with pytest.raises(ValueError):
        r.draw(frames, prims, colors, [(0, n0), (n0, len(prims) + 1)])
    with pytest.raises(ValueError):
        r.draw([frames[0][:, :, :2]], prims, colors, ranges[:1])
    assert r.draw([], prims, colors, []) == []


def _record(n, J, seed, gt=0):
    rs = np.random.RandomState(seed)
    rec = {'bbox_resize': [np.array([10. + 5 * i, 20., 60. + 5 * i, 50.]) for i in range(n)],
           'kpts_2d_pred': [rs.uniform(0, 80, (1, 2 * J)) for _ in range(n)]}
    if gt:
        rec['kpts_2d_gt'] = rs.uniform(0, 80, (gt, J, 3))
    return rec


def test_build_primitives_counts_order_and_colours():
    n, J = 3, 33
    rec = _record(n, J, 0, gt=2)
    prims, colors = build_primitives(rec, {'bbox_2d': 'y', 'bbox_3d': (1, 2, 3), 'kpts': ['rx', 'b']}, line_width=3.0,
                                     point_radius=2.5)
    assert prims.shape == (n * (4 + 12 + J) + 2 * 12, 6) and prims.dtype == np.float32 and colors.dtype == np.uint32
    per = 4 + 12 + J
    yellow, red, green = orf.rgb(255, 255, 0), orf.rgb(255, 0, 0), orf.rgb(0, 255, 0)
    for i in range(n):
        blk, col = prims[i * per:(i + 1) * per], colors[i * per:(i + 1) * per]
        x1, y1, x2, y2 = rec['bbox_resize'][i]
        want = np.array([(x1, y1, x2, y1), (x2, y1, x2, y2), (x2, y2, x1, y2), (x1, y2, x1, y1)], dtype=np.float32)
        assert np.array_equal(blk[:4, :4], want) and (col[:4] == yellow).all()
        k = rec['kpts_2d_pred'][i].reshape(-1, 2)
        for e, (a, b) in enumerate(CUBOID_EDGES):
            assert np.array_equal(blk[4 + e, :4], np.concatenate([k[1 + a], k[1 + b]]).astype(np.float32))
        assert (col[4:16] == orf.rgb(1, 2, 3)).all()
        assert np.array_equal(blk[16:, :2], k.astype(np.float32)) and np.array_equal(blk[16:, 2:4], blk[16:, :2])
        assert (col[16:] == red).all()
        assert (blk[:16, 4] == 1.5).all() and (blk[16:, 4] == 2.5).all() and (blk[:, 5] == 1.0).all()
    tail = prims[n * per:]
    for g in range(2):
        k = rec['kpts_2d_gt'][g]
        for e, (a, b) in enumerate(CUBOID_EDGES):
            assert np.array_equal(tail[12 * g + e, :4], np.concatenate([k[1 + a, :2], k[1 + b, :2]]).astype(np.float32))
    assert (colors[n * per:] == green).all()
    # defaults: the reference's post_process colours, bbox_3d falls back to bbox_2d's; no ground truth, no tail
    p2, c2 = build_primitives(_record(2, 9, 1))
    assert len(p2) == 2 * (4 + 12 + 9) and (c2 == red).all() and (p2[:16, 4] == 1.0).all() and (p2[16:25, 4] == 2.0).all()
    assert len(build_primitives({'bbox_resize': [], 'kpts_2d_pred': []})[0]) == 0
    assert parse_color('ro') == red and parse_color('k') == 0 and parse_color([9, 8, 7]) == orf.rgb(9, 8, 7)
    with pytest.raises(ValueError):
        parse_color('q')
    with pytest.raises(ValueError):
        parse_color((1, 2, 256))


def test_build_bev_primitives_hand_computed_box():
    # a 4 m x 2 m box centred at x = 5, z = 20 on the default canvas: 600 rows x 500 columns, u = (x + 25) 10, v = (60 - z) 10
    def rec(rho):
        return {'kpts_2d_pred': [np.zeros((1, 18))], 'euler_angles': np.array([[0., rho, 0.]]),
                'raw_txt_format': [{'locations': [5., 1.5, 20.], 'dimensions': [4., 1.5, 2.], 'rot_y': 0.3}]}
    prims, colors, shape, n = build_bev_primitives(rec(0.0))
    assert shape == (600, 500) and n == 1
    # vertical lines at x = -20, -10, 0, 10, 20 (x = +-25 are no multiples of 10): 5; horizontal at z = 0 .. 60: 7
    grid = 5 + 7
    assert len(prims) == grid + 2 * 5 and (colors[:grid] == orf.rgb(211, 211, 211)).all()
    assert (colors[grid:grid + 5] == orf.rgb(255, 0, 255)).all() and (colors[grid + 5:] == orf.rgb(255, 0, 0)).all()
    with_box = prims[grid + 5:]
    # rho = 0: length along x: corners x = 5 +- 2 -> u = 280 / 320, z = 20 +- 1 -> v = 390 / 410
    us = np.concatenate([with_box[:4, 0], with_box[:4, 2]])
    vs = np.concatenate([with_box[:4, 1], with_box[:4, 3]])
    assert (us.min(), us.max(), vs.min(), vs.max()) == (280., 320., 390., 410.)
    assert np.allclose(with_box[4, :4], (300., 400., 320., 400.))       # heading tick: centre -> middle of the front
    # rho = pi / 2 swaps the footprint's extents: x = 5 +- 1, z = 20 +- 2; the front (dx = +l/2) points to -z
    p90 = build_bev_primitives(rec(math.pi / 2))[0][grid + 5:]
    us = np.concatenate([p90[:4, 0], p90[:4, 2]])
    vs = np.concatenate([p90[:4, 1], p90[:4, 3]])
    assert np.allclose((us.min(), us.max(), vs.min(), vs.max()), (290., 310., 380., 420.), atol=1e-4)
    assert np.allclose(p90[4, :4], (300., 400., 300., 420.), atol=1e-4)
    # the magenta layer keeps the row's own rot_y
    c, s = math.cos(0.3), math.sin(0.3)
    assert np.allclose(prims[grid + 4, :4], (300., 400., (5 + 2 * c + 25) * 10, (60 - (20 - 2 * s)) * 10), atol=1e-4)
    # ground truth first, in black; a row without a placement (a 2-D detector's -1000) does not take part
    r = rec(0.0)
    r['raw_txt_format'][0]['locations'] = [-1000., -1000., -1000.]
    p, c, _, n = build_bev_primitives(r, gt_rows=[{'locations': [0., 1.5, 30.], 'dimensions': [4., 1.5, 2.],
                                                   'rot_y': 0.0}])
    assert n == 0 and len(p) == grid + 5 and (c[grid:] == 0).all()
    # ... unless it is refined: placement and size from the fit
    r.update(refine_status=np.array([1]), refine_dims=np.array([[4., 1.5, 2.]]),
             refine_rt=np.array([[1., 0, 0, 0, 1, 0, 0, 0, 1, 5., 0.75, 20.]]))
    p, c, _, n = build_bev_primitives(r, color_dict={'bbox_2d': 'r', 'bbox_3d': 'b'})
    assert n == 1 and len(p) == grid + 5 and (c[grid:] == orf.rgb(0, 0, 255)).all()
    assert np.allclose(p[grid + 4, :4], (300., 400., 320., 400.))


def _tiny_ego():
    cfg = configs.hrnet_config(8, (64, 64), 33, 'coordinates', modules=(1, 1, 1), num_blocks=1, lifter_neurons=128)
    ego = EgoNet(cfg, pre_trained=False)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=6))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=7))
    ego.LS = synth.synth_lifter_stats(66, 96, seed=1)
    return ego.eval()


def test_post_process_visualize_on_a_cpu_model(tmp_path):
    """Before the rasteriser existed this raised NotImplementedError."""
    from PIL import Image
    ego = _tiny_ego()
    paths = ['a/000007.png', 'b/000008.png']
    boxes = [np.array([[20., 30., 70., 60.], [60., 20., 110., 70.], [5., 5., 40., 40.]]),
             np.array([[30., 10., 90., 80.], [10., 40., 50., 90.], [70., 50., 120., 90.]])]
    records = ego.make_records({'path': paths, 'boxes': boxes})
    rec = ego.get_keypoints(synth.synth_crops(6, 3, 64, 64, seed=8), records, is_cuda=False)
    rec = ego.lift_2d_to_3d(rec, cuda=False)
    row = {'class': 'Car', 'truncation': 0., 'occlusion': 0., 'alpha': 0., 'bbox': [0., 0., 1., 1.],
           'dimensions': [3.9, 1.5, 1.6], 'locations': [2., 1.5, 15.], 'rot_y': 0.2}
    rec[paths[0]]['raw_txt_format'] = [dict(row, locations=[2. + 3 * i, 1.5, 15. + 5 * i]) for i in range(3)]
    images = {paths[0]: np.full((96, 128, 3), 10, dtype=np.uint8), paths[1]: orf.noise(100, 130, 3)}
    keep = {p: f.copy() for p, f in images.items()}
    colors = {'bbox_2d': 'y', 'bbox_3d': 'y', 'kpts': ['yx', 'y']}
    vis = tmp_path / 'vis'
    out = ego.post_process(rec, visualize=True, color_dict=colors, save_dict={'flag': False, 'vis_dir': str(vis)},
                           images=images)
    for p in paths:
        assert np.array_equal(images[p], keep[p])               # the caller's frames are not drawn into
        got = out[p]['plots']['image']
        assert got.dtype == np.uint8 and got.shape == keep[p].shape
        prims, cols = build_primitives(out[p], colors)
        assert len(prims) == 3 * (4 + 12 + 33)
        want, reach = orf.draw(keep[p], prims, cols)
        assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1
        changed = (got != keep[p]).any(-1)
        assert changed.any() and not changed[~reach].any()
        clearly = (np.abs(want.astype(np.int64) - keep[p].astype(np.int64)) > 1).any(-1)
        assert changed[clearly].all()
        stem = os.path.splitext(os.path.basename(p))[0]
        assert np.array_equal(np.array(Image.open(str(vis / (stem + '.png')))), got)
    bev = out[paths[0]]['plots']['bev']
    assert bev.shape == (600, 500, 3) and (bev == 255).any() and (bev == (255, 255, 0)).all(-1).any()
    assert (bev == (255, 0, 255)).all(-1).any()
    p, c, _, n = build_bev_primitives(out[paths[0]], color_dict=colors)
    assert n == 3
    assert np.array_equal(bev, _one(np.full((600, 500, 3), 255, dtype=np.uint8), p, c))
    assert np.array_equal(np.array(Image.open(str(vis / '000007_bev.png'))), bev)
    assert out[paths[1]]['plots']['bev'] is None and sorted(os.listdir(str(vis))) == [
        '000007.png', '000007_bev.png', '000008.png']
    # visualize=False is what it was: no plots, same angles
    again = ego.post_process({p: {k: v for k, v in r.items() if k != 'plots'} for p, r in out.items()})
    assert all('plots' not in r for r in again.values())
    assert all(np.array_equal(again[p]['euler_angles'], out[p]['euler_angles']) for p in paths)
