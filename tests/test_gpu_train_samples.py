"""Training-sample front end on the device (csrc/crop.hip egn_crop_frames_warp_normalize_u8,
egonet_amd/common/train_samples.py, the ``sample_builder`` hook of trainer.train):

1. the multi-frame crop launch against oracle/crop_oracle.py (bit for bit) and against per-frame calls of the
   one-frame entry (torch.equal);
2. the builder against the reference's batches (tests/golden/train_samples.npz);
3. back-to-back calls through the reused staging buffers;
4. trainer.train with ``sample_builder`` against trainer.train over the same batches captured ahead.
"""
import logging
import os

import numpy as np
import pytest
import torch

from conftest import golden
from egonet_amd import _lib, configs, synth, trainer
from egonet_amd.common import crop_gpu, train_samples as ts
from egonet_amd.model.heatmapModel import hrnet as hip_hrnet
from oracle import crop_oracle
from test_train_samples_cpu import CASES, case_cfgs, case_records

pytestmark = pytest.mark.gpu
MEAN, STD = crop_gpu.IMAGENET_MEAN, crop_gpu.IMAGENET_STD
G = golden('train_samples.npz')


def _oracle_crops(frames, box_frame, M, out_wh):
    mean = np.asarray(MEAN, dtype=np.float32).reshape(3, 1, 1)
    std = np.asarray(STD, dtype=np.float32).reshape(3, 1, 1)
    out = []
    for f, m in zip(box_frame, M):
        patch = crop_oracle.warp_affine_u8(frames[f], m.reshape(2, 3), out_wh)
        out.append((patch.transpose(2, 0, 1).astype(np.float32) / np.float32(255) - mean) / std)
    return np.stack(out)


def _multi_frame(frames, box_frame, M, out_wh):
    """One launch of the multi-frame entry over frames packed with gaps (odd offsets, pitch > 3 W)."""
    w, h = out_wh
    blob, tab, off = [], [], 0
    for i, img in enumerate(frames):
        H, W = img.shape[:2]
        pitch = 3 * W + 5 * (i % 2)
        rows = np.zeros((H, pitch), dtype=np.uint8)
        rows[:, :3 * W] = img.reshape(H, 3 * W)
        blob.append(np.zeros(7, np.uint8))
        off += 7
        tab.append([off, H, W, pitch])
        blob.append(rows.reshape(-1))
        off += rows.size
    dev = torch.device('cuda')
    data = torch.from_numpy(np.concatenate(blob)).to(dev)
    tab_d = torch.tensor(tab, dtype=torch.int64, device=dev)
    bf = torch.tensor(np.asarray(box_frame), dtype=torch.int32, device=dev)
    M_d = torch.from_numpy(np.ascontiguousarray(M, dtype=np.float64).reshape(-1, 6)).to(dev)
    n = M_d.shape[0]
    mean_t = torch.tensor(MEAN, dtype=torch.float32, device=dev)
    std_t = torch.tensor(STD, dtype=torch.float32, device=dev)
    out = torch.full((n, 3, h, w), float('nan'), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().egn_crop_frames_warp_normalize_u8(
        _lib.ptr(data), _lib.ptr(tab_d), len(frames), _lib.ptr(bf), _lib.ptr(M_d), n, h, w, _lib.ptr(mean_t),
        _lib.ptr(std_t), _lib.ptr(out), _lib.current_stream()), 'crop frames')
    return out


def _boxes_affines(frames, per, seed, out_wh):
    from egonet_amd.common import img_proc
    rng = np.random.RandomState(seed)
    box_frame, M = [], []
    w, h = out_wh
    for f, img in enumerate(frames):
        H, W = img.shape[:2]
        bx = synth.synth_boxes(per[f], seed=seed + f, img_w=W, img_h=H)
        if per[f] > 1:                                     # partly outside the frame
            bx[0] = [-0.3 * W, -0.2 * H, 0.25 * W, 0.4 * H]
        if per[f] > 2:
            bx[1] = [0.8 * W, 0.7 * H, 1.3 * W, 1.25 * H]
        for b in bx:
            r = img_proc.resize_bbox(*b, target_ar=h / w)
            s = r['s'] * rng.uniform(0.9, 1.1)
            M.append(img_proc.get_affine_transform(r['c'], s, 0, (h, w)).reshape(-1))
            box_frame.append(f)
    return np.array(box_frame), np.stack(M)


@pytest.mark.parametrize('sizes,per,out_wh', [
    ([(375, 1242), (96, 160), (201, 333)], [3, 4, 2], (256, 256)),       # frames of different sizes
    ([(120, 200)], [1], (64, 64)),                                      # n = 1
    ([(77, 131), (150, 90)], [3, 3], (62, 50)),                          # out_w % 4 != 0: the scalar stores
    ([(375, 1242)] * 24, [6] * 23 + [2], (256, 256)),                   # 140 boxes over 24 frames
])
def test_multi_frame_launch_equals_oracle_and_per_frame_calls(sizes, per, out_wh):
    rng = np.random.RandomState(len(sizes) * 7 + sum(per))
    frames = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in sizes]
    box_frame, M = _boxes_affines(frames, per, 3 + len(sizes), out_wh)
    got = _multi_frame(frames, box_frame, M, out_wh)
    torch.cuda.synchronize()
    assert not torch.isnan(got).any()
    # per-frame calls of the one-frame entry (inference's launch)
    ref = torch.empty_like(got)
    Md = torch.from_numpy(M).cuda()
    for f, img in enumerate(frames):
        idx = np.nonzero(box_frame == f)[0]
        if len(idx):
            ref[idx[0]:idx[-1] + 1] = crop_gpu.crop_boxes(img, None, None, out_wh, MEAN, STD,
                                                          affines=Md[idx[0]:idx[-1] + 1].contiguous())
    assert torch.equal(got, ref)
    # the CPU oracle, bit for bit (a subset of the 140-box case keeps the numpy time down)
    sel = np.arange(len(M)) if len(M) <= 16 else np.r_[0:6, 60:66, 134:140]
    want = _oracle_crops(frames, box_frame[sel], M[sel], out_wh)
    assert np.array_equal(got[torch.from_numpy(sel).cuda()].cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_multi_frame_launch_refuses_bad_arguments():
    L = _lib.lib()
    x = torch.zeros(64, dtype=torch.float64, device='cuda')
    p = _lib.ptr(x)
    assert L.egn_crop_frames_warp_normalize_u8(p, p, 0, p, p, 1, 8, 8, p, p, p, None) == -1      # no frame
    assert L.egn_crop_frames_warp_normalize_u8(p, p, 1, p, p, 0, 8, 8, p, p, p, None) == -1      # no box
    assert L.egn_crop_frames_warp_normalize_u8(p, p, 1, p, p, 1, 8, 5000, p, p, p, None) == -1   # too wide
    assert L.egn_crop_frames_warp_normalize_u8(None, p, 1, p, p, 1, 8, 8, p, p, p, None) == -1


@pytest.mark.parametrize('name', CASES)
def test_builder_matches_the_reference_batch(name):
    recs, c = case_records(G, name, with_images=True)
    pre = name + '/'
    b = ts.TrainSampleBuilder(case_cfgs(c['settings']), split=c['split'])
    np.random.seed(int(G[pre + 'np_seed']))
    images, targets, weights, meta = b(recs)
    torch.cuda.synchronize()
    kept = G[pre + 'kept']
    assert len(images) == len(kept)
    for key in ('center', 'scale', 'transformed_joints', 'joints_vis', 'original_joints'):
        assert meta[key].dtype == G[pre + key].dtype
        np.testing.assert_allclose(meta[key], G[pre + key], rtol=0, atol=1e-9, err_msg=key)
    iw, ih = c['settings']['input_size']
    hw, hh = c['settings']['heatmap_size']
    assert tuple(images.shape) == (len(kept), 3, ih, iw) and images.is_cuda
    assert tuple(targets.shape) == (len(kept), 33, hh, hw) and tuple(weights.shape) == (len(kept), 33, 1)
    if c['maps']:
        want_t, want_w = G[pre + 'targets'], G[pre + 'target_weights']
        got_t, got_w = targets.cpu().numpy(), weights.cpu().numpy()
        assert np.array_equal(got_w, want_w)
        assert np.array_equal(got_t > 0, want_t > 0)                       # the support, exactly
        np.testing.assert_allclose(got_t, want_t, rtol=0, atol=2e-7)
    # the pixels: the oracle's warp on the reference's own matrices (a subset of the 140 of 'limit')
    sel = np.arange(len(kept)) if len(kept) <= 16 else np.arange(0, len(kept), 10)
    frames = [r['image'] for r in recs]
    want = _oracle_crops(frames, G[pre + 'frame'][kept][sel], G[pre + 'warps'][kept][sel].reshape(-1, 6), (iw, ih))
    got = images[torch.from_numpy(sel).cuda()].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_back_to_back_calls_do_not_corrupt_each_other():
    cfg = case_cfgs({'input_size': [256, 256], 'heatmap_size': [64, 64], 'sigma': 1, 'scaling': [0.4, 0.4]})
    batches = [synth.synth_frame_records(4, 3, 33, seed=s, hw=hw)
               for s, hw in ((21, (375, 1242)), (22, (200, 300)), (23, (375, 1242)))]
    b = ts.TrainSampleBuilder(cfg)
    np.random.seed(8)
    outs = [b(recs) for recs in batches]            # the three copies queue back to back, no sync in between
    np.random.seed(8)
    for recs, out in zip(batches, outs):
        fresh = ts.TrainSampleBuilder(cfg)(recs)
        torch.cuda.synchronize()
        for x, y in zip(out[:3], fresh[:3]):
            assert torch.equal(x, y)
        for k in out[3]:
            if k != 'path':
                assert np.array_equal(out[3][k], fresh[3][k]), k


# ------------------------------------------------------------------------------------------------------------
# trainer.train with the builder
# ------------------------------------------------------------------------------------------------------------
class _Frames(torch.utils.data.Dataset):
    """Records whose frames are decoded in __getitem__ (PNG files, PIL) -- in the DataLoader workers."""

    def __init__(self, records, root):
        self.items = []
        from PIL import Image
        for i, r in enumerate(records):
            path = os.path.join(root, 'f%03d.png' % i)
            Image.fromarray(r['image']).save(path)
            self.items.append({'path': path, 'boxes': r['boxes'], 'joints': r['joints']})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        it = self.items[i]
        return dict(it, image=crop_gpu.load_rgb(it['path']))


class _Captured(torch.utils.data.Dataset):
    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __getitem__(self, i):
        return self.batches[i]


def _first(batch):
    return batch[0]


def _train_cfg(batch_size, workers):
    cfg = configs.tiny_config('coordinates', num_joints=33)
    cfg['heatmapModel'].update(jitter_bbox=True, jitter_params={'shift': [0.1, 0.1], 'scaling': [0.4, 0.4]},
                               sigma=1, target_type='gaussian')
    cfg.update(train=True, use_gpu=True, exp_type='test',
               dataset={'pth_transform': {'mean': list(MEAN), 'std': list(STD)}},
               optimizer={'optim_type': 'adam', 'lr': 1e-3, 'weight_decay': 0.0, 'momentum': 0.9,
                          'milestones': [3], 'gamma': 0.5},
               training_settings={'total_epochs': 1, 'batch_size': batch_size, 'num_threads': workers,
                                  'shuffle': False, 'report_every': 1, 'eval_during': False, 'plot_loss': False})
    return cfg


def _run(cfg, dataset, **kw):
    net = hip_hrnet.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=31))
    net = net.cuda()
    optim, _ = trainer.prepare_optim(net, cfg)
    lg = logging.getLogger('egonet_amd.test_train_samples')
    lg.handlers = [logging.NullHandler()]
    return trainer.train(dataset, net, None, optim, None, cfg, lg, **kw)['loss']


def test_trainer_train_with_sample_builder(tmp_path):
    os.environ.setdefault('EGONET_AMD_AUTOTUNE', '0')
    records = synth.synth_frame_records(9, 2, 33, seed=12, hw=(96, 160))
    ds = _Frames(records, str(tmp_path))
    builder = ts.TrainSampleBuilder(_train_cfg(3, 0))
    np.random.seed(77)
    captured = [builder(ts.collate_frames([ds[i] for i in range(j, j + 3)])) for j in (0, 3, 6)]
    want = _run(_train_cfg(1, 0), _Captured(captured), collate_fn=_first)
    assert len(want) == 3 and all(np.isfinite(want))
    for workers in (0, 2):
        np.random.seed(77)
        got = _run(_train_cfg(3, workers), ds, collate_fn=ts.collate_frames, sample_builder=builder)
        print('workers %d: %s vs %s' % (workers, got, want))
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
