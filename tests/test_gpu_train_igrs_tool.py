"""tools/train_IGRs.py end to end on a three-frame KITTI-like tree (the fixture's 'tiny' case, 64 x 48 PNG files):
``HC.pth`` loads strictly, the loss is finite, the validation reports, and the tool's last loss equals, bit for bit,
the one ``trainer.train`` gives on records built by hand from the reference's arrays -- the tool adds plumbing, not
arithmetic."""
import argparse
import json
import logging
import os

import numpy as np
import pytest
import torch

import pose_annot_cases as pc
from egonet_amd import trainer
from egonet_amd.common import crop_gpu, train_samples as ts
from egonet_amd.model.heatmapModel import hrnet
from tools import train_IGRs as tool

pytestmark = pytest.mark.gpu
G, CASES = pc.load()


def _write_tree(root):
    from PIL import Image
    rng = np.random.RandomState(11)
    records = pc.records_of(G, 'tiny')
    lt, ct = [r['labels_text'] for r in records], [r['calib_text'] for r in records]
    for d in ('image_2', 'label_2', 'calib'):
        os.makedirs(os.path.join(root, d))
    stems = []
    for f in range(len(lt)):
        stem = '%06d' % f
        w, h = records[f]['size']
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, 'image_2', stem + '.png'))
        for d, text in (('label_2', lt[f]), ('calib', ct[f])):
            with open(os.path.join(root, d, stem + '.txt'), 'w') as fh:
                fh.write(text)
        stems.append(stem)
    with open(os.path.join(root, 'val.txt'), 'w') as fh:
        fh.write('\n'.join(stems[1:]) + '\n')
    return stems


class _HandMade(torch.utils.data.Dataset):
    """Records from the reference's arrays, cut per frame by hand."""

    def __init__(self, root):
        want = pc.expected(G, 'tiny')
        self.items = [{'path': os.path.join(root, 'image_2', p), 'boxes': b, 'joints': k}
                      for p, b, k in zip(want['paths'], want['boxes'], want['kpts'])]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return dict(self.items[i], image=crop_gpu.load_rgb(self.items[i]['path']))


def test_tool_trains_writes_hc_and_adds_no_arithmetic(tmp_path, monkeypatch):
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    root, out_dir = str(tmp_path / 'kitti'), str(tmp_path / 'out')
    _write_tree(root)
    common = ['--kitti', root, '--out', out_dir, '--tiny', '--seed', '0', '--batch-frames', '2', '--workers', '0',
              '--report-every', '1']
    out = tool.main(common + ['--epochs', '2', '--max-steps', '2'])
    assert out['steps'] == 2 and np.isfinite(out['last_loss'])
    assert (out['frames'], out['frames_kept'], out['labels']) == (3, 3, 6)
    assert (out['kept_inlier'], out['dropped_inlier'], out['kept_visible'], out['dropped_visible']) == (5, 1, 5, 0)
    assert out['out'] == os.path.join(out_dir, 'HC.pth') and 'eval' not in out

    args = argparse.Namespace(tiny=True, lr=1e-3, epochs=1, batch_frames=2, workers=0, report_every=1, eval_every=0)
    cfgs = tool.igr_cfgs(args)
    state = torch.load(out['out'])
    assert all(torch.is_tensor(v) and not v.is_cuda for v in state.values())
    net = hrnet.get_pose_net(cfgs, is_train=False)
    net.load_state_dict(state, strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in state.values() if v.is_floating_point())

    # the same two steps without the tool: the reference's arrays, a plain DataLoader, the same seed.  The boxes are
    # equal integers; the tool's device-built key points may differ from the reference's in the last float64 bits
    # (below pose_annot_cases.BOUND), and the equality below holds because that vanishes where the training batch
    # rounds the transformed joints and the targets to float32.  If an ulp-level change of the annotation kernel ever
    # breaks this line, check that before suspecting the tool's plumbing.
    model = tool.build_model(cfgs, 0)
    optim, sche = trainer.prepare_optim(model, cfgs)
    lg = logging.getLogger('egonet_amd.test_train_igrs')
    lg.handlers = [logging.NullHandler()]
    record = trainer.train(_HandMade(root), model, None, optim, sche, cfgs, lg, collate_fn=ts.collate_frames,
                           sample_builder=ts.TrainSampleBuilder(cfgs, split='train'))
    print('tool %r, by hand %r' % (out['last_loss'], record['loss']))
    assert len(record['loss']) == 2 and record['loss'][-1] == out['last_loss']
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), state[k]), k

    # validation during training and at the end: a finite JointDistance2DSIP report over the two validation frames
    out = tool.main(common + ['--epochs', '1', '--eval-every', '1', '--valid-split-file', os.path.join(root, 'val.txt')])
    assert out['steps'] == 2 and np.isfinite(out['last_loss'])
    assert out['eval']['metric'] == 'JointDistance2DSIP' and np.isfinite(out['eval']['mean'])
    assert out['eval']['count'] == 2 * 3 * 33                   # two passes over 3 cars of 33 key points
