"""Writes tests/golden/integral_loss.npz: the REFERENCE's JointsCompositeLoss (libs/loss/function.py:61-202) on a
model output that is heat-maps only -- coordinates_pred == None, so the loss runs soft_arg_max (img_proc.py:678-707) on
the maps, divides by hm_size and feeds L_2d and L_cr (function.py:187-201).  Per case: the inputs, the loss and
d loss / d maps by torch autograd, float32 on the CPU.

    python tests/golden/make_integral_loss.py          (needs the reference checkout next to this repository's
                                                        fixtures maker, see make_golden.py: REF)

Stubs as in make_golden.py: cv2, the torch.cuda tensor types soft_arg_max hard-codes, ``.cuda()`` as identity.
Cases (h x w maps):
  sq     3 x 5 maps of 16 x 16, ['mse', 'l1', 'None']
  nsq    3 x 5 maps of 12 x 16 (hm_size = [16, 12]): pins x / hm_size[1], y / hm_size[0]
  cr     3 x 33 maps of 8 x 8, ['mse', 'l1', 'sl1'], cr_indices 'bbox12', apply_cr_loss, a threshold that keeps some
         lines and drops others (the kept count is recorded)
  mixed  the same with 2 labelled crops of 3: the maps are cut to the labelled prefix before the soft-arg-max
         (function.py:184-185), so the third crop's gradient is zero, L_cr included
Deterministic: re-running leaves the file byte-identical.
"""
import json
import os
import sys
from unittest import mock

import numpy as np
import torch
import torch.cuda.comm

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG          # noqa: E402  (the stubs and the reference's path)


def _maps(n, k, h, w, seed, peak):
    """Noise plus one Gaussian bump per map at a random place: the soft-arg-max spreads over the map."""
    g = torch.Generator().manual_seed(seed)
    cx = torch.rand(n, k, 1, 1, generator=g) * (w - 1)
    cy = torch.rand(n, k, 1, 1, generator=g) * (h - 1)
    ys = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
    xs = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w)
    bump = torch.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / 2.0) * peak
    return (bump + torch.randn(n, k, h, w, generator=g) * 0.5).contiguous()


def main():
    MG._install_stubs()
    sys.path.insert(0, MG.REF)
    import libs.loss.function as ref_loss
    from libs.dataset.KITTI.car_instance import cr_indices_dict
    bbox12 = cr_indices_dict['bbox12']
    cases = {
        'sq': dict(n=3, n_fs=3, k=5, h=16, w=16, spec=['mse', 'l1', 'None'], weights=[1.0, 0.1, 'None'], peak=4.0),
        'nsq': dict(n=3, n_fs=3, k=5, h=12, w=16, spec=['mse', 'l1', 'None'], weights=[1.0, 0.1, 'None'], peak=4.0),
        'cr': dict(n=3, n_fs=3, k=33, h=8, w=8, spec=['mse', 'l1', 'sl1'], weights=[1.0, 0.1, 0.05], peak=6.0,
                   thres=0.2),
        'mixed': dict(n=3, n_fs=2, k=33, h=8, w=8, spec=['mse', 'l1', 'sl1'], weights=[1.0, 0.1, 0.05], peak=6.0,
                      thres=0.2),
    }
    arrs = {'cases': np.array(json.dumps(cases)), 'bbox12': np.asarray(bbox12, np.int32)}
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with mock.patch.object(torch.cuda, 'FloatTensor', torch.FloatTensor, create=True), \
                mock.patch.object(torch.cuda.comm, 'broadcast', lambda t, devices: [t]):
            for i, (name, c) in enumerate(sorted(cases.items())):
                n, n_fs, k, h, w = c['n'], c['n_fs'], c['k'], c['h'], c['w']
                img = [4 * w, 4 * h]                                  # img_size = (width, height)
                crit = ref_loss.JointsCompositeLoss(spec_list=c['spec'], img_size=img, hm_size=[w, h],
                                                    loss_weights=c['weights'], target_cr=4 / 3,
                                                    cr_loss_thres=c.get('thres', 0.15))
                if c['spec'][2] != 'None':
                    crit.cr_indices = bbox12
                    crit.apply_cr_loss = True
                g = torch.Generator().manual_seed(500 + i)
                maps = _maps(n, k, h, w, 600 + i, c['peak']).requires_grad_(True)
                target = torch.rand(n_fs, k, h, w, generator=g)
                joints = torch.rand(n_fs, k, 3, generator=g) * torch.tensor([img[0], img[1], 1.0])
                loss = crit(maps, target, None, {'transformed_joints': joints.numpy().copy()})
                loss.backward()
                p = name + '/'
                arrs[p + 'maps'] = maps.detach().numpy().copy()
                arrs[p + 'target'] = target.numpy().copy()
                arrs[p + 'joints'] = joints.numpy().copy()
                arrs[p + 'loss'] = np.array(float(loss.detach()), np.float64)
                arrs[p + 'dmaps'] = maps.grad.numpy().copy()
                if c['spec'][2] != 'None':
                    coords, _ = MG_soft(maps.detach()[:n_fs], w, h)
                    mask = crit.get_cr_mask(coords.numpy(), crit.cr_loss_thres)
                    arrs[p + 'cr_mask'] = mask.numpy().reshape(n_fs, -1).copy()
                    assert 0 < float(mask.sum()) < mask.numel(), (name, float(mask.sum()), mask.numel())
                print(name, float(loss), float(maps.grad.abs().max()))
    finally:
        torch.Tensor.cuda = orig_cuda
    out = os.path.join(HERE, 'integral_loss.npz')
    np.savez_compressed(out, **arrs)
    print(out, os.path.getsize(out), 'bytes')


def MG_soft(maps, w, h):
    """The reference's soft_arg_max / hm_size on detached maps (for the recorded mask only)."""
    import libs.common.img_proc as ref_ip
    coords, maxvals = ref_ip.soft_arg_max(maps.clone())
    coords[:, :, 0] /= h
    coords[:, :, 1] /= w
    return coords, maxvals


if __name__ == '__main__':
    main()
