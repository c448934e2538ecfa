"""The algebra of csrc/conv_wgrad_wino.hip restated in numpy (no GPU): the weight gradient of a 3x3 / stride 1 /
pad 1 convolution as Winograd F(2x2,3x3),

    dU_f[co][ci] = sum_tiles dM_f[t][co] V_f[t][ci],   V = B^T d B,   dM = A dY A^T,   dg = G^T dU G,

organised the way the kernel organises it: eight "waves" (frequency row i, column pair jb), each reading only the
patch rows / columns its frequencies touch with ONE sign per direction (both transforms negate frequency 3),
folding its two columns into the two values (q0, q1) the three tap columns need, and the fixed-order sum over
the waves with the coefficients G[i][tap row] and the (q, sign) table of the source wave's jb.  Pinned against
torch's conv2d backward in float64."""
import numpy as np
import torch
import torch.nn.functional as F

from wgrad_sweep import wgrad_wino        # the restatement itself: shared with the weight-gradient sweep


def test_winograd_weight_gradient_organisation_equals_conv2d_backward():
    rng = np.random.default_rng(3)
    for n, ci, co, h, w in ((2, 3, 4, 4, 6), (1, 5, 2, 8, 2)):
        x, dy = rng.standard_normal((n, ci, h, w)), rng.standard_normal((n, co, h, w))
        wt = torch.zeros(co, ci, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(torch.from_numpy(x), wt, None, 1, 1).backward(torch.from_numpy(dy))
        np.testing.assert_allclose(wgrad_wino(x, dy), wt.grad.numpy(), rtol=0, atol=1e-11)


def test_lds_pixel_stride_is_conflict_free():
    """56 dwords per pixel: the four tiles of a K step (two pixels apart) and the 16 lanes of a group
    (consecutive channels) hit 64 distinct banks of a ds_read_b32 for every patch position."""
    for pos in range(0, 56 * 18 * 10, 56):                # any patch-position offset (a pixel multiple)
        for j in range(3):
            banks = {(pos + kq * 2 * 56 + li + 16 * j) % 64 for kq in range(4) for li in range(16)}
            assert len(banks) == 64
    # the unpadded 48-dword stride would put tiles kq and kq + 2 on the same banks
    assert len({(kq * 2 * 48 + li) % 64 for kq in range(4) for li in range(16)}) == 32
