"""The differentiable soft-arg-max of heat-maps (csrc/softargmax.hip): the coordinates the heat-map head's L_2d and
L_cr terms are computed on (libs/loss/function.py:187-201, soft_arg_max of libs/common/img_proc.py:678-707), forward
and backward on the padded NHWC maps ``[N, h, w, cs]`` of the training tape.  ``forward`` / ``backward`` launch the
kernels on CUDA tensors; ``forward_host`` / ``backward_host`` run the host twins on numpy arrays and return the same
bits (the arithmetic and its order are one header, csrc/softargmax_math.h).  There is no torch fall-back."""
import numpy as np
import torch

from . import _lib


def forward(z, n, h, w, K, cs, div_x, div_y, stream=None):
    """z: the maps, a float32 CUDA tensor of n*h*w*cs elements.  Returns (coords [n, K, 2] = soft-arg-max / (div_x,
    div_y), save [n, K, 4] for ``backward``).  One launch."""
    coords = torch.empty(n, K, 2, dtype=torch.float32, device=z.device)
    save = torch.empty(n, K, 4, dtype=torch.float32, device=z.device)
    _lib.check(_lib.lib().egn_softargmax_fwd_f32(_lib.ptr(z), n, h, w, K, cs, div_x, div_y, _lib.ptr(coords),
                                                 _lib.ptr(save), stream), 'softargmax forward')
    return coords, save


def backward(z, save, dcoords, n, n_rows, h, w, K, cs, div_x, div_y, dz, accumulate=True, stream=None):
    """dz (the maps' layout) += (accumulate) or = the gradient of the first ``n_rows`` images' maps for ``dcoords``
    [n, K, 2]; pad channels and the other images are left alone.  One launch."""
    _lib.check(_lib.lib().egn_softargmax_bwd_f32(_lib.ptr(z), _lib.ptr(save), _lib.ptr(dcoords), n, n_rows, h, w, K, cs,
                                                 div_x, div_y, int(bool(accumulate)), _lib.ptr(dz), stream),
               'softargmax backward')
    return dz


def forward_host(z, K, div_x, div_y):
    """z: numpy float32 [N, h, w, cs] (C order).  Returns (coords [N, K, 2], save [N, K, 4])."""
    n, h, w, cs = z.shape
    coords, save = np.empty((n, K, 2), np.float32), np.empty((n, K, 4), np.float32)
    _lib.check(_lib.lib().egn_softargmax_fwd_host_f32(z.ctypes.data, n, h, w, K, cs, div_x, div_y, coords.ctypes.data,
                                                      save.ctypes.data), 'softargmax forward (host)')
    return coords, save


def backward_host(z, save, dcoords, div_x, div_y, dz, n_rows=None, accumulate=True):
    """The host twin of ``backward`` on numpy arrays; ``dz`` [N, h, w, cs] is updated in place and returned."""
    n, h, w, cs = z.shape
    K = save.shape[1]
    _lib.check(_lib.lib().egn_softargmax_bwd_host_f32(z.ctypes.data, save.ctypes.data, dcoords.ctypes.data, n,
                                                      n if n_rows is None else n_rows, h, w, K, cs, div_x, div_y,
                                                      int(bool(accumulate)), dz.ctypes.data), 'softargmax backward (host)')
    return dz
