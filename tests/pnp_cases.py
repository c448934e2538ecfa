"""Seeded inputs shared by the reprojection-refinement tests (tests/test_pnp_refine_cpu.py, tests/test_gpu_pnp_refine.py):
car cuboids in KITTI's camera, their projected key points, a "lifted" shape that is the true one turned by a small
rotation, and a perturbed initial root.  Plain numpy, no project code."""
import numpy as np

KITTI_K = np.array([[707.0493, 0., 604.0814], [0., 707.0493, 180.5066], [0., 0., 1.]])

# cuboid edges as 0-based corner ids: 4 along h, 4 along l, 4 along w (car_instance.py:63-70)
EDGE_PARENT = (0, 2, 4, 6, 0, 1, 2, 3, 0, 1, 4, 5)
EDGE_CHILD = (1, 3, 5, 7, 4, 5, 6, 7, 2, 3, 6, 7)
COEF = (0.332, 0.667)


def rodrigues(v):
    v = np.asarray(v, dtype=np.float64)
    t = np.linalg.norm(v)
    if t < 1e-300:
        return np.eye(3)
    k = v / t
    kx = np.array([[0., -k[2], k[1]], [k[2], 0., -k[0]], [-k[1], k[0], 0.]])
    return np.eye(3) + np.sin(t) * kx + (1. - np.cos(t)) * kx @ kx


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0., s], [0., 1., 0.], [-s, 0., c]])


def canonical(l, h, w, J):
    """construct_box_3d's points about the box centre (car_instance.py:730-747): centre, 8 corners and, for J = 33,
    the bbox12 interpolation at 0.332 / 0.667 of every edge.  Bottom face at y = +h/2."""
    corners = np.array([[(l if c < 4 else 0.) - l / 2, (h if c & 1 else 0.) - h / 2, (0. if (c >> 1) & 1 else w) - w / 2]
                        for c in range(8)])
    pts = [np.zeros((1, 3)), corners]
    if J == 33:
        for cf in COEF:
            pts.append(np.stack([corners[p] + cf * (corners[c] - corners[p]) for p, c in zip(EDGE_PARENT, EDGE_CHILD)]))
    elif J != 9:
        raise ValueError(J)
    return np.concatenate(pts)


def project(pts, K=KITTI_K):
    return np.stack([K[0, 0] * pts[..., 0] / pts[..., 2] + K[0, 2], K[1, 1] * pts[..., 1] / pts[..., 2] + K[1, 2]], -1)


def make(n, J=33, seed=0, noisy=False, pert_deg=15.0, yaw_only_pert=None):
    """n instances.  Returns a dict of float64 arrays:
      shape [n,J-1,3]   the lifted shape handed to the refinement (true rotated shape turned by the perturbation)
      k     [n,J,2]     key points, intr [n,4], root0 [n,3] = true root + uniform +-(0.5, 0.2, 2.0) m
      pts   [n,J,3]     true camera points (root first), root [n,3], dims [n,3] = (l, h, w), yaw [n]
    yaw_only_pert (radians): the perturbation is that rotation about y instead of a random rotation vector.
    noisy: shape noise sigma 0.05 m (the root stays the origin) and pixel noise sigma 1 px."""
    rng = np.random.RandomState(seed)
    out = {k: [] for k in ('shape', 'k', 'pts', 'root', 'root0', 'dims', 'yaw')}
    for _ in range(n):
        l, h, w = rng.uniform(3.2, 4.6), rng.uniform(1.3, 1.9), rng.uniform(1.5, 1.9)
        yaw = -rng.uniform(-np.pi, np.pi)            # (-pi, pi]
        z = rng.uniform(6., 60.)
        root = np.array([rng.uniform(-0.45, 0.45) * z, rng.uniform(1., 2.), z])
        rel = canonical(l, h, w, J) @ rot_y(yaw).T
        pts = rel + root
        rv = np.deg2rad(rng.uniform(-pert_deg, pert_deg, 3))
        P = rodrigues(rv) if yaw_only_pert is None else rot_y(yaw_only_pert)
        shape = rel[1:] @ P.T
        k = project(pts)
        root0 = root + rng.uniform(-1., 1., 3) * np.array([0.5, 0.2, 2.0])
        if noisy:
            shape = shape + rng.normal(0., 0.05, shape.shape)
            k = k + rng.normal(0., 1.0, k.shape)
        for key, v in (('shape', shape), ('k', k), ('pts', pts), ('root', root), ('root0', root0),
                       ('dims', np.array([l, h, w])), ('yaw', yaw)):
            out[key].append(v)
    out = {k: np.ascontiguousarray(np.stack(v), dtype=np.float64) for k, v in out.items()}
    out['intr'] = np.ascontiguousarray(np.tile([KITTI_K[0, 0], KITTI_K[1, 1], KITTI_K[0, 2], KITTI_K[1, 2]], (n, 1)))
    return out


def garbage_weights(case, seed=1, n_bad=10):
    """n_bad of the non-root key points of every instance replaced by garbage (+-500 px) with weight 0.  The root's key
    point stays: it anchors the weak-perspective start."""
    rng = np.random.RandomState(seed)
    k = case['k'].copy()
    n, J = k.shape[:2]
    w = np.ones((n, J))
    for i in range(n):
        bad = 1 + rng.choice(J - 1, n_bad, replace=False)
        k[i, bad] += rng.choice([-1., 1.], (n_bad, 2)) * 500.
        w[i, bad] = 0.
    return k, w


def host_refine(L, shape, k, intr, weights=None, root0=None, max_shift=5.0):
    """egn_pnp_refine_host_f64 on numpy arrays -> (return code, dict of outputs)."""
    shape, k, intr = (np.ascontiguousarray(a, dtype=np.float64) for a in (shape, k, intr))
    n, J = k.shape[0], k.shape[1]
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    r0 = None if root0 is None else np.ascontiguousarray(root0, dtype=np.float64)
    out = {'refined': np.full((n, J, 3), np.nan), 'rt': np.full((n, 12), np.nan), 'cost': np.full((n, 2), np.nan),
           'iters': np.full(n, -7, dtype=np.int32), 'status': np.full(n, -7, dtype=np.int32),
           'dims': np.full((n, 3), np.nan)}
    rc = L.egn_pnp_refine_host_f64(shape.ctypes.data, k.ctypes.data, intr.ctypes.data,
                                   None if w is None else w.ctypes.data, None if r0 is None else r0.ctypes.data,
                                   n, J, float(max_shift), out['refined'].ctypes.data, out['rt'].ctypes.data,
                                   out['cost'].ctypes.data, out['iters'].ctypes.data, out['status'].ctypes.data,
                                   out['dims'].ctypes.data)
    return rc, out
