"""numpy restatement of the reference's lifter pair generation (libs/dataset/KITTI/car_instance.py:611-644,
730-790, 902-1010, 1051-1086, 1120-1123; basic_classes.py:26-44), kept next to the tests that use it.  It issues
the reference's numpy calls in the reference's order, per label and per frame (the matrix products included), so
that with the same numpy and libm the float32 rows are the reference's bits."""
import numpy as np

PARENTS = np.array([1, 3, 5, 7, 1, 2, 3, 4, 1, 2, 5, 6])        # interp_dict['bbox12'], car_instance.py:63-70
CHILDREN = np.array([2, 4, 6, 8, 5, 6, 7, 8, 3, 4, 7, 8])
STD_ROT = np.array([15., 50., 15.]) * np.pi / 180.
STD_TRANS = np.array([0.2, 0.01, 0.2])


def box_3d(l, h, w, coef):
    x = [0.5 * l, l, l, l, l, 0, 0, 0, 0]
    y = [0.5 * h, 0, h, 0, h, 0, h, 0, h]
    z = [0.5 * w, w, w, 0, 0, w, w, 0, 0]
    x = np.array(x) + (-np.float32(l) / 2)
    y = np.array(y) + (-np.float32(h))
    z = np.array(z) + (-np.float32(w) / 2)
    box = np.array([x, y, z])
    par, chi = box[:, PARENTS], box[:, CHILDREN]
    lines = chi - par
    return np.hstack([box, np.hstack([par + c * lines for c in coef])])


def frame_pairs(labels, P, size, coef, draws, T, yaw_draws, out_rep):
    """One frame: labels [n,7] (l h w x y z ry), P [3,4] float32, draws [n,7T+1] or None ->
    (input rows f64 [m,2J], output rows f64, roots [m,3], keep flags over the n(T+1) samples)."""
    P = np.asarray(P, dtype=np.float32)
    K = P[:, :3]
    shift = np.linalg.inv(K) @ P[:, 3].reshape(3, 1)
    cams = []
    for a, lab in enumerate(labels):
        l, h, w = lab[0], lab[1], lab[2]
        locs, rot_y = lab[3:6], lab[6]
        poses = [np.concatenate([locs, [0., rot_y, 0.]])]
        if T:
            rots = draws[a, :3 * T].reshape(T, 3) * STD_ROT.reshape(1, 3)
            rots[:, 1] += rot_y
            trans = 1 + draws[a, 3 * T:6 * T].reshape(T, 3) * STD_TRANS.reshape(1, 3)
            trans *= locs.reshape(1, 3)
            poses += [np.concatenate([trans[i], rots[i]]) for i in range(T)]
        fixed = box_3d(l, h, w, coef)
        for i, pose in enumerate(poses):
            ry = pose[4]
            if yaw_draws:
                ry += draws[a, 6 * T + i] * np.pi
            rot = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
            c = np.matmul(rot, fixed)
            c += np.array([pose[0], pose[1], pose[2]]).reshape([3, 1])
            cams.append((c + shift).T)
    n = len(cams)
    if n == 0:
        return None
    cam = np.vstack(cams)
    proj = K @ cam.T
    proj[:2, :] /= proj[2, :]
    p2d = np.split(proj[:2, :].T, n, axis=0)
    p3d = np.split(cam, n, axis=0)
    keep = np.zeros(n, dtype=bool)
    ins, outs, roots = [], [], []
    for i in range(n):
        j = p2d[i]
        vis = (j - np.array([[0., 0.]]) > 0.).prod(axis=1) * (j - np.array([[size[0], size[1]]]) < 0.).prod(axis=1)
        keep[i] = vis.sum() / len(j) >= 0.3
        if keep[i]:
            root = p3d[i][[0], :]
            rel = p3d[i][1:, :] - root
            ins.append(j.reshape(1, -1))
            outs.append((np.concatenate([root, rel], axis=0) if out_rep == 'R3d+T' else rel).reshape(1, -1))
            roots.append(root)
    return ins, outs, roots, keep


def build(frames, coef, T, yaw_draws, out_rep, draws=None):
    """frames: list of (labels [n,7], P, size).  draws [A,7T+1] over all labels in order, or None.
    -> dict(input f32 [N,2J], output f32, roots f64 [N,3], keep bool [A(T+1)])."""
    ins, outs, roots, keeps, a0 = [], [], [], [], 0
    for labels, P, size in frames:
        n = len(labels)
        r = frame_pairs(labels, P, size, coef, None if draws is None else draws[a0:a0 + n], T, yaw_draws, out_rep)
        a0 += n
        if r is None:
            continue
        ins += r[0]
        outs += r[1]
        roots += r[2]
        keeps.append(r[3])
    return {'input': np.vstack(ins).astype(np.float32), 'output': np.vstack(outs).astype(np.float32),
            'roots': np.vstack(roots), 'keep': np.concatenate(keeps)}


def statistics(inp, out):
    """get_statistics_1d on the float32 rows (operations.py:10-19): numpy's float32 reductions."""
    return {'mean_in': inp.mean(axis=0, keepdims=True), 'std_in': inp.std(axis=0, keepdims=True),
            'mean_out': out.mean(axis=0, keepdims=True), 'std_out': out.std(axis=0, keepdims=True)}


def normalize(data, mean, std):
    return (data - mean) / std
