"""Independent restatement of the GROUND (bird's-eye view) and BOX3D blocks of the KITTI evaluator (TEST
INFRASTRUCTURE ONLY; reference tools/kitti-eval/evaluate_object_3d_offline.cpp, functions cited inline), next to
oracle/kitti_eval_oracle.py, which restates the IMAGE block and lends the parts all three share (cleanData,
getThresholds, the division and max rules).

The intersection of two rotated rectangles -- the one thing the reference asks Boost.Geometry for -- is computed here
by a route that shares nothing with csrc/kitti_overlap_math.h's clip: the eight edge half-planes of the two corner
lists (corners as in toPolygon :268-291, in scene coordinates), a Chebyshev centre from ``scipy.optimize.linprog``,
``scipy.spatial.HalfspaceIntersection`` around it and the area from ``ConvexHull.volume``.

Frames are (gt rows, detection rows) of dicts as oracle.kitti_eval_oracle.parse_frame makes them, plus h w l t1 t2 t3 ry.
"""
import functools

import numpy as np
from scipy.optimize import linprog
from scipy.spatial import ConvexHull, HalfspaceIntersection

from oracle import kitti_eval_oracle as orc

METRICS = ('image', 'ground', '3d')
BOX_KEYS = ('x1', 'y1', 'x2', 'y2', 'alpha', 'h', 'w', 'l', 't1', 't2', 't3', 'ry')     # the C ABI's 12 doubles


def corners(b):                                                    # toPolygon :268-291
    c, s = np.cos(b['ry']), np.sin(b['ry'])
    R = np.array([[c, s], [-s, c]])
    local = np.array([[b['l'] / 2, b['l'] / 2, -b['l'] / 2, -b['l'] / 2],
                      [b['w'] / 2, -b['w'] / 2, -b['w'] / 2, b['w'] / 2]])
    return (R @ local).T + np.array([b['t1'], b['t3']])


def _halfplanes(pts):
    """[4][3] rows (nx, ny, c) with nx x + ny y + c <= 0 inside, unit normals, either corner orientation."""
    centre = pts.mean(axis=0)
    rows = []
    for k in range(4):
        a, b = pts[k], pts[(k + 1) % 4]
        n = np.array([b[1] - a[1], a[0] - b[0]])
        n = n / np.linalg.norm(n)
        if n @ (centre - a) > 0:
            n = -n
        rows.append([n[0], n[1], -(n @ a)])
    return np.array(rows)


def bev_intersection(d, g):
    """Area of the intersection of the two bird's-eye-view rectangles."""
    hs = np.vstack([_halfplanes(corners(d)), _halfplanes(corners(g))])
    # Chebyshev centre: max r with n.x + r + c <= 0 for every unit normal
    res = linprog([0, 0, -1], A_ub=np.hstack([hs[:, :2], np.ones((8, 1))]), b_ub=-hs[:, 2],
                  bounds=[(None, None), (None, None), (0, None)], method='highs')
    if res.status != 0 or res.x[2] <= 1e-12:
        return 0.0
    return float(ConvexHull(HalfspaceIntersection(hs, res.x[:2]).intersections).volume)


def _ratio(inter, a, b, criterion):
    if not inter > 0:
        return 0.0
    return inter / (a + b - inter) if criterion == -1 else (inter / a if criterion == 0 else inter / b)


def ground_overlap(d, g, criterion=-1, inter=None):                # :294-314
    inter = bev_intersection(d, g) if inter is None else inter
    return _ratio(inter, d['l'] * d['w'], g['l'] * g['w'], criterion)


def box3d_overlap(d, g, criterion=-1, inter=None):                 # :317-344
    inter = bev_intersection(d, g) if inter is None else inter
    ymax = min(d['t2'], g['t2'])
    ymin = max(d['t2'] - d['h'], g['t2'] - g['h'])
    return _ratio(inter * max(0.0, ymax - ymin), d['h'] * d['l'] * d['w'], g['h'] * g['l'] * g['w'], criterion)


def image_overlap(d, g, criterion=-1):                             # :227-261
    return orc.iou(d, g, over_a=(criterion == 0))


def parse_frame(gt_lines, det_lines):
    gts, dets = orc.parse_frame(gt_lines, det_lines)
    rows = lambda lines, n: [ln.split() for ln in lines if len(ln.split()) >= n]          # noqa: E731
    for objs, fields in ((gts, rows(gt_lines, 15)), (dets, rows(det_lines, 16))):
        for o, f in zip(objs, fields):
            o.update(zip(('h', 'w', 'l', 't1', 't2', 't3', 'ry'), map(float, f[8:15])))
    return gts, dets


def box12(o):
    return [o[k] for k in BOX_KEYS]


def overlap_tables(gts, dets):
    """{metric: [n_gt][n_det]}: over the union, over the detection where the row is a DontCare area (:582)."""
    tab = {m: [[0.0] * len(dets) for _ in gts] for m in METRICS}
    for i, g in enumerate(gts):
        crit = 0 if g['type'].lower() == 'dontcare' else -1
        for j, d in enumerate(dets):
            inter = bev_intersection(d, g)
            tab['image'][i][j] = image_overlap(d, g, crit)
            tab['ground'][i][j] = ground_overlap(d, g, crit, inter)
            tab['3d'][i][j] = box3d_overlap(d, g, crit, inter)
    return tab


def stats(cls, gts, dets, ov, gflag, dflag, with_fp, thresh):      # computeStatistics :456-615, no AOS
    NONE = -10000000
    min_ov = orc.MIN_OVERLAP[cls]                                  # :55, the same row for every metric
    taken = [False] * len(dets)
    low = [with_fp and d['score'] < thresh for d in dets]
    tp = fp = fn = 0
    scores = []
    for i in range(len(gts)):
        if gflag[i] == -1:
            continue
        pick, valid, best, small = -1, NONE, 0.0, False
        for j, d in enumerate(dets):
            if dflag[j] == -1 or taken[j] or low[j]:
                continue
            o = ov[i][j]
            if not with_fp and o > min_ov and d['score'] > valid:
                pick, valid = j, d['score']
            elif with_fp and o > min_ov and (o > best or small) and dflag[j] == 0:
                best, pick, valid, small = o, j, 1, False
            elif with_fp and o > min_ov and valid == NONE and dflag[j] == 1:
                pick, valid, small = j, 1, True
        if valid == NONE and gflag[i] == 0:
            fn += 1
        elif valid != NONE and (gflag[i] == 1 or dflag[pick] == 1):
            taken[pick] = True
        elif valid != NONE:
            tp += 1
            scores.append(dets[pick]['score'])
            taken[pick] = True
    if with_fp:
        fp = sum(1 for j in range(len(dets)) if not (taken[j] or dflag[j] != 0 or low[j]))
        for i, g in enumerate(gts):
            if g['type'].lower() != 'dontcare':
                continue
            for j in range(len(dets)):
                if taken[j] or dflag[j] != 0 or low[j]:
                    continue
                if ov[i][j] > min_ov:
                    taken[j] = True
                    fp -= 1
    return tp, fp, fn, scores


def eval_class(cls, level, frames, tables, metric):                # eval_class :622-706
    cleaned, allscores, n_gt = [], [], 0
    for (gts, dets), tab in zip(frames, tables):
        gflag, dflag, _, n = orc.clean(cls, level, gts, dets)      # difficulty by the 2D box in every metric
        n_gt += n
        cleaned.append((gflag, dflag))
        allscores += stats(cls, gts, dets, tab[metric], gflag, dflag, False, 0)[3]
    thr = orc.thresholds(allscores, float(n_gt)) if allscores else []
    counts = [[0, 0, 0] for _ in thr]
    for (gts, dets), tab, (gflag, dflag) in zip(frames, tables, cleaned):
        for t, th in enumerate(thr):
            tp, fp, fn, _ = stats(cls, gts, dets, tab[metric], gflag, dflag, True, th)
            counts[t][0] += tp
            counts[t][1] += fp
            counts[t][2] += fn
    prec = [0.0] * orc.SAMPLES
    for i, (tp, fp, fn) in enumerate(counts[:orc.SAMPLES]):
        prec[i] = orc._div(tp, tp + fp)
    for i in range(min(len(counts), orc.SAMPLES)):
        prec[i] = orc._max_from(prec, i)
    return prec, counts


def evaluate(frames, tables=None):
    """frames: [(gts, dets)] from ``parse_frame``.  -> {class: {metric: (precision[3][41], counts[3])}} with a metric
    present only where the class is scored in it (:162-167)."""
    tables = tables if tables is not None else [overlap_tables(g, d) for g, d in frames]
    field = {'image': ('x1', lambda v: v >= 0), 'ground': ('t1', lambda v: v != -1000), '3d': ('t2', lambda v: v != -1000)}
    out = {}
    for c, name in enumerate(orc.NAMES):
        for metric, (key, ok) in field.items():
            if any(d['type'].lower() == name and ok(d[key]) for _, dets in frames for d in dets):
                res = [eval_class(c, lv, frames, tables, metric) for lv in range(3)]
                out.setdefault(name, {})[metric] = ([r[0] for r in res], [r[1] for r in res])
    return out


# ---- frame sets shared by tests/test_kitti_eval3d_cpu.py and tests/test_gpu_kitti_eval3d.py ----

def gt_line(cls, trunc, occ, alpha, box, dims, loc, ry):
    return '%s %.2f %d %.4f %.2f %.2f %.2f %.2f %.4f %.4f %.4f %.4f %.4f %.4f %.4f' % (
        (cls, trunc, occ, alpha) + tuple(box) + tuple(dims) + tuple(loc) + (ry,))


def det_line(cls, alpha, box, dims, loc, ry, score):
    return '%s -1 -1 %.4f %.2f %.2f %.2f %.2f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.6f' % (
        (cls, alpha) + tuple(box) + tuple(dims) + tuple(loc) + (ry, score))


DONTCARE_3D = ((-1, -1, -1), (-1000, -1000, -1000), -10)


def random_frames(seed, n_frames=12):
    """{frame id: (gt lines, detection lines)} in the style of tests/test_kitti_eval_cpu.py::_random_frames, with 3D
    boxes: a detection near most objects (location, rotation_y and dimensions jittered), strays, detections inside
    DontCare areas, and some detections that carry no 3D box (t = -1000)."""
    rng = np.random.RandomState(seed)
    frames = {}
    for f in range(n_frames):
        gts, dets = [], []
        for _ in range(rng.randint(0, 7)):
            cls = rng.choice(['Car', 'Car', 'Car', 'Van', 'Pedestrian', 'Person_sitting', 'Cyclist', 'DontCare', 'Truck'])
            x1, y1 = rng.uniform(0, 1100), rng.uniform(100, 300)
            w, h = rng.uniform(20, 200), rng.uniform(15, 120)
            box = (x1, y1, x1 + w, y1 + h)
            alpha = rng.uniform(-3.1, 3.1)
            if cls == 'DontCare':
                gts.append(gt_line(cls, -1, -1, -10, box, *DONTCARE_3D))
                if rng.rand() < 0.7:                             # a detection inside the area, with or without a 3D box
                    in3d = ((1.5, 1.6, 3.9), (rng.uniform(-20, 20), 1.6, rng.uniform(5, 60)), 0.3) if rng.rand() < 0.5 \
                        else ((1.5, 1.6, 3.9), (-1000, -1000, -1000), 0.3)
                    dets.append(det_line('Car', 0.3, (x1 + 1, y1 + 1, x1 + w * 0.6, y1 + max(h * 0.6, 30)), *in3d,
                                         score=rng.uniform(0.05, 1.0)))
                continue
            dims = np.array([1.5, 1.6, 3.9]) * rng.uniform(0.8, 1.2, 3) if cls in ('Car', 'Van', 'Truck') \
                else np.array([1.7, 0.6, 0.9]) * rng.uniform(0.8, 1.2, 3)
            loc = np.array([rng.uniform(-20, 20), rng.uniform(1.2, 1.9), rng.uniform(5, 60)])
            ry = rng.uniform(-3.1, 3.1)
            gts.append(gt_line(cls, rng.choice([0.0, 0.1, 0.25, 0.4, 0.7]), rng.randint(0, 4), alpha, box, dims, loc, ry))
            if rng.rand() < 0.8:                                 # a detection near most objects
                j = rng.uniform(-0.12, 0.12, 4) * np.array([w, h, w, h])
                dcls = cls if cls in ('Car', 'Pedestrian', 'Cyclist') else rng.choice(['Car', 'Pedestrian'])
                spread = rng.choice([0.02, 0.1, 0.3])
                d3 = (dims * rng.uniform(0.93, 1.07, 3), loc + rng.normal(0, spread, 3) * np.array([1, 0.3, 1]),
                      ry + rng.normal(0, 0.08))
                if rng.rand() < 0.1:
                    d3 = (d3[0], (-1000, -1000, -1000), d3[2])
                dets.append(det_line(dcls, alpha + rng.normal(0, 0.4), np.array(box) + j, *d3, score=rng.uniform(0.05, 1.0)))
        for _ in range(rng.randint(0, 3)):                       # strays, some too small
            x1, y1 = rng.uniform(0, 1100), rng.uniform(100, 300)
            dets.append(det_line(rng.choice(['Car', 'Pedestrian', 'Cyclist']), rng.uniform(-3, 3),
                                 (x1, y1, x1 + rng.uniform(20, 150), y1 + rng.uniform(10, 90)),
                                 np.array([1.5, 1.6, 3.9]) * rng.uniform(0.8, 1.2, 3),
                                 (rng.uniform(-20, 20), rng.uniform(1.2, 1.9), rng.uniform(5, 60)), rng.uniform(-3, 3),
                                 rng.uniform(0.05, 1.0)))
        frames[f * 3 + 1] = (gts, dets)
    return frames


def to_arrays(lines, with_score):
    """Label / result lines of one frame -> the dict ``egonet_amd.evaluate.evaluate_frames`` takes."""
    rows = [ln.split() for ln in lines if len(ln.split()) >= (16 if with_score else 15)]
    num = np.array([[float(v) for v in r[1:15]] for r in rows], dtype=np.float64).reshape(len(rows), 14)
    fr = {'type': [r[0] for r in rows], 'truncation': num[:, 0], 'occlusion': num[:, 1].astype(np.int64),
          'alpha': num[:, 2], 'bbox': num[:, 3:7], 'dimensions': num[:, 7:10], 'location': num[:, 10:13],
          'rotation_y': num[:, 13]}
    if with_score:
        fr['score'] = np.array([float(r[15]) for r in rows], dtype=np.float64)
    return fr


@functools.lru_cache(maxsize=None)
def reference(seed, n_frames=12):
    """(frames as lines, parsed frames, overlap tables, evaluate(...)) of ``random_frames(seed)``, computed once."""
    frames = random_frames(seed, n_frames)
    parsed = [parse_frame(*frames[k]) for k in sorted(frames)]
    tables = [overlap_tables(g, d) for g, d in parsed]
    return frames, parsed, tables, evaluate(parsed, tables)
