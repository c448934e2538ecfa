"""What the pose-annotation tests share: the committed fixture (tests/golden/pose_annot.npz, made by
tests/golden/make_golden_pose_annot.py from the reference), its cases as builder records, and the bound."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pose_annot.npz')

# Largest |host path - reference| over kpts / raw_kpts of all cases, measured on the CPU: 2.2737367544323206e-13 px
# (one unit in the last place of a coordinate in [1024, 2048); the largest coordinate is 2243 px).  The bound is 4x that:
# cos / sin and the order of a three-term sum may differ by a few such units between numpy, the reference's BLAS
# and the device.  It is not taken from the device path.
MEASURED = 2.2737367544323206e-13
BOUND = 4 * MEASURED


def load():
    g = np.load(GOLDEN)
    return g, json.loads(str(g['cases']))


def cfgs_of(coef, enlarge=None):
    ds = {'detect_classes': ['Car'], '3d_kpt_sample_style': 'bbox9', '2d_kpt_style': 'bbox9',
          'interpolate': {'flag': True, 'style': 'bbox12', 'coef': list(coef)}}
    if enlarge is not None:
        ds['enlarge_factor'] = enlarge
    return {'dataset': ds}


def _texts(g, name, key):
    tname = json.loads(str(g['cases']))[name]['texts']
    return json.loads(g['texts/%s/%s' % (tname, key)].tobytes().decode())


def sizes_of(g, name):
    return g['texts/%s/sizes' % json.loads(str(g['cases']))[name]['texts']]


def records_of(g, name, root=''):
    lt, ct, sizes = _texts(g, name, 'label_text'), _texts(g, name, 'calib_text'), sizes_of(g, name)
    return [{'path': os.path.join(root, '%06d.png' % f), 'labels_text': lt[f], 'calib_text': ct[f],
             'size': tuple(int(v) for v in sizes[f])} for f in range(len(lt))]


def flat(g, name):
    """The reference's boxes, rots, kpts and raw_kpts of a case, concatenated over its kept frames.  The float64 rows
    are stored once, in the raw_kpts of the case's base (same texts and coefficients, threshold 4)."""
    base_raw = g[str(g[name + '/base']) + '/raw_kpts']
    return {'boxes': g[name + '/boxes'], 'rots': g[name + '/rots'],
            'kpts': base_raw[g[name + '/kpts_rows']][:, :, :2], 'raw_kpts': base_raw[g[name + '/raw_rows']]}


def expected(g, name):
    """The reference's five lists, cut per kept frame."""
    out = {'paths': json.loads(str(g[name + '/paths']))}
    ke = np.cumsum(g[name + '/frame_kept'])
    re = np.cumsum(g[name + '/frame_raw'])
    arrays = flat(g, name)
    for key, ends in (('boxes', ke), ('rots', ke), ('kpts', ke), ('raw_kpts', re)):
        out[key] = np.split(arrays[key], ends[:-1])
    return out


def assert_annotations(got, want, bound=BOUND, what=''):
    assert [os.path.basename(p) for p in got['paths']] == want['paths'], what
    for key in ('boxes', 'rots', 'kpts', 'raw_kpts'):
        assert len(got[key]) == len(want['paths']), (what, key)
    worst = 0.0
    for f in range(len(want['paths'])):
        assert np.issubdtype(got['boxes'][f].dtype, np.integer)
        assert np.array_equal(got['boxes'][f], want['boxes'][f]), (what, f)
        assert np.array_equal(got['rots'][f], want['rots'][f]), (what, f)
        assert got['kpts'][f].shape == want['kpts'][f].shape and got['kpts'][f].dtype == np.float64
        assert got['raw_kpts'][f].shape == want['raw_kpts'][f].shape
        assert np.array_equal(got['raw_kpts'][f][..., 2], want['raw_kpts'][f][..., 2]), (what, f)      # visibility
        worst = max(worst, np.abs(got['kpts'][f] - want['kpts'][f]).max(),
                    np.abs(got['raw_kpts'][f][..., :2] - want['raw_kpts'][f][..., :2]).max())
    print('%s: largest |difference| %.3e px (bound %.3e)' % (what, worst, bound))
    assert worst <= bound, (what, worst)
    return worst
