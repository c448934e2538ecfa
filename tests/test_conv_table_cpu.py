"""The conv config table (csrc/conv_plan.hip: kConfigs) answers every host-only question exactly as it did before its
rows got named fields: tests/golden/conv_table.npz holds what the product and the probe library of that commit said
(tools/dump_conv_table.py) -- filter kind, tile, kernel name of every id; plan, ticket words and BatchNorm partial rows of
every id on 1885 shapes (every key of the shipped table, the shapes of the planner tests, the edges the decoders branched
on).  The loaded library is asked the same questions and compared with the section of its build, field by field."""
import json
import os

import numpy as np

from egonet_amd import _lib
from tools import dump_conv_table as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_table.npz')


def _shape(row):
    return ', '.join('%s=%d' % kv for kv in zip(D.SHAPE_FIELDS, row))


def test_table_answers_match_the_recorded_ones():
    L = _lib.lib()
    sec = D.section_of(L)
    with np.load(GOLDEN) as z:
        want = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(sec + '/')}
        shapes = z['shapes']
    assert len(want) == 6, sorted(want)
    # the tool still asks what the fixture was asked (the shipped table, the shape lists)
    assert np.array_equal(shapes, D.shapes()), 'tools/dump_conv_table.py: shapes() changed since the fixture was written'
    ncfg = L.egn_conv_num_configs()
    assert ncfg == len(want['kind']) == want['plan'].shape[1] - 1
    got = D.dump(L, shapes)

    want_names, got_names = json.loads(str(want['names'])), json.loads(str(got['names']))
    for c in range(1, ncfg + 1):
        assert got['kind'][c - 1] == want['kind'][c - 1], '%s: cfg %d: kind %d, recorded %d' % (
            sec, c, got['kind'][c - 1], want['kind'][c - 1])
        assert tuple(got['tile'][c - 1]) == tuple(want['tile'][c - 1]), '%s: cfg %d: tile_m, tile_n %s, recorded %s' % (
            sec, c, tuple(got['tile'][c - 1]), tuple(want['tile'][c - 1]))
        assert got_names[c - 1] == want_names[c - 1], '%s: cfg %d: name %r, recorded %r' % (
            sec, c, got_names[c - 1], want_names[c - 1])

    def first_difference(field, g, w, names):
        if np.array_equal(g, w):
            return None
        idx = np.argwhere(g != w)[0]
        i, c = int(idx[0]), int(idx[1])
        what = field if names is None else names[int(idx[2])]
        return '%s: cfg %d on (%s): %s %d, recorded %d' % (sec, c, _shape(shapes[i]), what, g[tuple(idx)], w[tuple(idx)])

    for field, names in (('plan', D.PLAN_FIELDS), ('tickets', None), ('bnrows', None)):
        assert got[field].shape == want[field].shape, field
        msg = first_difference({'tickets': 'ticket words', 'bnrows': 'bnstats rows'}.get(field, field), got[field],
                               want[field], names)
        assert msg is None, msg


def test_fixture_covers_both_builds_and_every_config():
    """Every id 1..93 except the retired ones plans for at least one recorded shape in the probe build, every
    selectable one in the product build; the K-split and the statistics configs answer non-zero somewhere."""
    with np.load(GOLDEN) as z:
        for sec in ('product', 'probes'):
            plans = (z[sec + '/plan'][:, 1:, 0] == 0).any(axis=0)
            kind = z[sec + '/kind']
            retired = np.arange(1, len(kind) + 1)
            retired = (retired >= 31) & (retired <= 40)
            if sec == 'probes':
                assert plans[~retired].all() and not plans[retired].any()
            else:
                assert np.array_equal(plans, kind >= 0)
            assert set(np.nonzero((z[sec + '/tickets'] > 0).any(axis=0))[0]) == {83, 84}
            assert {51, 59, 70, 80, 82, 83, 84} <= set(np.nonzero((z[sec + '/bnrows'] > 0).any(axis=0))[0])
        assert z['shapes'].shape[0] >= 411
