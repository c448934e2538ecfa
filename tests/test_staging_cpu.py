"""The staging layout (egonet_amd/common/staging.py) and the sections TrainSampleBuilder hands it.  No GPU."""
import numpy as np
import pytest

from egonet_amd import synth
from egonet_amd.common import staging
from egonet_amd.common import train_samples as ts

SECTIONS = [('a', 5), ('b', 0), ('c', 64), ('d', 24)]


@pytest.mark.parametrize('align', [1, 8, 256])
def test_layout_is_ordered_aligned_and_disjoint(align):
    where, total = staging.layout(SECTIONS, align)
    assert list(where) == [name for name, _ in SECTIONS]
    end = 0
    for name, nbytes in SECTIONS:
        assert where[name] % align == 0 and where[name] >= end          # aligned, in order, past the one before
        end = where[name] + nbytes
        assert end <= total
    assert total % align == 0 and 0 <= total - end < align              # the aligned end of the last section
    assert staging.layout([], align) == ({}, 0)


def _batch():
    """2 frames of different sizes, 2 + 1 boxes, 33 key points, one angle pair per box."""
    recs = synth.synth_frame_records(2, 2, 33, seed=3, hw=(37, 51))
    recs[1] = dict(recs[1], image=np.ascontiguousarray(recs[1]['image'][:30, :45]), boxes=recs[1]['boxes'][:1],
                   joints=recs[1]['joints'][:1])
    rng = np.random.RandomState(3)
    for r in recs:
        r['rots'] = rng.uniform(-np.pi, np.pi, (len(r['boxes']), 2))
    return recs


# What the inline arithmetic of TrainSampleBuilder.__call__ gave for this batch before staging.py existed (commit
# aa0cb8a, its `up` / `offs` / `where` / `total` lines run on the shapes of _batch()): frame offsets, where, total.
PARENT = {'heatmap': ([0, 5888], {'tab': 9984, 'box_frame': 10240, 'M': 10496, 'joints': 10752, 'vis': 13312}, 13824),
          'theta': ([0, 5888], {'tab': 9984, 'box_frame': 10240, 'M': 10496, 'angles': 10752}, 11008)}


@pytest.mark.parametrize('target', ['heatmap', 'theta'])
def test_train_sample_sections_lay_out_as_before(target):
    cfgs = {'train': True, 'heatmapModel': {'jitter_bbox': False, 'input_size': [64, 64], 'heatmap_size': [16, 16],
                                            'num_joints': 33, 'target_type': 'gaussian', 'sigma': 1}}
    b = ts.TrainSampleBuilder(cfgs, device='cpu', target=target)
    recs = _batch()
    arrays = b.pack(recs, b.plan(recs, np.random.RandomState(0)))
    where, total = staging.layout([(name, a.nbytes) for name, a in arrays.items()], staging.ALIGN)
    offs, parent_where, parent_total = PARENT[target]
    assert [where['frame', f] for f in range(2)] == offs
    assert {k: v for k, v in where.items() if isinstance(k, str)} == parent_where and total == parent_total
    assert list(arrays)[:2] == [('frame', 0), ('frame', 1)] and list(arrays)[2:] == list(parent_where)
    assert arrays['tab'].tolist() == [[0, 37, 51, 153], [5888, 30, 45, 135]]
    assert len(arrays['box_frame']) == 3 and arrays['joints' if target == 'heatmap' else 'angles'].shape[0] == 3
