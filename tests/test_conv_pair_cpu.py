"""The paired F(4x4,3x3) launch without a GPU (csrc/conv_wino4.hip: egn_conv_pair_plan, conv_wino4_pair_kernel).

One launch runs two independent 3x3 convolutions: blocks [0, blocks_a) walk the items of ``a`` (16 x 16 pixel regions x 96
output channels, conv_wino4w_kernel's body), the rest the items of ``b`` (four 8 x 8 images x 48 output channels,
conv_wino4c_kernel<0, 1>'s).  This file restates the block -> (conv, item) -> (region, co-tile) mapping of the two bodies
in numpy and sweeps the host planner: every item of both convolutions is done exactly once, padding items fall outside
the regions, both shares are whole multiples of 8 blocks (a block keeps the XCD its item order assumes) and the items of
a block share their co-tile (pair).  Reference for the layers: libs/model/heatmapModel/hrnet.py:49-76, 286-287."""
import ctypes as C
import itertools

import numpy as np
import pytest

from egonet_amd import _lib, tuner


def _plan(na, ha, wa, cia, coa, nb, hb, wb, cib, cob, cus, stats=0, tickets=0):
    out = (C.c_int * 2)()
    rc = _lib.lib().egn_conv_pair_plan_query(na, ha, wa, cia, coa, nb, hb, wb, cib, cob, cus, stats, tickets, out)
    return None if rc else (out[0], out[1])


def _mode(nct):                     # w4_item_mode (csrc/conv_wino4.h)
    return 2 if nct % 8 == 0 else (1 if nct == 4 else 0)


def _nwork(mode, nreg, nct):        # w4_item_count, KS = 1
    if mode == 2:
        return nreg * nct
    if mode == 1:
        return 8 * -(-nreg // (8 // nct))
    return -(-nreg // 8) * nct * 8


def _items(nblk, nreg, nct):
    """(block, region, co-tile) of every item the share's blocks run; regions >= nreg are padding (skipped)."""
    mode = _mode(nct)
    w = np.arange(_nwork(mode, nreg, nct))
    xq, q = w & 7, w >> 3
    if mode == 0:
        ct, reg = q % nct, (q // nct) * 8 + xq
    elif mode == 1:
        lg = nct >> 1
        reg, ct = q * (8 >> lg) + (xq >> lg), xq & (nct - 1)
    else:
        qq = q // (nct >> 3)
        reg, ct = qq, (q - qq * (nct >> 3)) * 8 + xq
    return w % nblk, reg, ct


def _check_share(nblk, nreg, nct):
    assert nblk > 0 and nblk % 8 == 0
    blk, reg, ct = _items(nblk, nreg, nct)
    real = reg < nreg
    assert (ct >= 0).all() and (ct < nct).all() and (reg >= 0).all()
    done = np.zeros((nreg, nct), dtype=np.int64)
    np.add.at(done, (reg[real], ct[real]), 1)
    assert (done == 1).all()                                    # every item exactly once; padding items do nothing
    for b in range(nblk):
        assert len(set(ct[blk == b])) <= 1, 'a block changes its co-tile'
    assert len(set(blk)) == min(nblk, len(blk))                 # no block of the share is without an item slot


SWEEP = [(na, hw, coa, nb, cob, cus)
         for na, nb in ((1, 1), (3, 5), (8, 8), (16, 16), (20, 37), (64, 64), (128, 128), (7, 130))
         for hw in ((16, 16), (16, 32), (32, 32))
         for coa, cob in ((96, 48), (192, 384), (384, 192), (768, 96), (192, 144))
         for cus in (8, 16, 64, 256, 304)]


def test_every_item_of_both_convolutions_is_done_exactly_once():
    for na, (ha, wa), coa, nb, cob, cus in SWEEP:
        got = _plan(na, ha, wa, 32, coa, nb, 8, 8, 32, cob, cus)
        assert got is not None, (na, ha, wa, coa, nb, cob, cus)
        ga, gb = got
        ncp, nct = coa // 96, cob // 48
        nreg_a, nreg_b = (ha // 16) * (wa // 16) * na, -(-nb // 4)
        _check_share(ga, nreg_a, ncp)
        _check_share(gb, nreg_b, nct)
        wa_, wb_ = _nwork(_mode(ncp), nreg_a, ncp), _nwork(_mode(nct), nreg_b, nct)
        assert ga <= wa_ and gb <= wb_
        if wa_ + wb_ <= cus:
            assert (ga, gb) == (wa_, wb_)                       # both fit: one item per block
        else:                                                   # whole XCD rounds, within the chip where a round fits
            assert ga == wa_ or ga % (8 * ncp) == 0
            assert gb == wb_ or gb % (8 * nct) == 0
            assert ga + gb <= max(cus, 8 * ncp + 8 * nct) or ga == 8 * ncp or gb == 8 * nct


def test_stage4_of_w48_at_64_crops_is_one_block_per_cu():
    assert _plan(64, 16, 16, 192, 192, 64, 8, 8, 384, 384, 256) == (128, 128)
    key_a = (64, 16, 16, 192, 192, 192, 192, 3, 3, 1, 1, False, False)
    key_b = (64, 8, 8, 384, 384, 384, 384, 3, 3, 1, 1, False, False)
    assert tuner.pair_plans(key_a, key_b) == (128, 128)


@pytest.mark.parametrize('bad', [
    dict(stats=1), dict(tickets=1), dict(ha=24), dict(wa=8), dict(hb=16, wb=16), dict(hb=4, wb=4), dict(coa=144),
    dict(coa=48), dict(cob=40), dict(cob=100), dict(cia=20), dict(cib=24), dict(cus=0), dict(na=0)])
def test_the_plan_refuses_what_the_kernel_cannot_run(bad):
    args = dict(na=3, ha=16, wa=16, cia=32, coa=96, nb=5, hb=8, wb=8, cib=32, cob=48, cus=256, stats=0, tickets=0)
    assert _plan(**args) == (8, 8)
    args.update(bad)
    assert _plan(**args) is None, bad


def test_pair_usable_is_the_one_switch(monkeypatch):
    key_a = (64, 16, 16, 192, 192, 192, 192, 3, 3, 1, 1, False, False)
    key_b = (64, 8, 8, 384, 384, 384, 384, 3, 3, 1, 1, False, False)
    untabled = (5, 16, 16, 96, 96, 96, 96, 3, 3, 1, 1, True, False), (3, 8, 8, 48, 48, 48, 48, 3, 3, 1, 1, True, False)
    for k in ('EGONET_AMD_PAIR', 'EGONET_AMD_SKIP_CFG', 'EGONET_AMD_WINO', 'EGONET_AMD_F43'):
        monkeypatch.delenv(k, raising=False)
    tabled = bool(tuner._load_pairs().get(tuner.pair_key(key_a, key_b), {}).get('pair'))
    assert tuner.pair_usable(key_a, key_b) == (tabled and tuner.PAIR_DEFAULT == '1')
    monkeypatch.setenv('EGONET_AMD_PAIR', '1')
    assert not tuner.pair_usable(*untabled)                     # a shape with no entry is not paired
    assert tuner.pair_usable(key_a, key_b) == tabled
    monkeypatch.setenv('EGONET_AMD_PAIR', 'force')
    assert tuner.pair_usable(key_a, key_b) and tuner.pair_usable(*untabled)
    assert not tuner.pair_usable(key_b, key_a)                  # (the planner still decides)
    for var, val in (('EGONET_AMD_SKIP_CFG', '86'), ('EGONET_AMD_SKIP_CFG', '70,82'), ('EGONET_AMD_WINO', '43b'),
                     ('EGONET_AMD_WINO', '0'), ('EGONET_AMD_F43', '0')):
        monkeypatch.setenv(var, val)
        assert not tuner.pair_usable(key_a, key_b), (var, val)
        monkeypatch.delenv(var)
    monkeypatch.setenv('EGONET_AMD_PAIR', '0')
    assert not tuner.pair_usable(key_a, key_b)


def test_forced_pairs_keep_the_arena_invariant_and_the_fine_lanes(monkeypatch):
    """W48 with every applicable level paired: stage 4's branches 2 and 3 (3 modules x 4 blocks x 2 convs = 24 levels)
    become 24 ops on lane 2, each ordered behind what it reads by stream order; two arena tensors share bytes only if
    every use of one happens before the other is defined; branches 0 and 1 keep their lanes and lane 0 never waits."""
    from egonet_amd import configs, engine
    from egonet_amd.model.heatmapModel import hrnet

    def record(mode):
        monkeypatch.setenv('EGONET_AMD_PAIR', mode)
        net = hrnet.get_pose_net(configs.w48_config('heatmap'), is_train=False).eval()
        return engine.HRNetEngine(net)._record(2, 3, 256, 256, 1)[0]
    rec, rec0 = record('force'), record('0')
    pairs = [(i, op) for i, (k, op) in enumerate(rec.ops) if k == 'convpair']
    assert len(pairs) == 24 and all(op['lane'] == 2 for _, op in pairs)
    assert all((op['a']['x'].c, op['a']['x'].h, op['b']['x'].c, op['b']['x'].h) == (192, 16, 384, 8) for _, op in pairs)
    n_launch = [sum(1 for k, _ in r.ops if k not in ('fork', 'join')) for r in (rec, rec0)]
    assert n_launch[1] - n_launch[0] == 24
    assert [k for k, _ in rec.ops].count('fork') == [k for k, _ in rec0.ops].count('fork')
    # every tensor a pair reads was last written on the pair's lane in its region, or in an earlier region
    writer = {}
    for i, (k, op) in enumerate(rec.ops):
        if k == 'convpair':
            for half in (op['a'], op['b']):
                for src in (half['x'], half['res']):
                    if src is not None:
                        assert rec.happens_before(writer[id(src)], i), op['tag']
                writer[id(half['y'])] = i
        elif k in ('conv', 'fuse', 'to_nhwc'):
            writer[id(op['y'])] = i
    # the ops of stage 4 that are not the coarse pair sit on the lanes they have without pairing
    lanes = lambda r: [(op['tag'], op['lane']) for k, op in r.ops if k in ('conv', 'fuse') and '.branches.2.' not in op['tag']
                       and '.branches.3.' not in op['tag'] and not op['tag'].startswith('stage4.0.fuse_layers.3')
                       and not op['tag'].startswith('stage4.1.fuse_layers.3') and op['tag'] not in ('stage4.0.fuse3', 'stage4.1.fuse3')]
    assert lanes(rec) == lanes(rec0)
    total = rec.plan_arena()
    bufs = [b for b in rec.bufs if b.slot == engine.SLOT_ARENA and b.first >= 0]
    for a, b in itertools.combinations(bufs, 2):
        if a.off < b.off + b.nbytes and b.off < a.off + a.nbytes:
            assert all(rec.happens_before(u, b.first) for u in a.uses) or \
                all(rec.happens_before(u, a.first) for u in b.uses), (a.name, b.name)
    assert all(b.off + b.nbytes <= total for b in bufs)
