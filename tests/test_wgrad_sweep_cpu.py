"""No GPU: the weight-gradient sweep's corpus reaches every kernel the dispatch can launch (through the host-only
plan query), and its element-wise bound separates honest fp32 from the slips a kernel could make."""
import math

import torch

import wgrad_sweep as S


def _plans(reqs):
    out = []
    for r in reqs:
        p = S.plan(r['key'])
        assert p is not None, ('the planner refuses a request of the corpus', r)
        out.append((r, p))
    return out


def _served(plans):
    """The purposes a list of planned requests serves, in the supplement's terms."""
    got = set()
    for _, p in plans:
        got.add(('row', p['row']))
        got.add(('reduce', (p['lanes'], p['frag'])))
        got |= {('shrink', b) for b in S.shrink_branch(p)}
    return got


def test_every_corpus_request_plans_and_the_query_agrees_with_ws_bytes():
    reqs = S.corpus_requests()
    assert len(reqs) > 300 and len({r['key'] for r in reqs}) == len(reqs)
    for r, p in _plans(reqs + S.supplement_requests()):
        assert S.ws_bytes(r['key']) > 0
        assert 0 <= p['row'] < S.num_variants() and p['form'] in S.FORM_NAMES and p['frag'] == (p['form'] > 0)
        assert p['lanes'] == (32 if p['nsplit'] > 64 else 8 if p['nsplit'] > 4 else 2)
        assert p['nsplit'] == -(-p['ntiles'] // p['tiles_per_split'])
    # the query refuses exactly what egn_conv2d_wgrad_ws_bytes refuses
    for key in ((1, 8, 8, 4, 4, 4, 4, 5, 5, 1, 0), (1, 8, 8, 4, 6, 4, 4, 3, 3, 1, 1), (1, 2, 2, 4, 4, 4, 4, 3, 3, 1, 0),
                (0, 8, 8, 4, 4, 4, 4, 3, 3, 1, 1), (1, 8, 8, 8, 4, 4, 4, 1, 1, 1, 0)):
        assert S.plan(key) is None and S.ws_bytes(key) < 0, key


def test_corpus_and_supplement_reach_every_variant_and_the_supplement_is_needed():
    product = _served(_plans(S.corpus_requests()))
    sup = _plans(S.supplement_requests())
    for (key, purpose, why), (r, p) in zip(S.SUPPLEMENT, sup):
        assert purpose in _served([(r, p)]), ('this supplement entry does not do what it is there for', key, purpose, p)
        assert purpose not in product, ('the product corpus already reaches this: drop the supplement entry', key, purpose)
    purposes = [purpose for _, purpose, _ in S.SUPPLEMENT]
    assert len(set(purposes)) == len(purposes)
    got = product | _served(sup)
    assert {v for k, v in got if k == 'row'} == set(range(S.num_variants()))
    # every reduce width in both slab orders (dense, MFMA-fragment order of the Winograd slabs)
    assert {v for k, v in got if k == 'reduce'} == {(l, f) for l in (2, 8, 32) for f in (0, 1)}
    assert {v for k, v in got if k == 'shrink'} == {'TNB', 'TH', 'TW'}
    # both Winograd geometries, an odd batch in the pairs geometry (a half-empty last pair)
    assert any(p['form'] == 2 and r['key'][0] % 2 for r, p in _plans(S.corpus_requests()))


def test_host_derived_lifter_requests_carry_the_trainers_leading_dimensions():
    keys = {r['key'] for r in S.lifter_requests((7,))}
    assert (7, 1, 1, 66, 68, 1024, 1024, 1, 1, 1, 0) in keys          # input rows padded to 4 floats
    assert (7, 1, 1, 1024, 1024, 96, 96, 1, 1, 1, 0) in keys


# ---------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------
# (key, form the request runs in): K = N Ho Wo from 64 to 12 288, Cin from 3 to 192, odd maps, odd batches
CAL_SHAPES = [
    ((1, 8, 8, 3, 4, 16, 16, 3, 3, 1, 1), 0),             # K 64
    ((3, 13, 11, 66, 68, 66, 68, 3, 3, 1, 1), 0),         # K 429, partial tiles, 48-wide K-sliced
    ((100, 1, 1, 66, 68, 128, 128, 1, 1, 1, 0), 0),       # Linear
    ((2, 32, 32, 96, 96, 192, 192, 3, 3, 2, 1), 0),       # K 512, strided
    ((3, 32, 32, 192, 192, 96, 96, 1, 1, 1, 0), 0),       # K 3072
    ((3, 128, 128, 3, 4, 64, 64, 3, 3, 2, 1), 0),         # K 12 288, the stem
    ((3, 64, 64, 64, 64, 48, 48, 1, 1, 1, 0), 0),         # K 12 288
    ((1, 8, 8, 48, 48, 48, 48, 3, 3, 1, 1), 2),           # K 64
    ((5, 4, 4, 192, 192, 48, 48, 3, 3, 1, 1), 2),         # K 80, every tile at the border
    ((2, 6, 6, 48, 48, 192, 192, 3, 3, 1, 1), 2),         # K 72
    ((1, 8, 8, 192, 192, 192, 192, 3, 3, 1, 1), 2),       # K 64, Cin 192
    ((3, 8, 8, 192, 192, 48, 48, 3, 3, 1, 1), 2),         # odd batch in pairs
    ((3, 12, 20, 48, 48, 96, 96, 3, 3, 1, 1), 1),         # K 720, partial tiles
    ((2, 32, 32, 96, 96, 48, 48, 3, 3, 1, 1), 1),         # K 2048
    ((3, 64, 64, 48, 48, 48, 48, 3, 3, 1, 1), 1),         # K 12 288
]


def _measure():
    """[(key, form, K, honest ratio, {slip: ratio}, {slip: accepted by the old max-norm tolerance})]"""
    rows = []
    for key, form in CAL_SHAPES:
        p = S.plan(key)
        assert p is not None and p['form'] == form, (key, form, p)
        gen = torch.Generator().manual_seed(1000 + sum(key))
        x, dy = S.inputs(key, gen)
        want, A = S.reference(key, x, dy)
        ho, wo = S.out_hw(key)
        K = key[0] * ho * wo
        honest, _ = S.worst(S.honest_fp32(key, x, dy, form), want, A, form)
        tol = S.old_tolerance(want, K)
        sl, old = {}, {}
        for name, wrong in S.slips(key, x, dy, want).items():
            sl[name], _ = S.worst(wrong, want, A, form)
            old[name] = bool(float((wrong - want).abs().max()) <= tol)
        rows.append((key, form, K, honest, sl, old))
    return rows


_MEASURED = None


def measured():
    global _MEASURED
    if _MEASURED is None:
        _MEASURED = _measure()
    return _MEASURED


def calibration_table():
    for key, form, K, honest, sl, old in measured():
        print('%-46s %-15s K %5d  honest %6.2f  /sqrtK %6.3f  /logK %6.3f' % (key, S.FORM_NAMES[form], K, honest,
                                                                              honest / math.sqrt(K), honest / math.log(K)))
        for name in sl:
            print('      %-52s %10.1f   old tolerance %s' % (name, sl[name], 'ACCEPTS' if old[name] else 'rejects'))


def test_bound_passes_honest_fp32_and_rejects_slips():
    seen = set()
    for key, form, K, honest, sl, old in measured():
        C = S.C_BOUND[form]
        # honest fp32 sits about 4x inside the bound (the margin is for MFMA's rounding order)
        assert honest <= C / 3.0, (key, S.FORM_NAMES[form], honest, C)
        for name, r in sl.items():
            assert r > C, ('the bound accepts a slip', key, S.FORM_NAMES[form], name, r, C)
            seen.add((form > 0, name.split(' of ')[0]))
    # every slip was exercised in both the direct and the Winograd form (taps transposed: the stem is 3x3 too)
    names = {n for _, n in seen}
    assert len(names) == 7, names
    assert all((f, n) in seen for f in (False, True) for n in names)


def test_old_max_norm_tolerance_accepts_a_slip_the_bound_rejects():
    """What the element-wise bound adds over test_conv_wgrad's tolerance 2e-6 max|dw| max(1, sqrt(K)/8): on the same
    inputs the old tolerance accepts operands rounded to TF32 in the 16 lowest-scale output channels, on every direct
    layer of the calibration list; it rejects the other slips (recorded beside wgrad_sweep.C_BOUND)."""
    name = 'tf32 operands in the low-scale co block'
    direct = [(sl, old) for _, form, _, _, sl, old in measured() if form == 0 and name in old]
    assert len(direct) >= 5
    for sl, old in direct:
        assert old[name] and sl[name] > S.C_BOUND[0]


if __name__ == '__main__':
    calibration_table()
