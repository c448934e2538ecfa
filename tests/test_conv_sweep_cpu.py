"""Host side of the conv configuration sweep (tests/test_gpu_conv_sweep.py), no GPU: the error bound it applies
separates honest fp32 arithmetic from the slips a kernel makes, and the request corpus is what it claims to be."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_sweep as S
from egonet_amd import _lib, engine, tuner
from tools import wino43_error_study as W
from train_checks import conv_ref64

MATS = {1: W.mats([0.0, 1.0, -1.0]), 3: W.mats([0.0, 1.0, -1.0, 2.0, -2.0])}


def _case(seed, n=2, cin=32, cout=48, hw=16, kh=3, stride=1):
    g = torch.Generator().manual_seed(seed)
    x = S.act_like(n, hw, hw, cin, cin, g).permute(0, 3, 1, 2).contiguous()          # NCHW fp32
    w = S.filt(cout, cin, kh, kh, g)
    sc = torch.where(torch.rand(cout, generator=g) < 0.3, -1.0, 1.0) * (0.5 + torch.rand(cout, generator=g))
    sh = 0.5 * torch.randn(cout, generator=g)
    ho = (hw + 2 * (kh // 2) - kh) // stride + 1
    res = S.act_like(n, ho, ho, cout, cout, g).permute(0, 3, 1, 2).contiguous()
    return x, w, sc, sh, res


def _fp32(kind, x, w, stride, pad):
    """Honest fp32 convolution of a kernel kind: torch's fp32 conv2d (direct) or the Winograd emulation of
    tools/wino43_error_study.py (fp32 transforms, products and sums; filter transform in float64, rounded once)."""
    if kind == 0:
        return F.conv2d(x, w, None, stride, pad).double()
    AT, G, BT = MATS[kind]
    out = [torch.from_numpy(W.conv_wino(np.pad(xi.numpy(), ((0, 0), (1, 1), (1, 1))), w.double().numpy(), AT, G, BT)
                            .astype(np.float64)) for xi in x]
    return torch.stack(out)


def _epilogue32(z, sc, sh, res, act):
    y = z.float() * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1) + res
    return torch.relu(y) if act == engine.ACT_RELU else y


def _worst(kind, y, x, w, stride, pad, sc, sh, res, act):
    x64, w64 = x.double(), w.double()
    want = conv_ref64(x64, w64, stride, pad, sc.double(), sh.double(), res.double(), act)
    A = S.bound_A(x64, w64, stride, pad, sc.double(), sh.double(), res.double(), act)
    return float(S.ratio(y, want, A).max()) / S.C_BOUND[kind]


def _tf32(t):
    b = t.float().contiguous().view(torch.int32)
    return ((b + 0x1000) & ~0x1FFF).view(torch.float32)


MUTATIONS = ['tf32', 'drop_last_chunk', 'row_shift', 'taps_transposed']
SHAPES = {0: [(3, 1), (3, 2), (1, 1)], 1: [(3, 1)], 3: [(3, 1)]}       # (kh, stride) per kind


@pytest.mark.parametrize('kind', [0, 1, 3])
def test_bound_passes_honest_fp32_and_rejects_slips(kind):
    """Honest fp32 sits inside C_BOUND[kind] * 2^-24 * A on every element; each deliberate slip lands outside."""
    for kh, stride in SHAPES[kind]:
        for seed in range(2):
            x, w, sc, sh, res = _case(seed + 10 * kind, kh=kh, stride=stride)
            pad = kh // 2
            act = engine.ACT_RELU

            def run(xx, ww):
                return _epilogue32(_fp32(kind, xx, ww, stride, pad), sc, sh, res, act)
            honest = _worst(kind, run(x, w), x, w, stride, pad, sc, sh, res, act)
            assert honest <= 1.0, (kind, kh, stride, honest)
            for mut in MUTATIONS:
                if mut == 'taps_transposed' and kh == 1:
                    continue                        # (one tap: nothing to transpose)
                if mut == 'tf32':
                    y = run(_tf32(x), _tf32(w))
                elif mut == 'drop_last_chunk':
                    xm = x.clone()
                    xm[:, -16:] = 0
                    y = run(xm, w)
                elif mut == 'row_shift':
                    y = run(x, w).clone()
                    r = y.shape[2] // 2
                    y[:, :, r] = torch.roll(y[:, :, r], 1, dims=-1)
                else:
                    y = run(x, w.transpose(2, 3).contiguous())
                got = _worst(kind, y, x, w, stride, pad, sc, sh, res, act)
                assert got > 1.0, (kind, kh, stride, mut, got, honest)


def test_corpus_is_real_and_without_duplicates():
    reqs = S.inference_requests()
    prs = S.pairs(reqs)
    keys = {(p['key'], p['act'], p['entry'], p['alias'], p['stats'], p['cfg']) for p in prs}
    assert len(keys) == len(prs)
    distinct = {(p['key'], p['act']) for p in prs}
    assert len(distinct) >= 300, len(distinct)
    cfgs = {p['cfg'] for p in prs}
    # the inference programs reach the direct, F(2x2,3x3) and F(4x4,3x3) families, the K split, the stem, the 1x1 row
    # GEMM and the stride-2 kernel
    assert {0, 1, 30, 51, 59, 64, 70, 79, 80, 83, 84, 85, 86} <= cfgs, sorted(cfgs)
    assert any(r['key'][12] for r in reqs)                                        # NCHW head outputs
    assert any(r['act'] & engine.ACT_RES_AFTER for r in reqs)                     # the lifter's residual
    assert any((r['key'][7], r['key'][8]) in ((4, 4), (4, 3)) for r in reqs)     # the valid head convolutions
    assert {70, 20} <= {r['key'][0] for r in reqs}
    for p in prs:                     # a candidate's filter is one the caller can feed, and the planner takes the key
        assert tuner.kind_of(p['cfg']) in p['kinds'] and tuner.usable(p['key'], p['cfg'], p['kinds']), p


_KEY = re.compile(r'n(\d+)_h(\d+)_w(\d+)_ci(\d+)\.(\d+)_co(\d+)\.(\d+)_k(\d+)x(\d+)_s(\d+)_p(\d+)_r(\d+)_o(\d+)$')


def _table():
    """(shape_key arguments, entry) of every shape of the shipped table."""
    tab = tuner._load()
    assert tab
    for key, ent in tab.items():
        m = _KEY.match(key)
        assert m, key
        v = [int(t) for t in m.groups()]
        args = tuple(v[:11]) + (bool(v[11]), bool(v[12]))
        assert tuner.shape_key(*args) == key
        yield args, ent


def test_every_tabled_config_is_a_candidate():
    """Whatever the shipped table can hand out for a shape is a candidate the sweep runs for it (tuner.tune times
    exactly tuner.candidates; tuner._pick falls back to any of them)."""
    for args, ent in _table():
        cand = set(tuner.candidates(args, tuner.ALL_KINDS))
        # (ids retired since the table was measured have kind -1: tuner._pick never returns them)
        ids = {c for c in {int(k) for k in ent.get('ms', {})} | {int(ent['cfg'])} if tuner.kind_of(c) >= 0}
        assert ids and ids <= cand, (args, sorted(ids - cand))


def test_tape_candidates_follow_the_tape_rules():
    """What train_hrnet._Tape._conv_launch tells the tuner: no kind 2, no K split for the in-place residual."""
    key = (8, 16, 16, 192, 192, 192, 192, 3, 3, 1, 1, True, False)
    free = tuner.candidates(key, tuner.TAPE_F43, 1 << 16)
    alias = tuner.candidates(key, tuner.TAPE_F43, 1 << 16, inplace_res=True)
    assert 84 in free and 84 not in alias and set(alias) < set(free)
    assert 84 not in tuner.candidates(key, tuner.TAPE_F43, tuner.ticket_words(key, 84) - 1)     # too few ticket words
    assert all(_lib.lib().egn_conv_config_kind(c) != 2 for c in free if c)
    assert set(tuner.candidates(key, tuner.DIRECT, 1 << 16)) == {c for c in free if tuner.kind_of(c) == 0}


PROFILES = {                                    # what each caller passes to tuner.choose
    'program, plain epilogue': dict(kinds=tuner.ALL_KINDS),
    'program, other epilogue': dict(kinds=tuner.DIRECT),
    'tape forward': dict(kinds=tuner.TAPE_F43, ticket_cap=1 << 16),
    'tape aliased data gradient': dict(kinds=tuner.TAPE_F43, ticket_cap=1 << 16, inplace_res=True),
    'direct only': dict(kinds=tuner.DIRECT),
}


def test_choose_answers_with_a_candidate(monkeypatch):
    """With autotuning off, what ``choose`` hands each kind of caller for each tabled shape is one of ``candidates``
    for that caller -- the set the sweep runs."""
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    for name in ('EGONET_AMD_WINO', 'EGONET_AMD_F43', 'EGONET_AMD_F43_MATCH', 'EGONET_AMD_SKIP_CFG'):
        monkeypatch.delenv(name, raising=False)
    picked = set()
    for args, _ in _table():
        for who, prof in PROFILES.items():
            cfg = tuner.choose('cpu', args, **prof)
            assert cfg in tuner.candidates(args, **prof), (who, args, cfg)
            picked.add((who, tuner.kind_of(cfg)))
    assert ('tape forward', 3) in picked and ('program, plain epilogue', 3) in picked       # (not vacuous)
