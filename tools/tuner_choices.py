#!/usr/bin/env python
"""Print, as JSON, the tile configuration ``tuner.choose`` hands each kind of caller for every shape of the shipped
table and of the inference programs (host only, autotuning off).  Two commits choose alike exactly when their outputs
are the same file:

    python tools/tuner_choices.py > choices.json

On a commit from before ``tuner.usable`` the same questions go through that commit's ``choose(allow_wino, allow_f43)``
and the training tape's staged fall-back of the time, restated in ``_staged`` for that side only.
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
os.environ['EGONET_AMD_AUTOTUNE'] = '0'
for _v in ('EGONET_AMD_WINO', 'EGONET_AMD_F43', 'EGONET_AMD_F43_MATCH', 'EGONET_AMD_SKIP_CFG', 'EGONET_AMD_RETUNE'):
    os.environ.pop(_v, None)

from egonet_amd import _lib, tuner  # noqa: E402

KEY = re.compile(r'n(\d+)_h(\d+)_w(\d+)_ci(\d+)\.(\d+)_co(\d+)\.(\d+)_k(\d+)x(\d+)_s(\d+)_p(\d+)_r(\d+)_o(\d+)$')
TAPE_TICKETS = 1 << 16
PROFILES = {                # (filter kinds, ticket words the caller owns, the residual is y)
    'program plain': ((0, 1, 2, 3), None, False),
    'program direct-only': ((0,), None, False),
    'tape forward': ((0, 1, 3), TAPE_TICKETS, False),
    'tape forward, no F(4x4,3x3)': ((0, 1), TAPE_TICKETS, False),
    'tape aliased data gradient': ((0, 1, 3), TAPE_TICKETS, True),
    'direct only': ((0,), None, False),
}


def _staged(key, kinds, ticket_cap, inplace_res):
    """The parent's rule: two booleans, and for the tape (the caller with ticket words of its own) up to two more
    calls when the answer is a kind it cannot pack or a K split it cannot run."""
    L = _lib.lib()
    wino, f43 = 1 in kinds, 3 in kinds

    def kind_of(cfg):
        return L.egn_conv_config_kind(cfg) if cfg > 0 else 0
    cfg = tuner.choose('cpu', key, allow_wino=wino, allow_f43=f43)
    if ticket_cap is None:
        return cfg
    if kind_of(cfg) == 2:
        cfg = tuner.choose('cpu', key, allow_wino=wino, allow_f43=False)
    if kind_of(cfg) == 3:
        ntk = L.egn_conv2d_ticket_words(*[int(v) for v in key[:11]], cfg)
        if ntk > 0 and (ntk > ticket_cap or inplace_res):
            cfg = tuner.choose('cpu', key, allow_wino=wino, allow_f43=False)
    return cfg


def ask(key, kinds, ticket_cap, inplace_res):
    if hasattr(tuner, 'usable'):
        return tuner.choose('cpu', key, frozenset(kinds), ticket_cap=ticket_cap, inplace_res=inplace_res)
    return _staged(key, kinds, ticket_cap, inplace_res)


def main():
    import conv_sweep
    keys = set()
    for name in tuner._load():
        v = [int(t) for t in KEY.match(name).groups()]
        keys.add(tuple(v[:11]) + (bool(v[11]), bool(v[12])))
    n_table = len(keys)
    reqs = conv_sweep.inference_requests()
    keys |= {r['key'] for r in reqs}
    out = {who: {tuner.shape_key(*k): ask(k, *prof) for k in sorted(keys)} for who, prof in PROFILES.items()}
    # each conv of the inference programs as its program asks for it
    out['inference programs'] = ['%s %s act %d: %d' % (r['src'], tuner.shape_key(*r['key']), r['act'],
                                                       ask(r['key'], sorted(r['kinds']), None, False)) for r in reqs]
    out['_counts'] = dict(table_keys=n_table, keys=len(keys), profiles=len(PROFILES), program_requests=len(reqs),
                          choices=len(keys) * len(PROFILES) + len(reqs))
    json.dump(out, sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write('\n')


if __name__ == '__main__':
    main()
