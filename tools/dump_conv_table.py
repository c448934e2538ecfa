"""Everything the conv config table (csrc/conv_plan.hip: kConfigs) decides, as the host-only entry points report it.

    python tools/dump_conv_table.py OUT.npz [SECTION=LIB.so ...]

Without SECTION=LIB arguments the library that EGONET_AMD_LIB (or the default path) names is dumped into the section
its egn_probe_build() says ('product' / 'probes').  With them, each library is dumped in a child process (a process
loads one library) and the sections are merged: this is how tests/golden/conv_table.npz was made from the product and
the probe build of the commit before the table got named fields.  No GPU is needed.

Per section: for every config id 1..egn_conv_num_configs() its filter kind, tile_m / tile_n and kernel name; for every
shape of shapes() and every id 0..count the return code and the 12 ints of egn_conv_plan_query (id 0: out[0] is the
cost model's choice), egn_conv2d_ticket_words and egn_conv2d_bnstats_rows.  tests/test_conv_table_cpu.py asks the
loaded library the same questions and compares field by field.
"""
import ctypes as C
import itertools
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEY = re.compile(r'n(\d+)_h(\d+)_w(\d+)_ci(\d+)\.(\d+)_co(\d+)\.(\d+)_k(\d+)x(\d+)_s(\d+)_p(\d+)_r(\d+)_o(\d+)$')
PLAN_FIELDS = ('rc', 'cfg', 'wm', 'wn', 'mt', 'nt', 'TH', 'TW', 'TNB', 'tps', 'lds_bytes', 'tiles', 'co_tiles')
SHAPE_FIELDS = ('N', 'H', 'W', 'Cin', 'cs_in', 'Cout', 'cs_out', 'KH', 'KW', 'stride', 'pad', 'out_nchw')


def _sq(n, h, w, cin, cs_in, cout, cs_out, k, s, p, nchw=0):
    return (n, h, w, cin, cs_in, cout, cs_out, k, k, s, p, nchw)


def _test_shapes():
    """The shape tuples of tests/test_planner_r3_cpu.py and tests/test_conv_design_cpu.py."""
    out = [_sq(*t) for t in (
        (64, 64, 64, 48, 48, 48, 48, 3, 1, 1), (2, 256, 256, 3, 4, 64, 64, 3, 2, 1), (2, 256, 256, 3, 4, 48, 48, 3, 2, 1),
        (2, 256, 256, 16, 16, 64, 64, 3, 2, 1), (2, 256, 256, 3, 4, 64, 64, 3, 1, 1), (5, 32, 32, 96, 96, 144, 144, 3, 1, 1),
        (64, 16, 16, 192, 192, 192, 192, 3, 1, 1), (64, 64, 64, 64, 64, 64, 64, 3, 1, 1), (64, 64, 64, 24, 24, 48, 48, 3, 1, 1),
        (64, 64, 64, 48, 48, 48, 48, 3, 2, 1), (64, 64, 64, 48, 52, 48, 48, 3, 1, 1), (64, 64, 64, 48, 48, 48, 48, 1, 1, 0),
        (16, 64, 64, 48, 48, 48, 48, 3, 1, 1), (3, 32, 48, 16, 16, 96, 96, 3, 1, 1), (64, 8, 8, 384, 384, 384, 384, 3, 1, 1),
        (64, 24, 16, 48, 48, 48, 48, 3, 1, 1), (64, 16, 16, 24, 24, 48, 48, 3, 1, 1), (64, 16, 16, 192, 192, 64, 64, 3, 1, 1),
        (64, 16, 16, 192, 192, 192, 192, 3, 2, 1), (64, 1, 1, 1024, 1024, 1024, 1024, 1, 1, 0),
        (64, 1, 1, 1024, 1024, 96, 96, 1, 1, 0, 1), (64, 8, 8, 384, 384, 48, 48, 1, 1, 0), (64, 8, 8, 384, 384, 48, 48, 1, 1, 0, 1),
        (64, 1, 1, 66, 68, 1024, 1024, 1, 1, 0), (64, 64, 64, 48, 48, 33, 33, 1, 1, 0),
        # test_conv_design_cpu.py
        (64, 256, 256, 3, 4, 64, 64, 3, 2, 1), (64, 1, 1, 66, 68, 1024, 1024, 1, 1, 0), (1, 8, 8, 6, 6, 8, 8, 3, 1, 1),
        (64, 64, 64, 48, 48, 96, 96, 3, 1, 1), (64, 64, 64, 96, 96, 48, 48, 3, 1, 1), (64, 64, 64, 48, 48, 48, 48, 3, 1, 1, 1),
        (3, 19, 13, 48, 48, 48, 48, 3, 1, 1), (32, 16, 16, 192, 192, 192, 192, 3, 1, 1), (64, 64, 64, 35, 36, 48, 48, 3, 1, 1),
        (64, 64, 64, 48, 48, 64, 64, 3, 1, 1), (64, 63, 64, 48, 48, 48, 48, 3, 1, 1), (32, 64, 48, 32, 32, 32, 32, 3, 1, 1),
        (8, 8, 8, 256, 256, 256, 256, 3, 1, 1), (8, 16, 16, 80, 80, 80, 80, 3, 1, 1))]
    # its CASES: (N, H, W, Cin, Cout, k, s, p, nchw), channel strides rounded up to 4 (NHWC outputs)
    for n, h, w, cin, cout, k, s, p, nchw in ((2, 8, 8, 20, 24, 3, 1, 1, 0), (1, 9, 7, 16, 16, 3, 2, 1, 0), (3, 4, 4, 6, 10, 4, 1, 0, 1),
                                              (2, 6, 10, 35, 7, 1, 1, 0, 1), (5, 1, 1, 10, 40, 1, 1, 0, 0), (1, 12, 12, 8, 48, 3, 1, 1, 0),
                                              (1, 8, 8, 4, 64, 3, 2, 1, 0)):
        out.append(_sq(n, h, w, cin, (cin + 3) // 4 * 4, cout, cout if nchw else (cout + 3) // 4 * 4, k, s, p, nchw))
    return out


def _edge_shapes():
    """What the decoders branch on, each at N = 1 and N = 5."""
    out = []
    maps = ((8, 8), (16, 16), (16, 32), (24, 16), (32, 48), (7, 8), (8, 7), (15, 16), (16, 31))      # (the last four: Ho / Wo odd)
    for n, (h, w), cout, cin, pin, pout in itertools.product((1, 5), maps, (32, 48, 64, 96, 144), (4, 16, 24, 48), (0, 4),
                                                             (0, 4)):
        out.append(_sq(n, h, w, cin, cin + pin, cout, cout + pout, 3, 1, 1))
    for n in (1, 5):
        for h, w in ((64, 64), (32, 48), (12, 16), (30, 32)):
            for cout in (48, 96, 64):
                out.append(_sq(n, h, w, 48, 48, cout, cout, 3, 2, 1))          # 3x3 stride 2 from the 48-channel branch
        out.append(_sq(n, 256, 256, 3, 4, 64, 64, 3, 2, 1))                   # the stem
        out.append(_sq(n, 64, 64, 4, 4, 64, 64, 3, 2, 1))
        out.append(_sq(n, 63, 64, 3, 4, 64, 64, 3, 2, 1))
        for h in (1, 8):
            for nchw in (0, 1):
                out.append(_sq(n, h, h, 1024, 1024, 96, 96, 1, 1, 0, nchw))   # 1x1 on 1 x 1 and 8 x 8 maps
                out.append(_sq(n, h, h, 48, 48, 33, 33 if nchw else 36, 1, 1, 0, nchw))
    out.append(_sq(128, 512, 512, 32, 32, 32, 32, 3, 1, 1))       # x past the 2 GiB offset limit
    out.append(_sq(64, 256, 256, 16, 16, 144, 144, 3, 1, 1))      # x within it, y past it
    return out


def shapes():
    with open(os.path.join(ROOT, 'egonet_amd', 'tuned', 'gfx950.json')) as f:
        table = json.load(f)
    out = []
    for key in table:
        n, h, w, cin, cs_in, cout, cs_out, kh, kw, s, p, _r, o = (int(v) for v in KEY.match(key).groups())
        out.append((n, h, w, cin, cs_in, cout, cs_out, kh, kw, s, p, o))
    out += _test_shapes() + _edge_shapes()
    return np.array(list(dict.fromkeys(out)), np.int32)      # first occurrence of each, in order


def dump(L, shape_rows=None):
    """{field: array} for the loaded library L (egonet_amd._lib.lib())."""
    sh = shapes() if shape_rows is None else shape_rows
    ncfg = L.egn_conv_num_configs()
    kind = np.array([L.egn_conv_config_kind(c) for c in range(1, ncfg + 1)], np.int32)
    tile = np.zeros((ncfg, 2), np.int32)
    names = []
    buf = C.create_string_buffer(160)
    tm, tn = C.c_int(), C.c_int()
    for c in range(1, ncfg + 1):
        assert L.egn_conv_config_info(c, C.byref(tm), C.byref(tn)) == 0
        tile[c - 1] = tm.value, tn.value
        assert L.egn_conv_config_name(c, buf, 160) == 0
        names.append(buf.value.decode())
    plan = np.zeros((len(sh), ncfg + 1, 13), np.int32)
    tickets = np.zeros((len(sh), ncfg + 1), np.int64)
    bnrows = np.zeros((len(sh), ncfg + 1), np.int64)
    out = (C.c_int * 12)()
    for i, s in enumerate(sh.tolist()):
        for c in range(ncfg + 1):
            C.memset(out, 0, C.sizeof(out))
            plan[i, c, 0] = L.egn_conv_plan_query(*s, c, out)
            plan[i, c, 1:] = out[:]
            tickets[i, c] = L.egn_conv2d_ticket_words(*s[:11], c)
            bnrows[i, c] = L.egn_conv2d_bnstats_rows(*s[:11], c)
    return {'kind': kind, 'tile': tile, 'names': np.array(json.dumps(names)), 'plan': plan, 'tickets': tickets,
            'bnrows': bnrows}


def section_of(L):
    return 'probes' if L.egn_probe_build() else 'product'


def _dump_loaded(path):
    from egonet_amd import _lib
    L = _lib.lib()
    sec = section_of(L)
    np.savez_compressed(path, shapes=shapes(), **{sec + '/' + k: v for k, v in dump(L).items()})
    return sec


if __name__ == '__main__':
    dst, libs = sys.argv[1], sys.argv[2:]
    if not libs:
        print(_dump_loaded(dst), '->', dst)
        sys.exit(0)
    merged = {}
    for spec in libs:
        sec, path = spec.split('=', 1)
        part = dst + '.' + sec + '.npz'
        subprocess.check_call([sys.executable, os.path.abspath(__file__), part],
                              env=dict(os.environ, EGONET_AMD_LIB=os.path.abspath(path)))
        with np.load(part) as z:
            assert any(k.startswith(sec + '/') for k in z.files), (sec, z.files)
            merged.update({k: z[k] for k in z.files})
        os.remove(part)
    np.savez_compressed(dst, **merged)
    print(sorted(merged), '->', dst)
