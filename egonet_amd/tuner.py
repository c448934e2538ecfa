"""Measured choice of the conv tile configuration ("measure, don't guess").

For every distinct convolution shape of a program the engine asks ``choose``:
  1. a shipped table (``tuned/gfx950.json``, measured on MI355X, committed) and
     the in-process cache are consulted;
  2. on a miss -- unless ``EGONET_AMD_AUTOTUNE=0`` -- every configuration
     a caller could be handed (``candidates``) is timed on the real shape
     (scratch tensors, hipEvents on the current stream, min of 5 after 2
     warm-ups) and the fastest is kept;
  3. with autotuning off the library's cost-model planner decides (cfg 0).
Which configuration a given caller can be handed is ``usable``, the one
statement of that rule: ``choose`` answers with the fastest measured usable one.
``EGONET_AMD_TUNE_DUMP=<path>`` writes everything tuned in this process as
JSON at exit (that is how the shipped table is produced).
"""
import atexit
import ctypes as C
import functools
import json
import os

import torch

from . import _lib, filters

_HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_PATH = os.path.join(_HERE, 'tuned', 'gfx950.json')
_table = None
_tuned_here = {}

# What a caller can feed: the filter kinds (kind_of) it packs.
DIRECT = frozenset((filters.DIRECT,))    # a direct-packed filter only: the GEMM callers, a non-plain epilogue
# the inference program (filters.pack_for_kind transforms on the host)
ALL_KINDS = frozenset((filters.DIRECT, filters.WINO2, filters.WINO43, filters.WINO4))
# the training tape: never WINO43
TAPE_WINO, TAPE_F43 = frozenset((filters.DIRECT, filters.WINO2)), frozenset((filters.DIRECT, filters.WINO2, filters.WINO4))
F43_KINDS = frozenset((filters.WINO43, filters.WINO4))


def _load():
    global _table
    if _table is None:
        _table = {}
        if os.path.isfile(TABLE_PATH) and os.environ.get('EGONET_AMD_RETUNE', '0') != '1':
            try:
                with open(TABLE_PATH) as f:
                    _table = {k: v for k, v in json.load(f).items() if not k.startswith('_')}
            except (OSError, ValueError):
                _table = {}
    return _table


def shape_key(n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, out_nchw):
    return 'n%d_h%d_w%d_ci%d.%d_co%d.%d_k%dx%d_s%d_p%d_r%d_o%d' % (
        n, h, w, cin, cs_in, cout, cs_out, kh, kw, stride, pad, int(has_res), int(out_nchw))


def _time_cfg(L, args, cfg, stream, x, w, sc, sh, res, y):
    """One conv of shape ``args`` under configuration ``cfg`` as a ONE-OP PROGRAM -- the way the engine launches it
    (configurations that split a layer over several kernels when called through egn_conv2d_f32 run as one launch inside
    a program: conv_wino4c_kernel's ticket words belong to the program's op).  Min of 5 after 2 warm-ups, ms."""
    n, h, wd, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, out_nchw = args
    prog = C.c_void_p(L.egn_program_create(8))
    if not prog:
        return None
    try:
        refs = []
        for slot, t in enumerate((x, w, sc, sh, res if has_res else None, y)):
            if t is None:
                refs.append(_lib.NULL_REF)
                continue
            if L.egn_program_bind(prog, slot, _lib.ptr(t)) != 0:
                return None
            refs.append(_lib.Ref(slot, 0))
        if L.egn_program_add_conv2d(prog, *refs, n, h, wd, cin, cs_in, cout, cs_out, kh, kw, stride, pad, 1,
                                    int(out_nchw), cfg) != 0:
            return None

        def launch():
            return L.egn_program_run(prog, stream)
        if launch() != 0:
            return None
        launch()
        best = None
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1)
            best = t if best is None or t < best else best
        return best
    finally:
        torch.cuda.synchronize()
        L.egn_program_destroy(prog)


def kind_of(cfg):
    """Filter layout cfg's kernel reads (egn_conv_config_kind; -1: not selectable); the cost model, cfg <= 0: direct."""
    return _lib.lib().egn_conv_config_kind(cfg) if cfg > 0 else filters.DIRECT


@functools.lru_cache(maxsize=None)
def _facts(key, cfg):
    """(kind, the planner takes ``key``, ticket words of a K split): what the loaded library says, asked once."""
    L = _lib.lib()
    plans = L.egn_conv_plan_takes(*key[:11], int(key[11]), int(key[12]), cfg) == 0       # (with the key's residual)
    return kind_of(cfg), plans, L.egn_conv2d_ticket_words(*key[:11], cfg)


def ticket_words(key, cfg):
    """Zeroed words a K-split configuration needs to run ``key`` as one launch (0: not a K split)."""
    return _facts(tuple(key), cfg)[2] if cfg > 0 else 0


def usable(key, cfg, kinds, ticket_cap=None, inplace_res=False):
    """THE rule for which configuration a caller can be handed.  cfg 0 (the cost model) always.  Otherwise the id is
    selectable, the caller packs its filter kind (``kinds``), the planner takes the shape, and -- for a K split -- the
    caller owns enough ticket words (``ticket_cap``; None: a program op allocates its own) and the residual is not the
    output itself (``inplace_res``: the K split writes a raw share into y before the residual is read)."""
    if cfg <= 0:
        return True
    kind, plans, ntk = _facts(tuple(key), cfg)
    return kind in kinds and plans and (ntk <= 0 or (not inplace_res and (ticket_cap is None or ntk <= ticket_cap)))


def candidates(key, kinds, ticket_cap=None, inplace_res=False):
    """Every answer ``choose`` can give this caller for this shape: 0 plus each usable id."""
    return [0] + [cfg for cfg in range(1, _lib.lib().egn_conv_num_configs() + 1)
                  if usable(key, cfg, kinds, ticket_cap, inplace_res)]


def tune(device, args, skip=(), only=None):
    """Time every configuration a caller could be handed for the real shape (except ``skip``; ``only``: just these
    ids); returns (cfg, {cfg: ms})."""
    L = _lib.lib()
    n, h, wd, cin, cs_in, cout, cs_out, kh, kw, stride, pad, has_res, out_nchw = args
    ho = (h + 2 * pad - kh) // stride + 1
    wo = (wd + 2 * pad - kw) // stride + 1
    coutp = (cout + 15) // 16 * 16
    nchunk = (cin + 15) // 16
    with torch.cuda.device(device):
        x = torch.randn(n * h * wd * cs_in, device=device)
        # one buffer serves every packing (random data: only the timing matters); the Winograd kernels read 16
        # (F(2x2,3x3)) / 36 or 48 (F(4x4,3x3), conv_wino4_kernel's padded layout) floats per (co, ci)
        w = torch.randn(max(nchunk * kh * kw * 4 * coutp * 4, cout * cin * 48), device=device) * 0.05
        sc = torch.ones(coutp, device=device)
        sh = torch.zeros(coutp, device=device)
        ny = n * ho * wo * (cout if out_nchw else cs_out)
        y = torch.empty(ny, device=device)
        res = torch.randn(ny, device=device) if has_res else None
        stream = _lib.current_stream(device)
        times = {}
        for cfg in candidates(args, ALL_KINDS)[1:]:
            if cfg in skip or (only is not None and cfg not in only):
                continue
            t = _time_cfg(L, args, cfg, stream, x, w, sc, sh, res, y)
            if t is not None:
                times[cfg] = t
        torch.cuda.synchronize(device)
    return (min(times, key=times.get) if times else 0), times


def _pick(entry, key, kinds, ticket_cap=None, inplace_res=False):
    """A table entry's configuration if the caller can use it, else the fastest measured one it can (0: none)."""
    # EGONET_AMD_SKIP_CFG=86,84: same-box A/B runs of a new configuration against the table without it
    skip = {int(v) for v in os.environ.get('EGONET_AMD_SKIP_CFG', '').split(',') if v.strip()}

    def ok(cfg):
        return cfg not in skip and usable(key, cfg, kinds, ticket_cap, inplace_res)
    cfg = int(entry['cfg'])
    if cfg <= 0 or ok(cfg):
        return cfg
    fit = {int(k): v for k, v in entry.get('ms', {}).items() if ok(int(k))}
    return min(fit, key=fit.get) if fit else 0


def choose(device, key, kinds=DIRECT, ticket_cap=None, inplace_res=False, measure=True):
    """The fastest measured configuration the caller can use (``usable``) for the shape ``key`` (the ``shape_key``
    arguments): the shipped table, else the in-process autotune, else 0.  EGONET_AMD_WINO=0 never returns a Winograd
    configuration, =1 always the F(2x2,3x3) one where one is usable, =43 / =43b / =43w an F(4x4,3x3) one where one is
    (cfg 70 / cfg 80 / cfg 86, conv_wino4w_kernel, first; else F(2x2,3x3)); EGONET_AMD_F43=0 keeps F(4x4,3x3) out.
    ``measure=False`` (an export without a GPU, egonet_amd.plan): the table or 0, never a measurement."""
    key, kinds = tuple(key), frozenset(kinds)
    mode = os.environ.get('EGONET_AMD_WINO', '')
    if os.environ.get('EGONET_AMD_F43', '1') == '0' or mode in ('0', '1'):
        kinds = kinds - F43_KINDS
    if mode == '0':
        kinds = DIRECT
    elif mode in ('1', '43', '43b', '43w'):
        # parity tests pin the kernel families on the same fixtures: the first usable id of the widest family the
        # caller feeds (=43: cfg 70's 16 x 32 regions, cfg 80 for the maps only it plans; =43w: cfg 86, the table's own)
        first = {'43': (70, 80), '43b': (80, 70), '43w': (86, 80, 70)}.get(mode, ())
        ids = list(range(_lib.lib().egn_conv_num_configs(), 0, -1))
        for kind in sorted(kinds - DIRECT, reverse=True):
            for cfg in (list(first) if kind == filters.WINO4 else []) + ids:
                if kind_of(cfg) == kind and usable(key, cfg, kinds, ticket_cap, inplace_res):
                    return cfg
    name = shape_key(*key)
    only = os.environ.get('EGONET_AMD_F43_MATCH', '')        # debugging: F(4x4,3x3) only for shape keys containing this
    if only and only not in name:
        kinds = kinds - F43_KINDS
    entry = _load().get(name)
    if entry is None:
        if not measure or os.environ.get('EGONET_AMD_AUTOTUNE', '1') == '0':
            return 0           # deterministic: the shipped table or the cost model, whatever was tuned earlier
        if name not in _tuned_here:
            cfg, times = tune(device, key)
            _tuned_here[name] = {'cfg': cfg, 'ms': {str(k): round(v, 5) for k, v in times.items()}}
        entry = _tuned_here[name]
    return _pick(entry, key, kinds, ticket_cap, inplace_res)


def tabled_ms(key):
    """What the shipped table measured for the shape ``key`` under the configuration it names (ms; 0.0 where the table
    has no entry or no time): the recorder's estimate of when a chain of convs is done.  Never tunes."""
    entry = _load().get(shape_key(*key))
    if not entry:
        return 0.0
    ms = entry.get('ms', {})
    return float(ms.get(str(entry.get('cfg')), min(ms.values()) if ms else 0.0))


# ---------------------------------------------------------------------------
# paired launches: two independent 3x3 convolutions as one op (csrc/conv_wino4.hip, conv_wino4_pair_kernel)
# ---------------------------------------------------------------------------
PAIRS_PATH = os.path.join(_HERE, 'tuned', 'gfx950_pairs.json')
PAIR_CFGS = (86, 82)          # the single-convolution forms of the pair's two shares
PAIR_DEFAULT = '0'            # EGONET_AMD_PAIR when unset
_pairs = None


def _load_pairs():
    global _pairs
    if _pairs is None:
        _pairs = {}
        try:
            with open(PAIRS_PATH) as f:
                _pairs = {k: v for k, v in json.load(f).items() if not k.startswith('_')}
        except (OSError, ValueError):
            _pairs = {}
    return _pairs


def pair_key(key_a, key_b):
    return shape_key(*key_a) + '+' + shape_key(*key_b)


def pair_plans(key_a, key_b, cus=256):
    """(blocks on a, blocks on b) of the paired launch on a chip of ``cus`` compute units, None where the library's
    planner refuses the two shapes (egn_conv_pair_plan_query; no GPU needed)."""
    if any(tuple(k[7:11]) != (3, 3, 1, 1) or k[3] != k[4] or k[5] != k[6] or k[12] for k in (key_a, key_b)):
        return None
    out = (C.c_int * 2)()
    rc = _lib.lib().egn_conv_pair_plan_query(*key_a[:4], key_a[5], *key_b[:4], key_b[5], cus, 0, 0, out)
    return (out[0], out[1]) if rc == 0 else None


def pair_usable(key_a, key_b):
    """THE rule for running convolutions ``key_a`` and ``key_b`` (``shape_key`` arguments) as one paired launch
    (engine._Recorder.conv_pair).  Measured like every other choice: the pair is used where tuned/gfx950_pairs.json
    (``tune_pair``: the pair op as a one-op program against the sum of the two tabled singles) says it won -- a shape
    without an entry is not paired.  EGONET_AMD_PAIR=1 pairs by that table, =force wherever the planner takes the shapes
    (tests), =0 never.  The default is 0 (PAIR_DEFAULT; DESIGN 3.2d says why and what was measured).  Anything that
    keeps config 86 or 82 away from a caller keeps the pair away too: EGONET_AMD_SKIP_CFG naming one of them, any
    EGONET_AMD_WINO forcing, EGONET_AMD_F43=0."""
    key_a, key_b = tuple(key_a), tuple(key_b)
    mode = os.environ.get('EGONET_AMD_PAIR', PAIR_DEFAULT)
    if mode == '0' or os.environ.get('EGONET_AMD_WINO', '') or os.environ.get('EGONET_AMD_F43', '1') == '0':
        return False
    skip = {int(v) for v in os.environ.get('EGONET_AMD_SKIP_CFG', '').split(',') if v.strip()}
    if skip & set(PAIR_CFGS):
        return False
    if mode != 'force':
        entry = _load_pairs().get(pair_key(key_a, key_b))
        if entry is None or not entry.get('pair'):
            return False
    return pair_plans(key_a, key_b) is not None


def _time_program(L, build, stream):
    """Min of 5 after 2 warm-ups, ms, of the program ``build(prog)`` records (None: it refused)."""
    prog = C.c_void_p(L.egn_program_create(16))
    if not prog:
        return None
    try:
        if not build(prog) or L.egn_program_run(prog, stream) != 0:
            return None
        L.egn_program_run(prog, stream)
        best = None
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.egn_program_run(prog, stream)
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1)
            best = t if best is None or t < best else best
        return best
    finally:
        torch.cuda.synchronize()
        L.egn_program_destroy(prog)


def tune_pair(device, key_a, key_b):
    """Time the pair op as a one-op program against the two TABLED singles (``choose``), each a one-op program; the
    entry for tuned/gfx950_pairs.json: pair = it beat their sum."""
    L = _lib.lib()
    key_a, key_b = tuple(key_a), tuple(key_b)
    with torch.cuda.device(device):
        stream = _lib.current_stream(device)
        halves, singles = [], {}
        for which, key in (('a', key_a), ('b', key_b)):
            n, h, w, cin, _, cout = key[:6]
            t = dict(x=torch.randn(n * h * w * cin, device=device), w=torch.randn(cout * cin * 48, device=device) * 0.05,
                     sc=torch.ones(cout, device=device), sh=torch.zeros(cout, device=device),
                     res=torch.randn(n * h * w * cout, device=device) if key[11] else None,
                     y=torch.empty(n * h * w * cout, device=device))
            halves.append(t)
            cfg = choose(device, key, ALL_KINDS)
            singles[which] = (cfg, _time_cfg(L, key, cfg, stream, t['x'], t['w'], t['sc'], t['sh'], t['res'], t['y']))

        def build(prog):
            args, slot = [], 0
            for t, key in zip(halves, (key_a, key_b)):
                for name in ('x', 'w', 'sc', 'sh', 'res', 'y'):
                    if t[name] is None:
                        args.append(_lib.NULL_REF)
                        continue
                    if L.egn_program_bind(prog, slot, _lib.ptr(t[name])) != 0:
                        return False
                    args.append(_lib.Ref(slot, 0))
                    slot += 1
                args += [key[0], key[1], key[2], key[3], key[5], 1]
            return L.egn_program_add_conv2d_pair(prog, *(args + [0])) == 0
        t_pair = _time_program(L, build, stream)
    ta, tb = singles['a'][1], singles['b'][1]
    won = t_pair is not None and ta is not None and tb is not None and t_pair < ta + tb
    return {'pair': bool(won), 'ms': {'pair': None if t_pair is None else round(t_pair, 5),
                                      'a_cfg%d' % singles['a'][0]: None if ta is None else round(ta, 5),
                                      'b_cfg%d' % singles['b'][0]: None if tb is None else round(tb, 5)}}


def tuned_in_process():
    return dict(_tuned_here)


def _dump():
    path = os.environ.get('EGONET_AMD_TUNE_DUMP')
    if path and _tuned_here:
        merged = dict(_load())
        merged.update(_tuned_here)
        try:
            with open(path, 'w') as f:
                json.dump(merged, f, indent=0, sort_keys=True)
        except OSError:
            pass


atexit.register(_dump)
