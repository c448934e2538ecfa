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

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_PATH = os.path.join(_HERE, 'tuned', 'gfx950.json')
_table = None
_tuned_here = {}

# What a caller can feed: the filter kinds (kind_of) it packs.
DIRECT = frozenset((0,))                 # a direct-packed filter only: the GEMM callers, a non-plain epilogue
ALL_KINDS = frozenset((0, 1, 2, 3))      # the inference program (engine.pack_for_kind transforms on the host)
TAPE_WINO, TAPE_F43 = frozenset((0, 1)), frozenset((0, 1, 3))      # the training tape: never kind 2
F43_KINDS = frozenset((2, 3))


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
    return _lib.lib().egn_conv_config_kind(cfg) if cfg > 0 else 0


@functools.lru_cache(maxsize=None)
def _facts(key, cfg):
    """(kind, the planner takes ``key``, ticket words of a K split): what the loaded library says, asked once."""
    L = _lib.lib()
    plans = L.egn_conv_plan_query(*key[:11], int(key[12]), cfg, (C.c_int * 12)()) == 0
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


def choose(device, key, kinds=DIRECT, ticket_cap=None, inplace_res=False):
    """The fastest measured configuration the caller can use (``usable``) for the shape ``key`` (the ``shape_key``
    arguments): the shipped table, else the in-process autotune, else 0.  EGONET_AMD_WINO=0 never returns a Winograd
    configuration, =1 always the F(2x2,3x3) one where one is usable, =43 / =43b / =43w an F(4x4,3x3) one where one is
    (cfg 70 / cfg 80 / cfg 86, conv_wino4w_kernel, first; else F(2x2,3x3)); EGONET_AMD_F43=0 keeps F(4x4,3x3) out."""
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
            for cfg in (list(first) if kind == 3 else []) + ids:
                if kind_of(cfg) == kind and usable(key, cfg, kinds, ticket_cap, inplace_res):
                    return cfg
    name = shape_key(*key)
    only = os.environ.get('EGONET_AMD_F43_MATCH', '')        # debugging: F(4x4,3x3) only for shape keys containing this
    if only and only not in name:
        kinds = kinds - F43_KINDS
    entry = _load().get(name)
    if entry is None:
        if os.environ.get('EGONET_AMD_AUTOTUNE', '1') == '0':
            return 0           # deterministic: the shipped table or the cost model, whatever was tuned earlier
        if name not in _tuned_here:
            cfg, times = tune(device, key)
            _tuned_here[name] = {'cfg': cfg, 'ms': {str(k): round(v, 5) for k, v in times.items()}}
        entry = _tuned_here[name]
    return _pick(entry, key, kinds, ticket_cap, inplace_res)


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
