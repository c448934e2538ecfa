"""The recorded program with point-to-point dependencies (EGONET_AMD_DEPS=1: fuse term (i, j) waits for branch j's signal,
no join between a module's branches and its fuse rows), checked without a GPU against a model of what egn_program_run
does with the op list -- written here from the runner's rules, not taken from the recorder:

  * lane 0, FORK and JOIN are issued on the caller's stream, lane k > 0 on side stream k: stream order;
  * the first op of a side lane behind a FORK or JOIN waits for the latest FORK;
  * a JOIN waits for the last op of every side lane used since the last FORK / JOIN;
  * an op waits for every op its ``waits`` name.

Every read must be reachable from the last write of its buffer, any two ops that touch overlapping arena bytes (one of
them writing) must be ordered, and ``_Recorder.happens_before`` may claim nothing the model does not give.
EGONET_AMD_DEPS=0 must record the program as it was before dependencies existed (tests/golden/program_ops_joined.json:
kind, lane, region and tag of every op, the same list at 1 and 64 crops).
"""
import itertools
import json
import os

import pytest

from egonet_amd import configs, engine
from egonet_amd.model.heatmapModel import hrnet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'program_ops_joined.json')
CASES = [(m, n) for m in ('w48', 'tiny') for n in (1, 64)]
_cache = {}


def _record(model, n, deps):
    key = (model, n, deps)
    if key not in _cache:
        saved = {k: os.environ.get(k) for k in ('EGONET_AMD_DEPS', 'EGONET_AMD_DEPS_MIN_N', 'EGONET_AMD_PAIR',
                                                'EGONET_AMD_AUTOTUNE')}
        # (EGONET_AMD_DEPS_MIN_N=1: the dependency recording at every batch size, also below the default threshold)
        os.environ.update(EGONET_AMD_DEPS=deps, EGONET_AMD_DEPS_MIN_N='1', EGONET_AMD_PAIR='0', EGONET_AMD_AUTOTUNE='0')
        try:
            cfg, size = (configs.w48_config('heatmap'), 256) if model == 'w48' else (configs.tiny_config('heatmap'), 64)
            net = hrnet.get_pose_net(cfg, is_train=False).eval()
            rec = engine.HRNetEngine(net)._record(n, 3, size, size, 1)[0]
            rec.arena_bytes = rec.plan_arena()
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        _cache[key] = rec
    return _cache[key]


def _reads_writes(kind, op):
    """(buffers read, buffers written) of a recorded op; external tensors (Ref) are not buffers."""
    if kind in ('conv', 'convh', 'convhx'):
        rd, wr = [op['x'], op.get('res')], [op['y']]
    elif kind == 'convh2':
        rd, wr = [op['x']], [op['y']]
    elif kind == 'convpair':
        rd = [h[k] for h in (op['a'], op['b']) for k in ('x', 'res')]
        wr = [op['a']['y'], op['b']['y']]
    elif kind == 'fuse':
        rd, wr = [t for t, _ in op['terms']], [op['y']]
    elif kind == 'pwpair':
        rd, wr = [op['h'], op['res']], [op['out'], op['hn']]
    elif kind in ('to_nhwc', 'ramps'):
        rd, wr = [], [op['y']]
    elif kind in ('to_nchw', 'pixshuf'):
        rd, wr = [op['x']], []
    else:
        assert kind in ('fork', 'join', 'decode'), kind
        rd, wr = [], []
    keep = lambda bs: [b for b in bs if isinstance(b, engine.Buf)]
    return keep(rd), keep(wr)


def _runner_order(rec):
    """before[d]: bit set of the ops that are complete before op d starts, by the runner's rules (module docstring)."""
    before = []
    last_on = {}                 # stream (0 = caller's, k = side stream k) -> last op issued on it
    used = set()                 # side lanes with an op since the last FORK / JOIN
    fork = None
    forked = False               # (before the first FORK there are no side streams: every op runs on the caller's)
    for i, (kind, op) in enumerate(rec.ops):
        preds = []
        if kind == 'fork':
            stream, fork, forked, used = 0, i, True, set()
        elif kind == 'join':
            stream = 0
            preds += [last_on[k] for k in used]
            used = set()
        else:
            stream = op['lane'] if forked else 0
            if stream > 0 and stream not in used:
                preds.append(fork)
                used.add(stream)
            preds += list(op.get('waits', ()))
        if stream in last_on:
            preds.append(last_on[stream])
        m = 0
        for p in preds:
            assert p < i
            m |= before[p] | (1 << p)
        before.append(m)
        last_on[stream] = i
    return before


@pytest.mark.parametrize('model,n', CASES)
def test_every_read_follows_its_write_and_shared_bytes_are_ordered(model, n):
    rec = _record(model, n, '1')
    before = _runner_order(rec)
    done = lambda u, d: bool((before[d] >> u) & 1)
    writer, touch = {}, {}
    for i, (kind, op) in enumerate(rec.ops):
        rd, wr = _reads_writes(kind, op)
        for b in rd:
            assert id(b) in writer, (op.get('tag'), b.name)
            assert done(writer[id(b)], i), (op.get('tag'), b.name)
            assert rec.happens_before(writer[id(b)], i), (op.get('tag'), b.name)
            touch.setdefault(id(b), []).append((i, False))
        for b in wr:
            for u, _ in touch.get(id(b), []):            # (ramps writes into head1's tensor: a second writer)
                assert done(u, i), (op.get('tag'), b.name)
            writer[id(b)] = i
            touch.setdefault(id(b), []).append((i, True))
    bufs = [b for b in rec.bufs if b.slot == engine.SLOT_ARENA and b.first >= 0]
    assert all(b.off + b.nbytes <= rec.arena_bytes for b in bufs)
    shared = 0
    for a, b in itertools.combinations(bufs, 2):
        if a.off < b.off + b.nbytes and b.off < a.off + a.nbytes:
            shared += 1
            for (u, wu), (v, wv) in itertools.product(touch[id(a)], touch[id(b)]):
                if wu or wv:
                    assert done(u, v) or done(v, u), (a.name, b.name, rec.ops[u][1].get('tag'), rec.ops[v][1].get('tag'))
    assert shared > 0
    # the recorder's relation is the arena planner's only rule: it may not claim an order the runner does not give
    nops = len(rec.ops)
    launches = [i for i, (k, _) in enumerate(rec.ops) if k not in ('fork', 'join')]
    for u, d in itertools.product(launches, launches):
        if u != d and rec.happens_before(u, d):
            assert done(u, d), (u, d, rec.ops[u][1].get('tag'), rec.ops[d][1].get('tag'))
    assert nops == len(before)


@pytest.mark.parametrize('model,n', CASES)
def test_waits_name_earlier_signals_and_terms_wait_for_their_branch(model, n):
    rec = _record(model, n, '1')
    nwaits = 0
    for i, (kind, op) in enumerate(rec.ops):
        for w in op.get('waits', ()):
            nwaits += 1
            assert 0 <= w < i and rec.ops[w][1].get('signal') and rec.ops[w][0] not in ('fork', 'join'), (i, w)
            # a term conv (i, j) waits for the last op of branch j of its module, on another lane
            src = rec.ops[w][1]
            mod = op['tag'].split('.fuse')[0]
            assert src['tag'].startswith(mod + '.branches.') and src['lane'] != op['lane'], (op['tag'], src['tag'])
            if '.fuse_layers.' in op['tag']:
                assert src['tag'].startswith('%s.branches.%s.' % (mod, op['tag'].split('.')[4])), (op['tag'], src['tag'])
        assert kind not in ('fork', 'join') or not op.get('signal')
    assert nwaits > 0
    kinds = [k for k, _ in rec.ops]
    # one fork and one join per stage with more than one branch: a stage is one region
    assert kinds.count('fork') == kinds.count('join') == 3


@pytest.mark.parametrize('model,n', CASES)
def test_deps_off_records_the_joined_program_and_deps_on_the_same_launches(model, n):
    rec0, rec1 = _record(model, n, '0'), _record(model, n, '1')
    with open(GOLDEN) as f:
        want = json.load(f)[model]
    assert [[k, op['lane'], op['region'], op.get('tag', '')] for k, op in rec0.ops] == want
    assert not any(op.get('waits') or op.get('signal') for _, op in rec0.ops)
    launch = lambda rec: sorted((k, op['tag'], op['lane']) for k, op in rec.ops if k not in ('fork', 'join'))
    assert launch(rec0) == launch(rec1)                      # the same ops on the same lanes, in another order
    gone = len(rec0.ops) - len(rec1.ops)
    forks = lambda rec: sum(1 for k, _ in rec.ops if k in ('fork', 'join'))
    assert gone == forks(rec0) - forks(rec1) and gone > 0
    # a fuse op takes its terms in the reference's order whatever the launch order of the term convs
    fuse = lambda rec: {op['tag']: [(t.name, s) for t, s in op['terms']] for k, op in rec.ops if k == 'fuse'}
    assert fuse(rec0) == fuse(rec1)
    assert rec1.arena_bytes >= rec0.arena_bytes


def test_rows_start_with_the_branch_expected_first():
    """W48 at 64 crops: the shipped table has every branch conv, so the expected finish times differ and a row's terms
    are recorded in ascending order of them (ties by j)."""
    from egonet_amd import tuner
    rec = _record('w48', 64, '1')
    eta = {}
    for k, op in rec.ops:
        if k == 'conv' and '.branches.' in op['tag']:
            parts = op['tag'].split('.')
            key = (parts[0] + '.' + parts[1], int(parts[3]))
            eta[key] = eta.get(key, 0.0) + tuner.tabled_ms(engine.Program._conv_key(op))
    assert all(v > 0 for v in eta.values())
    rows = {}
    for k, op in rec.ops:
        if k == 'conv' and '.fuse_layers.' in op['tag']:
            parts = op['tag'].split('.')
            seq = rows.setdefault((parts[0] + '.' + parts[1], int(parts[3])), [])
            if int(parts[4]) not in seq:
                seq.append(int(parts[4]))
    assert rows
    for (mod, i), seq in rows.items():
        assert seq == sorted(seq, key=lambda j: (eta[(mod, j)], j)), (mod, i, seq)


def test_set_deps_refuses_anything_but_an_earlier_signal():
    """egn_program_set_deps on a hand-built program (building needs no GPU): the op itself, a later index, an op that does
    not signal and a fork are EGN_E_BADARG (-1), so waits cannot form a cycle; before any op it is EGN_E_STATE (-3)."""
    import ctypes as C
    from egonet_amd import _lib
    L = _lib.lib()
    prog = C.c_void_p(L.egn_program_create(2))
    ints = lambda *v: (C.c_int * len(v))(*v)
    try:
        assert L.egn_program_set_deps(prog, 1, None, 0) == -3
        assert L.egn_program_fork(prog) == 0                                                # op 0
        assert L.egn_program_set_deps(prog, 1, None, 0) == -1
        assert L.egn_program_set_lane(prog, 1) == 0
        assert L.egn_program_add_ramps(prog, _lib.Ref(0, 0), 1, 4, 4, 4, 1) == 0            # op 1: signals
        assert L.egn_program_set_deps(prog, 1, None, 0) == 0
        assert L.egn_program_add_ramps(prog, _lib.Ref(0, 256), 1, 4, 4, 4, 1) == 0          # op 2: does not
        assert L.egn_program_set_lane(prog, 0) == 0
        assert L.egn_program_add_ramps(prog, _lib.Ref(0, 512), 1, 4, 4, 4, 1) == 0          # op 3
        for bad in (3, 4, 7, -1, 2, 0):
            assert L.egn_program_set_deps(prog, 0, ints(bad), 1) == -1, bad
        assert L.egn_program_set_deps(prog, 0, ints(1, 3), 2) == -1
        assert L.egn_program_set_deps(prog, 0, ints(1), 1) == 0
        assert L.egn_program_num_ops(prog) == 4
    finally:
        L.egn_program_destroy(prog)


def test_a_recorder_without_signal_is_recorded_with_the_joins():
    """The training tape brings a recorder of its own: no ``signal``, no ``ops`` list.  ``_module`` must ask it for
    nothing but the calls it has always made, and keep the join between the branches and the fuse rows."""
    class Tape(object):
        def __init__(self):
            self._r = engine._Recorder()
            for name in ('fork', 'join', 'lane', 'conv', 'fuse', 'new', 'nchw_to_nhwc', 'decode'):
                setattr(self, name, getattr(self._r, name))
    tape = Tape()
    net = hrnet.get_pose_net(configs.tiny_config('heatmap'), is_train=False).eval()
    engine.HRNetEngine(net)._record(2, 3, 64, 64, 1, r=tape)
    kinds = [k for k, _ in tape._r.ops]
    assert kinds.count('fork') == kinds.count('join') == 6           # branches and fuse rows of three modules
    assert not any(op.get('waits') or op.get('signal') for _, op in tape._r.ops)


def test_small_batches_keep_the_joins_by_default(monkeypatch):
    """The dependency recording starts at EGONET_AMD_DEPS_MIN_N crops (default 16: the smallest batch measured without
    any regression); below it the default records the joined program."""
    for k in ('EGONET_AMD_DEPS', 'EGONET_AMD_DEPS_MIN_N', 'EGONET_AMD_PAIR'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('EGONET_AMD_AUTOTUNE', '0')
    with open(GOLDEN) as f:
        want = json.load(f)['w48']
    net = hrnet.get_pose_net(configs.w48_config('heatmap'), is_train=False).eval()
    for n, deps in ((1, False), (2, False), (15, False), (16, True), (64, True)):
        rec = engine.HRNetEngine(net)._record(n, 3, 256, 256, 1)[0]
        assert any(op.get('waits') for _, op in rec.ops) == deps, n
        if not deps:
            assert [[k, op['lane'], op['region'], op.get('tag', '')] for k, op in rec.ops] == want, n
