"""Inference plans without a GPU (egonet_amd/plan.py, csrc/plan.cpp): what export_plan writes is what the engine's own
recorder, planner and call log say; pieces are stored once; egn_plan_open refuses every damaged file with its error code;
the parser survives 20 000 mutated files under AddressSanitizer / UBSan as a stand-alone program; egn_box_to_crop_f64
gives modify_bbox's and forward_affines' float64 bits."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from egonet_amd import _lib, configs, engine, plan, synth
from egonet_amd.common import crop_gpu, img_proc
from egonet_amd.model.egonet import EgoNet

SIZES = (1, 4)
E = dict(TRUNCATED=-11, MAGIC=-12, VERSION=-13, FINGERPRINT=-14, CRC=-15, COUNT=-16, OP=-17, SLOT=-18, REF=-19, WAIT=-20,
         FORMAT=-21)
# the recorder's op names -> OpKind of csrc/program.hip
KIND = {'conv': 1, 'fuse': 2, 'to_nhwc': 3, 'to_nchw': 4, 'ramps': 5, 'decode': 6, 'fork': 7, 'join': 8, 'pixshuf': 9,
        'pwpair': 10, 'convpair': 11, 'convh': 12, 'convh2': 13, 'convhx': 14}


def make_ego(head='coordinates', J=33, **kw):
    cfg = configs.tiny_config(head, num_joints=J, **kw)
    ego = EgoNet(cfg, pre_trained=False)
    ego.HC.load_state_dict(synth.synth_state_dict(ego.HC.state_dict(), seed=6))
    ego.L.load_state_dict(synth.synth_state_dict(ego.L.state_dict(), seed=7))
    ego.LS = synth.synth_lifter_stats(2 * J, (J - 1) * 3, seed=1)
    return ego.eval()


@pytest.fixture(scope='module')
def exported(tmp_path_factory):
    ego = make_ego()          # (a CPU model and device=None: nothing below touches a GPU)
    path = str(tmp_path_factory.mktemp('plan') / 'tiny.egnplan')
    plan.export_plan(ego, path, batch_sizes=SIZES, device=None)
    with open(path, 'rb') as f:
        data = f.read()
    return ego, path, data


# ---------------------------------------------------------------------------
# 1. structure
# ---------------------------------------------------------------------------
def own_record(name, args_list, lane, tag_call, deps_call):
    """The canonical op record, packed here from the raw logged calls (not by plan.encode_op)."""
    ints, refs = [], []
    for a in args_list:
        for v in (a if isinstance(a, list) else [a]):
            (refs if isinstance(v, _lib.Ref) else ints).append(v)
    signal, waits = (deps_call[0], list(deps_call[1])) if deps_call else (0, [])
    tag, flops, nbytes = tag_call if tag_call else (b'', 0.0, 0.0)
    out = struct.pack('<4I', plan.KIND_OF_CALL[name], lane, signal, len(waits)) + struct.pack('<%dI' % len(waits), *waits)
    out += struct.pack('<I', len(ints)) + b''.join(struct.pack('<i', v) for v in ints)
    out += struct.pack('<I', len(refs)) + b''.join(struct.pack('<iq', r.slot, r.off) for r in refs)
    return out + struct.pack('<ddI', flops, nbytes, len(tag)) + tag


def records_of_log(log):
    recs, lane, k = [], 0, 0
    while k < len(log):
        name, args = log[k]
        k += 1
        if name == 'egn_program_set_lane':
            lane = args[0]
            continue
        tag = deps = None
        if name in ('egn_program_fork', 'egn_program_join'):
            lane = 0
        while k < len(log) and log[k][0] in ('egn_program_tag', 'egn_program_set_deps'):
            if log[k][0] == 'egn_program_tag':
                tag = log[k][1]
            else:
                deps = log[k][1]
            k += 1
        recs.append(own_record(name, args, lane, tag, deps))
    return recs


def test_structure(exported):
    ego, path, _ = exported
    P = plan.Plan(path)
    i, L = P.info, _lib.lib()
    assert (i['J'], i['C'], i['H'], i['W'], i['head_type'], i['decode'], i['precision']) == \
        (33, 3, 64, 64, 'coordinates', 'coords', 'f32')
    assert i['batch_sizes'] == SIZES and i['n_programs'] == 2 * len(SIZES)
    assert (i['lifter_in'], i['lifter_out'], i['ld_in'], i['mul'], i['arch']) == (66, 96, 68, (64.0, 64.0), 'gfx950')
    assert i['lib_version'] == L.egn_version() and i['fingerprint'] == L.egn_conv_table_fingerprint()
    assert i['format_version'] == plan.FORMAT_VERSION and 'lanes=1' in i['switches']
    for k in plan.LS_KEYS:
        assert i['LS'][k].tobytes() == np.asarray(ego.LS[k], dtype=np.float64).reshape(-1).tobytes()
    for s, n in enumerate(SIZES):
        rec, nslots, shapes = ego.HC._hip_engine()._record(n, 3, 64, 64, None)
        assert i['map_size'] == tuple(shapes['maps'][2:])
        lrec = ego.L._hip_engine()._record(n, 68)
        for ptype, r, nuser in ((0, rec, nslots), (1, lrec, 2)):
            got = P.program_info(2 * s + ptype)
            log = []
            engine.Program(r, None, nuser, log=log, native=False)
            assert (got['type'], got['n']) == (ptype, n)
            assert got['n_ops'] == len(r.ops) and got['kinds'] == [KIND[kind] for kind, _ in r.ops]
            assert got['arena_bytes'] == r.plan_arena() and got['weight_bytes'] == r.blob_off
            want = records_of_log(log)
            assert len(want) == got['n_ops']
            for k, w in enumerate(want):
                assert P.op_record(2 * s + ptype, k) == w, (ptype, n, k)
    P.close()


# ---------------------------------------------------------------------------
# 2. pieces
# ---------------------------------------------------------------------------
def test_pieces_are_stored_once(exported, tmp_path):
    ego, path, _ = exported
    contents = set()
    for n in SIZES:
        progs, _ = plan.record_programs(ego, n, None, None, engine.pack_for_kind)
        for ptype, r, roles, ops, arena_bytes, weight_bytes in progs:
            contents |= {t.detach().float().contiguous().numpy().tobytes() for t in r.blobs}
    P = plan.Plan(path)
    assert P.info['n_pieces'] == len(contents)
    twice = str(tmp_path / 'twice.egnplan')
    plan.export_plan(ego, twice, batch_sizes=(1, 4, 4), device=None)
    Q = plan.Plan(twice)
    assert Q.info['n_programs'] == 6 and Q.info['n_pieces'] == P.info['n_pieces']
    # ... and the sizes share what does not depend on the batch: fewer pieces than placements
    assert os.path.getsize(twice) - os.path.getsize(path) < 64 * 1024
    P.close()
    Q.close()


# ---------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------
def sections(data):
    out, at = [], 12
    while at < len(data):
        tag, length = struct.unpack_from('<IQ', data, at)
        out.append((tag, at + 12, length))
        at += 12 + length + 4
    assert at == len(data)
    return out


def assemble(head12, parts):
    out = [head12]
    for tag, payload in parts:
        out.append(struct.pack('<IQ', tag, len(payload)) + payload + struct.pack('<I', zlib.crc32(payload) & 0xffffffff))
    return b''.join(out)


def parts_of(data):
    return [(tag, bytes(data[off:off + length])) for tag, off, length in sections(data)]


def op_fields(payload):
    """Offsets inside a PROG payload: (offset of the op count, [per op: dict of field offsets])."""
    at = 24
    (nplaces,) = struct.unpack_from('<I', payload, at)
    places_at = at
    at += 4 + 12 * nplaces
    (nuser,) = struct.unpack_from('<I', payload, at)
    at += 4 + 12 * nuser
    nops_at = at
    (nops,) = struct.unpack_from('<I', payload, at)
    at += 4
    ops = []
    for _ in range(nops):
        f = {'start': at}
        kind, lane, signal, nwaits = struct.unpack_from('<4I', payload, at)
        f.update(kind=kind, signal=signal, nwaits_at=at + 12, waits_at=at + 16)
        at += 16 + 4 * nwaits
        (nints,) = struct.unpack_from('<I', payload, at)
        f.update(ints_at=at + 4, nints=nints)
        at += 4 + 4 * nints
        (nrefs,) = struct.unpack_from('<I', payload, at)
        f.update(refs_at=at + 4, nrefs=nrefs)
        at += 4 + 12 * nrefs + 16
        (taglen,) = struct.unpack_from('<I', payload, at)
        at += 4 + taglen
        ops.append(f)
    assert at == len(payload)
    return places_at, nops_at, ops


def code_of(tmp_path, data, name='bad.egnplan'):
    p = str(tmp_path / name)
    with open(p, 'wb') as f:
        f.write(data)
    return plan.open_code(p)


def edited(data, part, fn):
    """``data`` with ``fn(bytearray payload)`` applied to section ``part`` (its return value replaces the payload if it is
    not None); length and CRC repaired."""
    parts = parts_of(data)
    tag, payload = parts[part]
    b = bytearray(payload)
    r = fn(b)
    parts[part] = (tag, bytes(b if r is None else r))
    return assemble(bytes(data[:12]), parts)


def first_prog(data):
    return [k for k, (tag, _, _) in enumerate(sections(data)) if tag == plan.SEC_PROG][0]


def test_valid_file_and_truncations(exported, tmp_path):
    _, path, data = exported
    assert plan.open_code(path) == 0
    assert assemble(data[:12], parts_of(data)) == data          # (the helpers reproduce the writer's bytes)
    cuts = {0, 5, 11, 12, len(data) - 1, len(data) - 3}
    for tag, off, length in sections(data):
        cuts |= {off - 12, off - 7, off, off + length // 2, off + length, off + length + 2}
    for cut in sorted(c for c in cuts if 0 <= c < len(data)):
        assert code_of(tmp_path, data[:cut]) == E['TRUNCATED'], cut


def test_magic_version_fingerprint_crc(exported, tmp_path):
    data = exported[2]
    assert code_of(tmp_path, b'EGNPLAM\0' + data[8:]) == E['MAGIC']
    assert code_of(tmp_path, data[:8] + struct.pack('<I', plan.FORMAT_VERSION + 1) + data[12:]) == E['VERSION']

    def bump(at):
        def fn(b):
            struct.pack_into('<I', b, at, (struct.unpack_from('<I', b, at)[0] + 1) & 0xffffffff)
        return fn
    assert code_of(tmp_path, edited(data, 0, bump(0))) == E['VERSION']           # egn_version() of the writer
    assert code_of(tmp_path, edited(data, 0, bump(4))) == E['FINGERPRINT']
    for tag, off, length in sections(data):
        if length:
            b = bytearray(data)
            b[off + length // 2] ^= 0x40
            assert code_of(tmp_path, bytes(b)) == E['CRC'], tag
        b = bytearray(data)
        b[off + length] ^= 1                        # the CRC itself
        assert code_of(tmp_path, bytes(b)) == E['CRC'], tag


def test_op_kind_slot_ref_extent(exported, tmp_path):
    data = exported[2]
    g = first_prog(data)
    payload = parts_of(data)[g][1]
    _, _, ops = op_fields(payload)
    arena_bytes, weight_bytes = struct.unpack_from('<QQ', payload, 8)
    conv = [f for f in ops if f['kind'] == 1][3]

    def put(at, fmt, *v):
        def fn(b):
            struct.pack_into(fmt, b, at, *v)
        return fn
    assert code_of(tmp_path, edited(data, g, put(ops[5]['start'], '<I', 99))) == E['OP']
    assert code_of(tmp_path, edited(data, g, put(conv['refs_at'], '<i', 50))) == E['SLOT']
    assert code_of(tmp_path, edited(data, g, put(conv['refs_at'] + 12 * 5, '<i', -1))) == E['SLOT']        # y may not be NULL
    assert code_of(tmp_path, edited(data, g, put(conv['refs_at'] + 4, '<q', 1 << 39))) == E['REF']         # past the slot
    assert code_of(tmp_path, edited(data, g, put(conv['refs_at'] + 4, '<q', -256))) == E['REF']
    assert code_of(tmp_path, edited(data, g, put(conv['refs_at'] + 4, '<q', 8))) == E['REF']               # misaligned
    # the offset lies inside the slot, the tensor behind it does not: x and y in the arena, the filter in the weights
    assert code_of(tmp_path, edited(data, g, put(conv['refs_at'] + 4, '<q', arena_bytes - 16))) == E['REF']
    assert code_of(tmp_path, edited(data, g, put(conv['refs_at'] + 12 * 5 + 4, '<q', arena_bytes - 16))) == E['REF']
    assert code_of(tmp_path, edited(data, g, put(conv['refs_at'] + 12 + 4, '<q', weight_bytes - 16))) == E['REF']
    (n0,) = struct.unpack_from('<i', payload, conv['ints_at'])
    assert code_of(tmp_path, edited(data, g, put(conv['ints_at'], '<i', n0 * 4096))) == E['REF']           # N grows the extents
    assert code_of(tmp_path, edited(data, g, put(conv['ints_at'], '<i', 0))) == E['FORMAT']
    # every op's first reference moved to the last 16 bytes of its slot is refused, whatever the kind
    slot_bytes = {0: max(arena_bytes, 256), 1: max(weight_bytes, 256)}
    nuser_at = 24 + 4 + 12 * struct.unpack_from('<I', payload, 24)[0]
    for u in range(struct.unpack_from('<I', payload, nuser_at)[0]):
        slot_bytes[2 + u] = struct.unpack_from('<Q', payload, nuser_at + 4 + 12 * u + 4)[0]
    seen = set()
    for f in ops:
        if f['nrefs'] and f['kind'] not in seen:
            seen.add(f['kind'])
            (slot,) = struct.unpack_from('<i', payload, f['refs_at'])
            assert code_of(tmp_path, edited(data, g, put(f['refs_at'] + 4, '<q', slot_bytes[slot] - 16))) == E['REF'], f['kind']
    assert seen >= {1, 2, 3, 4, 5, 10}


def test_waits(exported, tmp_path):
    data = exported[2]
    g = first_prog(data)
    _, _, ops = op_fields(parts_of(data)[g][1])
    k = [j for j, f in enumerate(ops) if f['kind'] == 1][4]

    def wait_on(op, target, signal_on=None):
        def fn(b):
            f = ops[op]
            struct.pack_into('<I', b, f['nwaits_at'], 1)
            if signal_on is not None:
                struct.pack_into('<I', b, ops[signal_on]['start'] + 8, 1)
            return b[:f['waits_at']] + struct.pack('<I', target) + b[f['waits_at']:]
        return fn
    assert ops[k - 1]['kind'] not in (7, 8)
    assert code_of(tmp_path, edited(data, g, wait_on(k, k - 1, signal_on=k - 1))) == 0           # an earlier op that signals
    assert code_of(tmp_path, edited(data, g, wait_on(k, k - 1))) == E['WAIT']                    # ... that does not
    assert code_of(tmp_path, edited(data, g, wait_on(k, k + 1, signal_on=k + 1))) == E['WAIT']   # a later op
    assert code_of(tmp_path, edited(data, g, wait_on(k, k, signal_on=k))) == E['WAIT']           # itself
    assert code_of(tmp_path, edited(data, g, wait_on(k, 1 << 31))) == E['WAIT']


def test_counts_of_two_to_the_31(exported, tmp_path):
    data = exported[2]
    secs = sections(data)
    g = first_prog(data)
    piec = [k for k, (tag, _, _) in enumerate(secs) if tag == plan.SEC_PIEC][0]
    payload = parts_of(data)[g][1]
    places_at, nops_at, ops = op_fields(payload)
    big = 1 << 31

    def put(at, fmt='<I', v=big):
        def fn(b):
            struct.pack_into(fmt, b, at, v)
        return fn
    head = parts_of(data)[0][1]
    arch_len_at = 8
    ls_at = 8 + 4 + struct.unpack_from('<I', head, 8)[0] + 12 + 24 + 16 + 12
    for part, at in ((g, nops_at), (g, places_at), (g, places_at + 4 + 12 * struct.unpack_from('<I', payload, places_at)[0]),
                     (g, ops[3]['nwaits_at']), (g, ops[3]['ints_at'] - 4), (g, ops[3]['refs_at'] - 4),
                     (piec, 0), (0, arch_len_at), (0, ls_at)):
        assert code_of(tmp_path, edited(data, part, put(at))) == E['COUNT'], (part, at)
    assert code_of(tmp_path, edited(data, piec, put(4, '<Q', big))) == E['COUNT']               # a piece's length
    assert code_of(tmp_path, edited(data, piec, put(4, '<Q', (1 << 64) - 4))) == E['COUNT']


# ---------------------------------------------------------------------------
# 4. the parser alone, sanitized, on 20 000 mutants
# ---------------------------------------------------------------------------
def test_sanitized_parser_survives_mutations(tmp_path):
    ego = make_ego('heatmap', J=3, input_size=(32, 32), width=4)
    path = str(tmp_path / 'fuzz.egnplan')
    plan.export_plan(ego, path, batch_sizes=(1, 2), device=None)
    exe = str(tmp_path / 'plan_fuzz')
    cxx = os.environ.get('CXX', 'c++')
    cmd = [cxx, '-O2', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
           os.path.join(ROOT, 'tests', 'plan_fuzz_main.cpp'), os.path.join(ROOT, 'egonet_amd', 'csrc', 'plan.cpp')]
    # the runtimes inside the program where the compiler can (g++; clang's default): it then runs as it is, whatever
    # else the process' environment loads first
    if subprocess.call(cmd + ['-static-libasan', '-static-libubsan'], stderr=subprocess.DEVNULL, timeout=600) != 0:
        subprocess.check_call(cmd, timeout=600)
    r = subprocess.run([exe, path, '20000', '20240229'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    out, err = r.stdout.decode(), r.stderr.decode()
    print(out)
    assert r.returncode == 0, (r.returncode, err[-4000:])
    assert 'Sanitizer' not in err and 'runtime error' not in err, err[-4000:]
    assert '20000 mutants' in out
    accepted = int(out.split('mutants,')[1].split('accepted')[0])
    assert 0 < accepted < 20000            # (some mutants only touch a tag or a cost figure; most are refused)


# ---------------------------------------------------------------------------
# 5. egn_box_to_crop_f64
# ---------------------------------------------------------------------------
def box_to_crop(boxes, target_ar, out_wh):
    boxes = np.ascontiguousarray(boxes, dtype=np.float64)
    n = len(boxes)
    c, s, m = np.empty((n, 2)), np.empty((n, 2)), np.empty((n, 6))
    _lib.check(_lib.lib().egn_box_to_crop_f64(boxes.ctypes.data, n, float(target_ar), 1.1, int(out_wh[0]), int(out_wh[1]),
                                              c.ctypes.data, s.ctypes.data, m.ctypes.data))
    return c, s, m


@pytest.mark.parametrize('out_wh', [(256, 256), (192, 256), (64, 96)])
def test_box_to_crop_bits(out_wh):
    rng = np.random.RandomState(1234 + out_wh[0])
    x1 = rng.uniform(-60.0, 1200.0, 1000)
    y1 = rng.uniform(-40.0, 360.0, 1000)
    boxes = np.stack([x1, y1, x1 + rng.uniform(2.0, 400.0, 1000), y1 + rng.uniform(2.0, 300.0, 1000)], 1)
    H, W = 130, 240             # the 'edge' case of tests/golden/make_golden_train_samples.py
    edge = np.array([[-35.0, -20.5, 60.25, 48.0], [W - 50.5, H - 30.0, W + 42.0, H + 25.75], [-10.0, 20.0, W + 15.0, 70.0],
                     [W + 5.0, H + 3.0, W + 80.0, H + 60.0]])
    boxes = np.concatenate([boxes, edge])
    target_ar = out_wh[1] / out_wh[0]
    rets = [img_proc.modify_bbox(b, target_ar) for b in boxes]
    want_c = np.stack([r['c'] for r in rets]).astype(np.float64)
    want_s = np.stack([r['s'] for r in rets]).astype(np.float64)
    want_m = crop_gpu.forward_affines(want_c, want_s, out_wh)
    c, s, m = box_to_crop(boxes, target_ar, out_wh)
    assert c.tobytes() == want_c.tobytes() and s.tobytes() == want_s.tobytes() and m.tobytes() == want_m.tobytes()
    assert _lib.lib().egn_box_to_crop_f64(None, 1, 1.0, 1.1, 64, 64, None, None, None) == -1
