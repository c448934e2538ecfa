"""Inference plans: write the planned, tuned and packed network of ``EgoNet.infer_crops(refine=None)`` to one file
(``export_plan``) and run it from that file with nothing but the shared library (``Plan``; from C: egn_plan_open /
egn_plan_load / egn_plan_infer, include/egonet_hip.h; tools/egonet_run.cpp is a Python-free caller).

A plan holds, per exported batch size, the HRNet and the lifter launch program as THE calls the engine makes -- the log of
``engine.ProgramCalls``, the one place ``Program._emit`` reaches the library through -- the packed filters / folded
BatchNorm vectors as pieces stored once and keyed by content, and the constants of the chain (resolution, lifter
statistics, ...).  DESIGN 3.23 gives the byte layout and what the library validates before it loads a file.

``Plan`` touches no ``nn.Module``: a process that runs a plan builds no model, records nothing, packs no filter and tunes
nothing.  Out of scope: ``refine='pnp'``, ``kpts_x_for_alpha``, the second in-flight copy (``slot=1``) and training.
"""
import ctypes as C
import hashlib
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib

MAGIC = b'EGNPLAN\0'
FORMAT_VERSION = 1
SEC_HEAD, SEC_PIEC, SEC_PROG, SEC_END = 1, 2, 3, 4
ROLE_CROPS, ROLE_MAPS, ROLE_COORDS, ROLE_XY, ROLE_MAX, ROLE_IDX, ROLE_LIFT_IN, ROLE_LIFT_OUT = range(1, 9)
PRECISIONS = ('f32', 'f16', 'f16s2', 'f16x')
HEAD_TYPES = ('coordinates', 'heatmap')
DECODES = ('hard', 'soft', 'coords')
LS_KEYS = ('mean_in', 'std_in', 'mean_out', 'std_out')
# the op kind (OpKind of csrc/program.hip) each building call records
KIND_OF_CALL = {
    'egn_program_add_conv2d': 1, 'egn_program_add_fuse': 2, 'egn_program_add_nchw_to_nhwc': 3,
    'egn_program_add_nhwc_to_nchw': 4, 'egn_program_add_ramps': 5, 'egn_program_add_decode': 6, 'egn_program_fork': 7,
    'egn_program_join': 8, 'egn_program_add_pixel_shuffle': 9, 'egn_program_add_pw_pair': 10,
    'egn_program_add_conv2d_pair': 11, 'egn_program_add_conv3x3_h': 12, 'egn_program_add_conv3x3s2_h': 13,
    'egn_program_add_conv3x3_hx': 14,
}


# ---------------------------------------------------------------------------
# the logged calls -> op records
# ---------------------------------------------------------------------------
def calls_to_ops(log):
    """The ops a log of ``engine.ProgramCalls`` builds: one per egn_program_add_* / fork / join call, with the lane set
    before it and the tag / dependencies set behind it.  An op is a dict kind, lane, signal, waits, ints, refs (slot,
    offset), flops, bytes, tag -- ints and refs in the order of the call's arguments."""
    ops, lane = [], 0
    for name, args in log:
        if name == 'egn_program_set_lane':
            lane = int(args[0])
        elif name == 'egn_program_tag':
            ops[-1].update(tag=bytes(args[0]), flops=float(args[1]), bytes=float(args[2]))
        elif name == 'egn_program_set_deps':
            ops[-1].update(signal=int(args[0]), waits=[int(w) for w in args[1]])
        else:
            ints, refs = [], []
            for a in args:
                for v in (a if isinstance(a, list) else [a]):
                    if isinstance(v, _lib.Ref):
                        refs.append((int(v.slot), int(v.off)))
                    else:
                        ints.append(int(v))
            barrier = name in ('egn_program_fork', 'egn_program_join')
            if barrier:
                lane = 0
            ops.append(dict(kind=KIND_OF_CALL[name], lane=lane, signal=0, waits=[], ints=ints, refs=refs, flops=0.0,
                            bytes=0.0, tag=b''))
    return ops


def encode_op(op):
    """The canonical little-endian record of an op (egn_plan_op_record returns the same bytes from a parsed file)."""
    out = [struct.pack('<IIII', op['kind'], op['lane'], op['signal'], len(op['waits']))]
    out.append(struct.pack('<%dI' % len(op['waits']), *op['waits']))
    out.append(struct.pack('<I%di' % len(op['ints']), len(op['ints']), *op['ints']))
    out.append(struct.pack('<I', len(op['refs'])))
    out += [struct.pack('<iq', slot, off) for slot, off in op['refs']]
    out.append(struct.pack('<ddI', op['flops'], op['bytes'], len(op['tag'])))
    out.append(op['tag'])
    return b''.join(out)


def _text(s):
    b = s.encode() if isinstance(s, str) else bytes(s)
    return struct.pack('<I', len(b)) + b


# ---------------------------------------------------------------------------
# writing
# ---------------------------------------------------------------------------
class PlanWriter(object):
    """Collects programs and their weights, then writes the file.  ``add_program`` stores every tensor of a program's
    weights blob as a piece keyed by its content: programs of several batch sizes (and a program added twice) share
    what they can."""

    def __init__(self, header):
        self.header = header
        self.pieces = []             # 1-D fp32 CPU tensors
        self._by_content = {}
        self._by_id = {}             # id(tensor) -> piece (tensors a packing memo hands out again are hashed once)
        self.programs = []

    def _piece(self, t):
        known = self._by_id.get(id(t))
        if known is not None and known[0] is t:
            return known[1]
        src, t = t, t.detach().to(torch.float32).contiguous().cpu()
        raw = t.numpy()
        key = (raw.nbytes, hashlib.blake2b(memoryview(raw).cast('B'), digest_size=16).digest())
        idx = self._by_content.get(key)
        if idx is None:
            idx = len(self.pieces)
            self.pieces.append(t)
            self._by_content[key] = idx
        self._by_id[id(src)] = (src, idx)          # (holds the tensor: its id is not reused while the writer lives)
        return idx

    def add_program(self, ptype, n, arena_bytes, blobs, weight_bytes, roles, ops):
        """``blobs``: the recorder's weight tensors in blob order (each at the next 256-byte boundary); ``roles``:
        (role, bytes) of the user slots; ``ops``: ``calls_to_ops`` of the program's log."""
        places, off = [], 0
        for t in blobs:
            places.append((self._piece(t), off))
            off += (t.numel() * 4 + 255) // 256 * 256
        assert off == weight_bytes, (off, weight_bytes)
        self.programs.append(dict(type=ptype, n=n, arena_bytes=arena_bytes, weight_bytes=weight_bytes, places=places,
                                  roles=list(roles), ops=list(ops)))

    # -- bytes --
    def head_payload(self):
        h = self.header
        out = [struct.pack('<II', h['lib_version'], h['fingerprint']), _text(h['arch']),
               struct.pack('<III', PRECISIONS.index(h['precision']), HEAD_TYPES.index(h['head_type']),
                           DECODES.index(h['decode'])),
               struct.pack('<IIIIII', h['J'], h['C'], h['H'], h['W'], h['map_h'], h['map_w']),
               struct.pack('<dd', h['mul_x'], h['mul_y']),
               struct.pack('<III', h['lifter_in'], h['lifter_out'], h['ld_in'])]
        for k in LS_KEYS:
            v = np.ascontiguousarray(h['LS'][k], dtype='<f8').reshape(-1)
            out += [struct.pack('<I', v.size), v.tobytes()]
        out.append(struct.pack('<I%dI' % len(h['sizes']), len(h['sizes']), *h['sizes']))
        out.append(_text(h['switches']))
        return b''.join(out)

    @staticmethod
    def program_payload(g):
        out = [struct.pack('<IIQQ', g['type'], g['n'], g['arena_bytes'], g['weight_bytes']),
               struct.pack('<I', len(g['places']))]
        out += [struct.pack('<IQ', piece, off) for piece, off in g['places']]
        out.append(struct.pack('<I', len(g['roles'])))
        out += [struct.pack('<IQ', role, nbytes) for role, nbytes in g['roles']]
        out.append(struct.pack('<I', len(g['ops'])))
        out += [encode_op(op) for op in g['ops']]
        return b''.join(out)

    @staticmethod
    def _section(f, tag, chunks):
        length = sum(len(c) for c in chunks)
        f.write(struct.pack('<IQ', tag, length))
        crc = 0
        for c in chunks:
            crc = zlib.crc32(c, crc)
            f.write(c)
        f.write(struct.pack('<I', crc & 0xffffffff))

    def write(self, path):
        tmp = path + '.tmp'
        with open(tmp, 'wb') as f:
            f.write(MAGIC + struct.pack('<I', FORMAT_VERSION))
            self._section(f, SEC_HEAD, [self.head_payload()])
            for g in self.programs:
                self._section(f, SEC_PROG, [self.program_payload(g)])
            chunks = [struct.pack('<I', len(self.pieces))]
            for t in self.pieces:
                chunks += [struct.pack('<Q', t.numel() * 4), memoryview(t.numpy()).cast('B')]
            self._section(f, SEC_PIEC, chunks)
            self._section(f, SEC_END, [])
        os.replace(tmp, path)
        return path


def switches_text(hrnet_engine):
    """The EGONET_AMD_* switches that shaped the recording: the environment's and what the engine read from it."""
    env = ['%s=%s' % (k, v) for k, v in sorted(os.environ.items()) if k.startswith('EGONET_AMD_')]
    eng = ['lanes=%d' % hrnet_engine.lanes, 'pw_fuse=%d' % hrnet_engine.fuse_layer1, 'chain=%d' % hrnet_engine.chain_regions,
           'deps=%d' % hrnet_engine.deps, 'deps_min_n=%d' % hrnet_engine.deps_min_n]
    return ';'.join(env + eng)


def record_programs(ego, n, decode_mode, device, pack, logs=None):
    """The HRNet and the lifter recording of ``ego`` for ``n`` crops as (type, recorder, roles, ops, arena bytes, weight
    bytes) -- recorded, planned, tile-chosen and packed by the engine's own code, emitted into a log instead of a
    native program.  ``logs``: a list that receives the two raw call logs."""
    from . import engine
    HC, J = ego.HC, ego.HC.num_joints
    width, height = ego.resolution
    cin = HC.conv1.weight.shape[1]
    ld_in = (2 * J + 3) // 4 * 4
    out = []
    rec, nslots, shapes = HC._hip_engine()._record(n, cin, height, width, decode_mode)
    roles = [(ROLE_CROPS, n * cin * height * width * 4), (ROLE_MAPS, int(np.prod(shapes['maps'])) * 4)]
    if 'coords' in shapes:
        roles.append((ROLE_COORDS, n * J * 2 * 4))
    if decode_mode is not None:
        roles += [(ROLE_XY, n * J * 2 * 4), (ROLE_MAX, n * J * 4), (ROLE_IDX, n * J * 4)]
    assert len(roles) == nslots, (roles, nslots)
    lrec = ego.L._hip_engine()._record(n, ld_in)
    lroles = [(ROLE_LIFT_IN, n * ld_in * 4), (ROLE_LIFT_OUT, n * ego.L.w2.out_features * 4)]
    for ptype, r, rl in ((0, rec, roles), (1, lrec, lroles)):
        log = []
        prog = engine.Program(r, device, len(rl), log=log, native=False, pack=pack)
        if logs is not None:
            logs.append(log)
        out.append((ptype, r, rl, calls_to_ops(log), prog.arena_bytes, prog.weight_bytes))
    return out, shapes


def export_plan(ego, path, batch_sizes=(1, 2, 4, 8, 16, 32, 64), decode='auto', device=None):
    """Write the plan of ``ego.infer_crops(..., decode=decode, refine=None)`` for the given batch sizes to ``path``.
    ``device``: the GPU whose measurements choose the tile configurations (shapes the shipped table does not hold are
    autotuned there, as the engine does); None: the device of the model's parameters if that is a GPU, else no device at
    all -- the export then takes the table's choices or the cost model's 0 and never measures, and needs no GPU."""
    from .filters import pack_for_kind
    HC = ego.HC
    if HC.head_type not in HEAD_TYPES:
        raise ValueError('export_plan: no plan for the %r head (infer_crops has none either)' % (HC.head_type,))
    if ego.LS is None:
        raise ValueError('lifter statistics LS are not loaded')
    if HC._hip_engine().activations != 'f32':
        raise ValueError("export_plan: plans hold fp32-storage programs only, got activations = %r (set it to 'f32')"
                         % (HC._hip_engine().activations,))
    if decode == 'auto':
        decode = 'coords' if HC.head_type == 'coordinates' else 'soft'
    if decode not in DECODES or (decode == 'coords' and HC.head_type != 'coordinates'):
        raise ValueError('decode must be one of %r for the %s head, got %r' % (DECODES, HC.head_type, decode))
    sizes = [int(s) for s in batch_sizes]
    if not sizes or min(sizes) < 1 or max(sizes) > 65535:
        raise ValueError('batch_sizes must be 1 .. 65535, got %r' % (batch_sizes,))
    if device is None:
        p = next(HC.parameters())
        device = p.device if p.is_cuda else None
    elif not torch.cuda.is_available():
        device = None
    decode_mode = None if decode == 'coords' else DECODES.index(decode)
    memo = {}

    def pack(w, kind):          # a filter is packed once per layout, whatever the number of batch sizes
        key = (w.data_ptr(), tuple(w.shape), kind)
        if key not in memo:
            memo[key] = pack_for_kind(w, kind)
        return memo[key]

    J = HC.num_joints
    width, height = ego.resolution
    writer = PlanWriter(None)
    shapes = None
    for n in sizes:
        progs, shapes = record_programs(ego, n, decode_mode, device, pack)
        for ptype, r, roles, ops, arena_bytes, weight_bytes in progs:
            writer.add_program(ptype, n, arena_bytes, r.blobs, weight_bytes, roles, ops)
    mh, mw = shapes['maps'][2], shapes['maps'][3]
    mul = (float(width), float(height)) if decode == 'coords' else (float(width) / mw, float(height) / mh)
    L = _lib.lib()
    writer.header = dict(
        lib_version=L.egn_version(), fingerprint=L.egn_conv_table_fingerprint(), arch='gfx950',
        precision=HC._hip_engine().precision, head_type=HC.head_type, decode=decode, J=J, C=HC.conv1.weight.shape[1],
        H=height, W=width, map_h=mh, map_w=mw, mul_x=mul[0], mul_y=mul[1], lifter_in=ego.L.w1.in_features,
        lifter_out=ego.L.w2.out_features, ld_in=(2 * J + 3) // 4 * 4, LS=ego.LS, sizes=sizes,
        switches=switches_text(HC._hip_engine()))
    return writer.write(path)


# ---------------------------------------------------------------------------
# reading and running
# ---------------------------------------------------------------------------
def _dev_f64(a, device):
    if torch.is_tensor(a):
        return a.to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(device)


class PlanError(_lib.EgonetHipError):
    """egn_plan_open / _load / _infer refused; ``code`` is the library's error code (EGN_E_PLAN_*)."""

    def __init__(self, code, what):
        _lib.EgonetHipError.__init__(self, '%s: %s (code %d)' % (what, _lib.lib().egn_strerror(code).decode(), code))
        self.code = code


def open_code(path):
    """egn_plan_open's return code for ``path`` (0: a valid plan; it is closed again)."""
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.egn_plan_open(os.fsencode(path), C.byref(h))
    if rc == 0:
        L.egn_plan_close(h)
    return rc


class Plan(object):
    """An opened plan file.  ``info``: the header; ``load(device)``: upload and build the programs; ``infer_crops``:
    ``EgoNet.infer_crops`` (refine=None) from the file, same keys, dtypes and -- the same launches -- bytes."""

    def __init__(self, path):
        self.lib = _lib.lib()
        self.handle = C.c_void_p()
        rc = self.lib.egn_plan_open(os.fsencode(path), C.byref(self.handle))
        if rc:
            self.handle = None
            raise PlanError(rc, 'egn_plan_open(%s)' % path)
        self.path = path
        self.device = None
        raw = _lib.PlanInfo()
        _lib.check(self.lib.egn_plan_get_info(self.handle, C.byref(raw)))
        buf = C.create_string_buffer(1 << 16)
        _lib.check(self.lib.egn_plan_get_text(self.handle, 1, buf, len(buf)))
        self.info = dict(
            format_version=raw.format_version, lib_version=raw.lib_version, fingerprint=raw.fingerprint,
            arch=raw.arch.decode(), precision=PRECISIONS[raw.precision], head_type=HEAD_TYPES[raw.head_type],
            decode=DECODES[raw.decode], J=raw.J, C=raw.C, H=raw.H, W=raw.W, map_size=(raw.map_h, raw.map_w),
            mul=(raw.mul_x, raw.mul_y), lifter_in=raw.lifter_in, lifter_out=raw.lifter_out, ld_in=raw.ld_in,
            batch_sizes=tuple(raw.sizes[:raw.n_sizes]), n_pieces=raw.n_pieces, n_programs=raw.n_programs,
            switches=buf.value.decode(), LS={})
        for k, name in enumerate(LS_KEYS):
            v = np.empty(raw.lifter_in if k < 2 else raw.lifter_out, dtype=np.float64)
            _lib.check(self.lib.egn_plan_get_stats(self.handle, k, v.ctypes.data, v.size))
            self.info['LS'][name] = v

    def program_info(self, i):
        t, n, ab, wb, nops, nw = C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong(), C.c_int(), C.c_int()
        _lib.check(self.lib.egn_plan_program_info(self.handle, i, C.byref(t), C.byref(n), C.byref(ab), C.byref(wb),
                                                  C.byref(nops), C.byref(nw), None, 0))
        kinds = (C.c_int * max(nops.value, 1))()
        _lib.check(self.lib.egn_plan_program_info(self.handle, i, None, None, None, None, None, None, kinds, nops.value))
        return dict(type=t.value, n=n.value, arena_bytes=ab.value, weight_bytes=wb.value, n_ops=nops.value,
                    ops_with_waits=nw.value, kinds=list(kinds[:nops.value]))

    def op_record(self, i, k):
        used = C.c_int()
        _lib.check(self.lib.egn_plan_op_record(self.handle, i, k, None, 0, C.byref(used)))
        buf = C.create_string_buffer(max(used.value, 1))
        _lib.check(self.lib.egn_plan_op_record(self.handle, i, k, buf, used.value, C.byref(used)))
        return buf.raw[:used.value]

    def native_program(self, i):
        """The egn_program handle of program ``i`` of a loaded plan (owned by the plan)."""
        return C.c_void_p(self.lib.egn_plan_native_program(self.handle, i))

    def load(self, device=None):
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        with torch.cuda.device(device):
            rc = self.lib.egn_plan_load(self.handle, -1)
        if rc:
            raise PlanError(rc, 'egn_plan_load(%s)' % self.path)
        self.device = device
        return self

    @torch.no_grad()
    def infer_crops(self, instances, centers, scales, K=None, alpha_mode='proj', to_host=True):
        if self.device is None:
            raise ValueError('Plan.load(device) first')
        if not instances.is_cuda or instances.device != self.device:
            raise ValueError('infer_crops takes CUDA crops on the device the plan was loaded on (%s)' % (self.device,))
        i = self.info
        n = instances.shape[0]
        if tuple(instances.shape[1:]) != (i['C'], i['H'], i['W']):
            raise ValueError('the plan takes [n,%d,%d,%d] crops, got %s' % (i['C'], i['H'], i['W'], tuple(instances.shape)))
        dev, J, D = self.device, i['J'], i['lifter_out']
        x = instances.float().contiguous()
        c_d, s_d = _dev_f64(centers, dev), _dev_f64(scales, dev)
        if tuple(c_d.shape) != (n, 2) or tuple(s_d.shape) != (n, 2):
            raise ValueError('centers / scales must be [n,2]')
        local = torch.empty(n, J, 2, dtype=torch.float32, device=dev)
        screen = torch.empty(n, 2 * J, dtype=torch.float64, device=dev)
        pred3d = torch.empty(n, D, dtype=torch.float64, device=dev)
        res = {'local': local, 'kpts_2d': screen, 'kpts_3d': pred3d.view(n, -1, 3)}
        outs = _lib.PlanOutputs(_lib.ptr(local), _lib.ptr(screen), _lib.ptr(pred3d), None, None)
        if D == 96:
            euler = torch.empty(n, 3, dtype=torch.float64, device=dev)
            alpha = torch.empty(n, dtype=torch.float64, device=dev)
            outs.euler, outs.alpha = _lib.ptr(euler), _lib.ptr(alpha)
            res.update(euler=euler, alpha=alpha, translation=pred3d.view(n, -1, 3)[:, 0, :])
        fx, cx = (float(K[0, 0]), float(K[0, 2])) if K is not None else (1.0, 0.0)
        with torch.cuda.device(dev):
            rc = self.lib.egn_plan_infer(self.handle, _lib.ptr(x), n, _lib.ptr(c_d), _lib.ptr(s_d), int(K is not None), fx,
                                         cx, 0 if alpha_mode == 'proj' else 1, C.byref(outs), _lib.current_stream(dev))
        if rc == -1:
            raise ValueError('egn_plan_infer: %d crops cannot be composed of the exported batch sizes %r (or a bad '
                             'argument)' % (n, i['batch_sizes']))
        if rc:
            raise PlanError(rc, 'egn_plan_infer')
        if to_host:
            res = {k: v.cpu().numpy() for k, v in res.items()}
        return res

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.egn_plan_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
