"""What the native training steps and autograd bridges of both models share (``train_hrnet``, ``train_lifter``,
``autograd``, ``graph``): the flat parameter / optimizer buffers, the one-launch step counters, the packed-filter
cache, and the few pieces of host plumbing every owner needs exactly once -- the weight-gradient side stream, the
gradient all-reduce / optimizer tail of a native step, a bridge's fresh gradient views, ``bench.py``'s timing
bracket.  Nothing here knows a model."""
import contextlib
import gc
import os

import torch

from . import _lib, filters
from .engine import _round_up


class StepCounters(object):
    """The BatchNorm layers' ``num_batches_tracked`` += 1 and the loss accumulator = 0 as ONE launch at the start of a
    native step (``egn_step_counters_i64``) instead of a ``torch._foreach_add_`` and a ``tensor.zero_()`` [round 6]: the
    device array of the counters' addresses is built once and rebuilt if a buffer moved (``.to()``, ``load_state_dict``
    onto new storage)."""

    def __init__(self):
        self.ptrs = None
        self.table = None

    def tick(self, bns, loss_dev, stream):
        L = _lib.lib()
        ptrs = [bn.num_batches_tracked.data_ptr() for bn in bns if bn.num_batches_tracked is not None]
        if ptrs != self.ptrs:
            dev = loss_dev.device if loss_dev is not None else bns[0].num_batches_tracked.device
            self.table = torch.tensor(ptrs, dtype=torch.int64, device=dev) if ptrs else None
            self.ptrs = ptrs
        _lib.check(L.egn_step_counters_i64(_lib.ptr(self.table), len(ptrs), _lib.ptr(loss_dev), stream), 'step counters')


class FlatParams(object):
    """Trainable parameters as views of one flat fp32 buffer (+ flat grad, m, v)."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError('no trainable parameters')
        dev = self.params[0].device
        self.offsets = []
        total = 0
        for p in self.params:
            self.offsets.append(total)
            total += _round_up(p.numel(), 4)          # every view stays 16-byte aligned
        self.numel = total
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.m = torch.zeros(total, dtype=torch.float32, device=dev)
        self.v = torch.zeros(total, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, off in zip(self.params, self.offsets):
                view = self.flat[off:off + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                p.grad = self.grad[off:off + p.numel()].view_as(p)
        # step counter and learning rate live in device memory (hipGraph-safe)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.lr_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self._lr_host = None

    @property
    def t(self):
        return int(self.step_dev.item())

    # -- save / resume (train_state.py): this object's part -----------------------------------------------------
    def layout(self, names):
        """Per parameter, in order: its name (``names``: id(parameter) -> name), its shape and its offset in floats."""
        return [{'name': names[id(p)], 'shape': [int(s) for s in p.shape], 'offset': int(off)}
                for p, off in zip(self.params, self.offsets)]

    def cut(self, buf, i):
        """Parameter ``i``'s own elements of a flat buffer with this layout (a view, in the parameter's shape)."""
        p, off = self.params[i], self.offsets[i]
        return buf[off:off + p.numel()].view(p.shape)

    def state(self):
        """CPU copies of the moments, padding included, and the step count (one read-back)."""
        return {'step': self.t, 'm': self.m.detach().to('cpu', copy=True), 'v': self.v.detach().to('cpu', copy=True)}

    def load_state(self, m, v, step):
        """In place: the buffers and the counter keep their addresses.  ``v`` None (SGD): zeroed."""
        with torch.no_grad():
            self.m.copy_(m)
            if v is None:
                self.v.zero_()
            else:
                self.v.copy_(v)
            self.step_dev.fill_(int(step))

    def set_lr(self, lr):
        """The learning rate the next optimizer launch reads from device memory: refilled only when the scheduler
        changed it on the host (never inside a graph; ``GraphedStep`` calls this before each replay)."""
        if lr != self._lr_host:
            self.lr_dev.fill_(lr)
            self._lr_host = lr

    def adam_step(self, lr, betas, eps, stream, weight_decay=0.0):
        """torch.optim.Adam (optimizer.py:19-21); weight_decay is the coupled L2 form torch implements."""
        self.set_lr(lr)
        L = _lib.lib()
        if weight_decay:
            _lib.check(L.egn_adam_l2_step_dev_f32(_lib.ptr(self.flat), _lib.ptr(self.grad), _lib.ptr(self.m),
                                                  _lib.ptr(self.v), self.numel, _lib.ptr(self.lr_dev), betas[0],
                                                  betas[1], eps, weight_decay, _lib.ptr(self.step_dev), stream), 'adam')
        else:
            _lib.check(L.egn_adam_step_dev_f32(_lib.ptr(self.flat), _lib.ptr(self.grad), _lib.ptr(self.m),
                                               _lib.ptr(self.v), self.numel, _lib.ptr(self.lr_dev), betas[0],
                                               betas[1], eps, _lib.ptr(self.step_dev), stream), 'adam')

    def sgd_step(self, lr, momentum, weight_decay, stream):
        """torch.optim.SGD(momentum, weight_decay), dampening 0, no Nesterov (optimizer.py:23-26); the
        momentum buffer lives in ``m``."""
        self.set_lr(lr)
        _lib.check(_lib.lib().egn_sgd_step_dev_f32(_lib.ptr(self.flat), _lib.ptr(self.grad), _lib.ptr(self.m),
                                                   self.numel, _lib.ptr(self.lr_dev), momentum, weight_decay,
                                                   _lib.ptr(self.step_dev), stream), 'sgd')

    def update(self, o, stream):
        """One optimizer step as configured on the step object ``o`` (lr, optim_type, betas, eps, momentum,
        weight_decay)."""
        if o.optim_type == 'sgd':
            self.sgd_step(o.lr, o.momentum, o.weight_decay, stream)
        else:
            self.adam_step(o.lr, o.betas, o.eps, stream, o.weight_decay)


@contextlib.contextmanager
def _gc_paused():
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class PackedFilters(object):
    """The packed forward / data-gradient filters of every conv weight of a model.

    The weights change once per iteration (in the optimizer step), so from the second
    step on ALL filters are packed by one launch at the start of the step
    (``egn_pack_conv_weights_batch_f32``) instead of ~600 small ones; the first step
    packs them one by one while it discovers which (weight, direction) pairs exist."""

    _DESC = [('w', '<u8'), ('dst', '<u8'), ('Cout', '<i4'), ('Cin', '<i4'), ('taps', '<i4'), ('code', '<i4'),
             ('begin', '<i8')]

    def __init__(self, device):
        self.dev = device
        self.L = _lib.lib()
        self.entries = {}          # (id(weight), kind, dgrad) -> (weight, packed tensor)
        self.table = None          # device descriptor table once the set is known
        self.total = 0
        self.ptrs = None

    def get(self, weight, dgrad, stream, kind=filters.DIRECT):
        """The filter of ``weight`` in the layout ``kind`` (filters.DIRECT / WINO2 / WINO4, what tuner.kind_of says
        the chosen kernel reads); ``dgrad``: the data-gradient filter."""
        key = (id(weight), kind, int(dgrad))
        ent = self.entries.get(key)
        if ent is not None and self.table is not None:
            return ent[1]
        if ent is None:
            nfl = filters.device_floats(kind, weight.shape, dgrad)
            ent = self.entries[key] = (weight, torch.empty(nfl, dtype=torch.float32, device=self.dev))
            self.table = None
        filters.pack_on_device(weight, kind, dgrad, ent[1], stream)
        return ent[1]

    def _pointers(self):
        return [w.data_ptr() for (w, _) in self.entries.values()]

    def finalize(self):
        """Build the device descriptor table for the (weight, direction) pairs seen so far."""
        import numpy as np
        if self.table is not None or not self.entries:
            return
        desc = np.zeros(len(self.entries), dtype=np.dtype(self._DESC, align=True))
        assert desc.dtype.itemsize == self.L.egn_pack_desc_bytes(), (desc.dtype.itemsize, self.L.egn_pack_desc_bytes())
        begin = 0
        for i, ((_, kind, dgrad), (w, wp)) in enumerate(self.entries.items()):
            cout, cin, kh, kw = w.shape
            code, unit_floats = filters.DEVICE_PACK[kind]
            desc[i] = (w.data_ptr(), wp.data_ptr(), cout, cin, kh * kw, code | dgrad, begin)
            begin += wp.numel() // unit_floats
        self.total = begin
        self.table = torch.from_numpy(desc.view(np.uint8)).to(self.dev)
        self.ptrs = self._pointers()

    def pack_all(self, stream):
        """One launch for every filter; False if the table is not built yet (first step) or a
        parameter was re-allocated since (``.to()`` / ``load_state_dict`` on a new storage)."""
        if self.table is None:
            return False
        if self._pointers() != self.ptrs:
            self.table = None
            return False
        _lib.check(self.L.egn_pack_conv_weights_batch_f32(_lib.ptr(self.table), len(self.entries), self.total,
                                                          stream), 'pack all')
        return True


def grad_views(params, dev):
    """One fresh, zeroed flat gradient buffer per backward of an autograd bridge -> (views, {id(param): view}).  The
    views go back to autograd, which accumulates them into (or, when .grad is None, adopts them as) the parameters'
    .grad."""
    sizes = [(p.numel() + 3) // 4 * 4 for p in params]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
    views, off = [], 0
    for p, sz in zip(params, sizes):
        views.append(flat[off:off + p.numel()].view_as(p))
        off += sz
    return views, {id(p): v for p, v in zip(params, views)}


# -- weight gradients on a side stream --------------------------------------------------------------------------
# Nothing on the backward chain waits for a weight gradient (only the all-reduce and the optimizer do): issued on a
# second stream once their operands exist, the chain's latency-bound BatchNorm / reduction kernels overlap their
# MFMA work.  One side stream per owner: its launches share one workspace.
def wgrad_side_stream(dev, priority=0):
    """The owner's ``wgrad_stream`` (EGONET_AMD_WGRAD_STREAM=0: None, everything on one stream)."""
    if os.environ.get('EGONET_AMD_WGRAD_STREAM', '1') == '0':
        return None
    return torch.cuda.Stream(device=dev, priority=priority)


def _after(waiter, signaller):
    """What ``waiter`` is given from here on runs after everything ``signaller`` has been given so far."""
    ev = torch.cuda.Event()
    ev.record(signaller)
    waiter.wait_event(ev)


def fork_wgrad(side, dev, keep, operands):
    """Before one weight-gradient launch on ``side`` that reads ``operands``: ordered after the current stream's work
    so far.  ``keep`` holds the operands alive until ``join_wgrad``."""
    _after(side, torch.cuda.current_stream(dev))
    keep.append(operands)


def join_wgrad(side, dev, keep):
    """The side stream's weight gradients are complete for everything issued after this on the current stream
    (gradient all-reduce, optimizer); the tensors they read may be released."""
    if side is not None and keep:
        _after(torch.cuda.current_stream(dev), side)
    del keep[:]


# -- the tail of a native step ``o`` (o.grad_sync, o.flat, o.wgrad_stream, the optimizer settings) ----------------
def begin_grad_sync(o, closures=()):
    """-> the overlapped all-reduce session of this backward, or None (no ``grad_sync``, one without sessions, or the
    overlap switched off: ``finish_step`` then reduces the whole flat gradient once).  The session starts the
    all-reduce of a slice of the flat buffer (on a communication stream) as soon as ``sess.done(params)`` has
    reported every parameter in it.  ``closures``: backward closures with a ``.params`` attribute -- a parameter
    written by several of them (shared weights) is final after its LAST report."""
    if not hasattr(o.grad_sync, 'begin'):
        return None
    counts = {}
    for fn in closures:
        for q in getattr(fn, 'params', ()):
            counts[id(q)] = counts.get(id(q), 0) + 1
    return o.grad_sync.begin(o.flat, torch.cuda.current_stream(o.dev), o.wgrad_stream, report_counts=counts)


def finish_step(o, sess, update, stream):
    """After the backward (side stream joined): the gradient exchange, then the optimizer.  A grouped update
    (``o.grouped``, optim.py) takes its gradient norm here too, after the all-reduce of the whole buffer has completed
    on this stream: every rank computes the same clip coefficient."""
    if sess is not None:
        sess.finish()
    elif o.grad_sync is not None:
        o.grad_sync(o.flat.grad)
    if update:
        if getattr(o, 'grouped', None) is not None:
            o.grouped.update(stream)
        else:
            o.flat.update(o, stream)


# -- bench.py: ``owner.timing = []`` collects (cfg, flops, start, end[, ...]) per forward / data-gradient launch ----
def timing_begin(tm, dev):
    """-> the start hipEvent, recorded on the current stream (None when nothing is collected)."""
    if tm is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record(torch.cuda.current_stream(dev))
    return e0


def timing_end(tm, dev, e0, cfg, flops, *more):
    if tm is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(torch.cuda.current_stream(dev))
        tm.append((cfg, flops, e0, e1) + more)
