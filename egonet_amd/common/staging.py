"""Host arrays -> device tensors through one pinned buffer and ONE ``non_blocking`` copy on the current stream: the
upload of ``TrainSampleBuilder`` (common/train_samples.py) and of the device metrics (metric/criterions.py).

The kernels that read the views run on the same stream, so their ordering needs nothing more.  The pinned buffers
are double-buffered and each is guarded by an event recorded after its copy: an upload refills buffer ``k`` only
after waiting on ``k``'s event (the copy two uploads back), so a copy still in flight is never overwritten.
"""
import numpy as np
import torch

ALIGN = 256                    # byte alignment of every section: a view of any dtype starts on a multiple of its item size


def layout(sections, align):
    """``[(name, nbytes), ...]`` -> ``({name: offset}, total)``: the sections in list order, each offset (and the
    total) rounded up to ``align``."""
    where, total = {}, 0
    for name, nbytes in sections:
        where[name] = total
        total += (nbytes + align - 1) // align * align
    return where, total


class PinnedStaging(object):
    """Two pinned buffers of at least ``min_bytes``, their events and whose turn it is."""

    def __init__(self, min_bytes):
        self.min_bytes = min_bytes
        self._pinned, self._events, self._turn = [None, None], [None, None], 0

    def upload(self, arrays, dev, views=None, before_copy=None, after_copy=None):
        """``arrays`` {name: host numpy array, any dtype and shape, empty allowed} -> ``({name: device view of the
        array's dtype and shape}, the uint8 device block that holds them at ``layout``'s offsets)``.
        ``views``: the names to hand out views of, all by default (``TrainSampleBuilder``'s frames are read through
        the block).  ``before_copy`` / ``after_copy`` are called with the stream right before the copy is issued and
        right after the buffer's event is recorded (its timing events)."""
        where, total = layout([(name, a.nbytes) for name, a in arrays.items()], ALIGN)
        k = self._turn
        self._turn ^= 1
        if self._events[k] is None:
            self._events[k] = torch.cuda.Event()
        else:
            self._events[k].synchronize()           # the copy that last read buffer k has finished
        pinned = self._pinned[k]
        if pinned is None or pinned.numel() < total:
            pinned = self._pinned[k] = torch.empty(max(total, self.min_bytes), dtype=torch.uint8, pin_memory=True)
        host = pinned.numpy()
        for name, a in arrays.items():
            host[where[name]:where[name] + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        stream = torch.cuda.current_stream(dev)
        if before_copy is not None:
            before_copy(stream)
        block = torch.empty(total, dtype=torch.uint8, device=dev)
        block.copy_(pinned[:total], non_blocking=True)
        self._events[k].record(stream)
        if after_copy is not None:
            after_copy(stream)

        def view(name):
            a, off = arrays[name], where[name]
            return block[off:off + a.nbytes].view(_TORCH_DTYPE[a.dtype]).view(a.shape)
        return {name: view(name) for name in (arrays if views is None else views)}, block


_TORCH_DTYPE = {np.dtype(name): getattr(torch, name) for name in (
    'bool', 'uint8', 'int8', 'int16', 'int32', 'int64', 'float16', 'float32', 'float64')}
