"""Sentinel guard bands around the buffers a swept kernel writes (helper module of tests/test_gpu_conv_sweep.py and
tests/test_gpu_train_ops_sweep.py; imported, not a conftest): a write outside its output lands in a band and is seen."""
import torch

GUARD = 1 << 14                  # elements of sentinel on each side of every written buffer
SENT32 = 0x5A5A5A5A
SENT64 = 0x5A5A5A5A5A5A5A5A


def _guarded(numel, dtype, fill):
    """(whole buffer, body view): the body sits between two sentinel bands."""
    it = torch.int32 if dtype == torch.float32 else torch.int64
    whole = torch.full((numel + 2 * GUARD,), SENT32 if it == torch.int32 else SENT64, dtype=it, device='cuda')
    body = whole[GUARD:GUARD + numel].view(dtype)
    if fill is not None:
        body.fill_(fill)
    return whole, body


def _guards_intact(whole):
    s = SENT32 if whole.dtype == torch.int32 else SENT64
    return bool((whole[:GUARD] == s).all()) and bool((whole[-GUARD:] == s).all())
