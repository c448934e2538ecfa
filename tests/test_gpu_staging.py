"""PinnedStaging (egonet_amd/common/staging.py) on the device: three uploads from one object with nothing synchronised
in between, so the third refills the first's pinned buffer behind its event while the second's copy may be in flight,
and has to grow it.  Every view must hold its own round's bytes."""
import numpy as np
import pytest
import torch

from egonet_amd.common import staging

pytestmark = pytest.mark.gpu


def _round(r):
    rng = np.random.RandomState(10 + r)
    arrays = {'u8': rng.randint(0, 256, 5).astype(np.uint8),             # odd length: padding follows
              'i64': rng.randint(-2 ** 62, 2 ** 62, (2, 4)).astype(np.int64),
              'f64': rng.standard_normal(3),
              'empty': np.zeros(0, dtype=np.float32)}
    if r == 2:
        arrays['big'] = rng.randint(0, 256, 100000).astype(np.uint8)     # past min_bytes: the buffer is replaced
    return arrays


def test_three_uploads_in_flight_keep_their_bytes():
    dev = torch.device('cuda', torch.cuda.current_device())
    st = staging.PinnedStaging(min_bytes=1 << 16)
    rounds = [_round(r) for r in range(3)]
    sent = [st.upload(arrays, dev) for arrays in rounds]                # no synchronise between the three
    assert sent[2][1].numel() > 1 << 16 >= sent[0][1].numel()
    torch.cuda.synchronize()
    for arrays, (views, block) in zip(rounds, sent):
        assert list(views) == list(arrays) and block.dtype == torch.uint8 and block.device == dev
        for name, a in arrays.items():
            got = views[name].cpu().numpy()
            assert got.dtype == a.dtype and got.shape == a.shape and got.tobytes() == a.tobytes(), name
