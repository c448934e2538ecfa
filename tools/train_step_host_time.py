#!/usr/bin/env python
"""Host and wall time of one warm ``HRNetTrainStep.step`` (W48, coordinates head, 32 crops), and what the tuner costs it.

    python tools/train_step_host_time.py        # from the root of the checkout to measure

Prints one JSON line: wall time per step (host clock around step + synchronise, median / min of 30 after 5 warm
steps), time until ``step`` returns (the host side), ``tuner.choose`` calls per step and microseconds per call for the
tape's question on a tabled 3x3 layer.  The package is taken from the working directory, so one copy of this script
times two checkouts alternately on one machine; it speaks both the ``kinds`` and the older two-boolean ``choose``.
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402
from egonet_amd import configs, synth, tuner  # noqa: E402
from egonet_amd.model.heatmapModel import hrnet  # noqa: E402
from egonet_amd.train_hrnet import HRNetTrainStep  # noqa: E402

B = 32
cfg = configs.w48_config('coordinates')
net = hrnet.get_pose_net(cfg, is_train=False)
net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=1))
g = torch.Generator().manual_seed(100)
x = synth.synth_crops(B, 3, 256, 256, seed=50).cuda()
tgt = torch.rand(B, 33, 64, 64, generator=g).cuda()
jt = torch.rand(B, 33, 2, generator=g) * 256
net = net.cuda().train()
tr = HRNetTrainStep(net, lr=1e-3)
calls = [0]
orig = tuner.choose


def counted(*a, **k):
    calls[0] += 1
    return orig(*a, **k)


tuner.choose = counted
tr.step(x, tgt, jt)
torch.cuda.synchronize()
n_calls = calls[0]
tuner.choose = orig
for _ in range(4):
    tr.step(x, tgt, jt)
torch.cuda.synchronize()
wall, ret = [], []
for _ in range(30):
    t0 = time.perf_counter()
    tr.step(x, tgt, jt)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    wall.append((t2 - t0) * 1e3)
    ret.append((t1 - t0) * 1e3)

# the tuner alone: the tape's question for a tabled 3x3 layer, per call
key = (32, 64, 64, 48, 48, 48, 48, 3, 3, 1, 1, False, False)
if hasattr(tuner, 'usable'):
    def ask():
        return tuner.choose('cuda', key, tuner.TAPE_F43, ticket_cap=1 << 16, inplace_res=False)
else:
    def ask():
        return tuner.choose('cuda', key, allow_wino=True, allow_f43=True)
ask()
t0 = time.perf_counter()
for _ in range(5000):
    c = ask()
us = (time.perf_counter() - t0) / 5000 * 1e6
print(json.dumps(dict(crops=B, steps=len(wall), choose_calls_per_step=n_calls, wall_ms_median=statistics.median(wall),
                      wall_ms_min=min(wall), wall_ms_all=[round(v, 3) for v in wall],
                      step_returns_ms_median=statistics.median(ret), step_returns_ms_min=min(ret),
                      choose_us_per_call=us, choose_answer=c)))
