#!/usr/bin/env python3
"""Latency of the rolling sessions (SlidingWindowDecoder.rolling_session): the headline plan -- [[144,12,12]], p = 0.003, 12 rounds,
(W,F) = (3,1), OSD-CS 10 -- as the template of a 200-round experiment, fed one 72-row detector round per push_device.  HIP-event time
of every push that completes a body window (merge + window decode + commit and frame shift on one stream), median and maximum over
the steady-state steps (head and tail left out) of one run after a warm-up run, for B = 1, 64, 4096; next to it the per-step figures
of the fixed session (SlidingWindowDecoder.session) on the 12-round plan itself, measured the same way.
Writes profiles/rolling_latency.json (or the path given as the first argument)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402
from slidingwindowdecoder_amd import DemSampler, SlidingWindowDecoder  # noqa: E402
from slidingwindowdecoder_amd.circuit import bb_dem  # noqa: E402
from slidingwindowdecoder_amd.codes import bb_code  # noqa: E402

ROUNDS, FIXED_BATCHES, WARMUP = 200, 10, 2
plan = bench.build_problem()
kw = dict(bench.DECODER_KW, osd_order=10)
dec = SlidingWindowDecoder(plan, **kw)
h = plan.n_half
code, A, Bm = bb_code(144)
long_dem = bb_dem(code, A, Bm, 0.003, ROUNDS)
assert long_dem.chk.shape[0] == (ROUNDS + 1) * h
long_sampler = DemSampler(long_dem.chk, long_dem.obs, long_dem.priors)
short_sampler = DemSampler(plan.chk, plan.obs, plan.priors)
stream = torch.cuda.Stream()
out = {"template": "[[144,12,12]] p=0.003, 12 rounds, (3,1), osd_cs 10", "rounds": ROUNDS, "rows_per_push": h, "sizes": {}}


def timed(push):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    n = push()
    e1.record(stream)
    stream.synchronize()  # the next round arrives after this one has been handled
    return (e0, e1), n


for B in (1, 64, 4096):
    ses = dec.rolling_session(B)
    steps = []
    for k in range(2):  # a warm-up run, then the run that counts
        det, _ = long_sampler.sample_device(B, seed=2000 + k)
        torch.cuda.synchronize()
        ev = []
        with torch.cuda.stream(stream):
            ses.begin(B)
            for r in range(ROUNDS):
                ev.append(timed(lambda: len(ses.push_device(det[:, r * h:(r + 1) * h], stream=stream))))
            t = ses.finish_device(det[:, ROUNDS * h:], stream=stream)[0]
            stream.synchronize()
        assert t == ROUNDS - 2 and sum(n for _, n in ev) == t
        steps = [e0.elapsed_time(e1) for (e0, e1), n in ev if n][1:]  # without the head
    rolling_bytes = ses.device_bytes
    ses.close()
    fixed, fses = [], dec.session(B)
    for k in range(WARMUP + FIXED_BATCHES):
        det, _ = short_sampler.sample_device(B, seed=1000 + k)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            fses.begin(B)
            ev = [timed(lambda: fses.push_device(det[:, r * h:(r + 1) * h], stream=stream)[1]) for r in range(plan.chk.shape[0] // h)]
        if k >= WARMUP:
            fixed += [e0.elapsed_time(e1) for (e0, e1), n in ev if n][1:-1]  # its body windows
    fses.close()
    rec = {"rolling_steps": len(steps), "rolling_step_ms_median": float(np.median(steps)), "rolling_step_ms_max": float(np.max(steps)),
           "fixed_steps": len(fixed), "fixed_step_ms_median": float(np.median(fixed)), "fixed_step_ms_max": float(np.max(fixed)),
           "rolling_device_bytes": int(rolling_bytes)}
    out["sizes"][str(B)] = rec
    print(f"B = {B}: rolling step median {rec['rolling_step_ms_median']:.3f} ms, max {rec['rolling_step_ms_max']:.3f} ms over {len(steps)} steps; "
          f"fixed session step median {rec['fixed_step_ms_median']:.3f} ms, max {rec['fixed_step_ms_max']:.3f} ms over {len(fixed)} steps; "
          f"{rolling_bytes} B of session memory", flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rolling_latency.json")
json.dump(out, open(path, "w"), indent=1)
print("wrote", path)
