#!/usr/bin/env python3
"""Latency of the online sessions (SlidingWindowDecoder.session): the headline plan -- [[144,12,12]], p = 0.003, 12 rounds, (W,F) =
(3,1), OSD-CS 10 -- fed one detector round per push_device.  HIP-event time of every push that completes a window (merge + window
decode + commit on one stream), median and maximum over 20 batches after warm-up, for B = 1, 64, 4096; next to it the one-launch
decode_device of the same batches.  Writes profiles/session_latency.json (or the path given as the first argument)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402
from slidingwindowdecoder_amd import DemSampler, SlidingWindowDecoder  # noqa: E402

BATCHES, WARMUP = 20, 3
plan = bench.build_problem()
kw = dict(bench.DECODER_KW, osd_order=10)
dec = SlidingWindowDecoder(plan, **kw)
sampler = DemSampler(plan.chk, plan.obs, plan.priors)
h = plan.n_half
rounds = plan.chk.shape[0] // h
stream = torch.cuda.Stream()
out = {"plan": "[[144,12,12]] p=0.003, 12 rounds, (3,1), osd_cs 10", "windows": dec.W, "rows_per_push": h, "batches": BATCHES, "sizes": {}}
for B in (1, 64, 4096):
    ses = dec.session(B)
    steps, sums, whole = [], [], []
    for k in range(WARMUP + BATCHES):
        det, _ = sampler.sample_device(B, seed=1000 + k)
        torch.cuda.synchronize()
        ev, done = [], []
        with torch.cuda.stream(stream):
            ses.begin(B)
            for r in range(rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                _, count = ses.push_device(det[:, r * h:(r + 1) * h], stream=stream)
                e1.record(stream)
                stream.synchronize()  # the next round arrives after this one has been handled
                ev.append((e0, e1))
                done.append(count)
            a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a0.record(stream)
            total, _, _ = dec.decode_device(det, stream=stream)
            a1.record(stream)
            stream.synchronize()
        assert sum(done) == dec.W and torch.equal(total, ses.total_device())
        if k >= WARMUP:
            ms = [e0.elapsed_time(e1) for (e0, e1), c in zip(ev, done) if c]
            steps += ms
            sums.append(sum(ms))
            whole.append(a0.elapsed_time(a1))
    ses.close()
    rec = {"step_ms_median": float(np.median(steps)), "step_ms_max": float(np.max(steps)), "steps_sum_ms_median": float(np.median(sums)),
           "one_launch_ms_median": float(np.median(whole)), "one_launch_ms_max": float(np.max(whole))}
    rec["sum_over_one_launch"] = rec["steps_sum_ms_median"] / rec["one_launch_ms_median"]
    out["sizes"][str(B)] = rec
    print(f"B = {B}: window step median {rec['step_ms_median']:.3f} ms, max {rec['step_ms_max']:.3f} ms; {dec.W} steps {rec['steps_sum_ms_median']:.3f} ms; "
          f"one launch {rec['one_launch_ms_median']:.3f} ms (x{rec['sum_over_one_launch']:.2f})", flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "session_latency.json")
json.dump(out, open(path, "w"), indent=1)
print("wrote", path)
