#!/usr/bin/env python
"""What the device window loop gives on a plan beyond the one-launch pipeline kernels.

Workload: the [[756,16,<=34]] BB code, 5 rounds, p = 0.003, (W, F) = (3, 1): 4 windows of 1134 x 8694 and 1134 x 9072 (3 distinct),
refused by the pipeline on checks, so every window decodes in the general form of osd_window (pre 8 / post 100 iterations, osd_0).
  (a) MemoryExperiment(window_loop="device").run: sample + window loop + account on the device, shots/s
  (b) on the detectors the experiment's sampler draws for shot numbers 0 ..: decode() through the device window loop and through
      the host window loop (one batched device decode per window through host memory, host commit, dense residual update),
      decodes/s, and that the two return the same faults
Wall-clock time around whole calls that end synchronised (the host loop works on the host between its launches, so device events
would not see it); one warm-up call, then the median of --repeats calls, all kept.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=512)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--p", type=float, default=0.003)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_loop_rate.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from slidingwindowdecoder_amd import MemoryExperiment, SlidingWindowDecoder
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    kw = dict(pre_max_iter=8, post_max_iter=100, ms_scaling_factor=1.0, osd_method="osd_0")
    t0 = time.perf_counter()
    exp = MemoryExperiment.bb(756, args.p, 5, 3, 1, window_loop="device", **kw)
    t_create = time.perf_counter() - t0
    dec, plan = exp.decoder, exp.plan
    res = {"workload": f"[[756,16,<=34]] 5 rounds p={args.p} (W,F)=(3,1) osd_window {kw}", "device": torch.cuda.get_device_name(0),
           "windows": [[int(x) for x in w.mat.shape] for w in plan.windows], "distinct_windows": dec.distinct_windows,
           "shots": args.shots, "batch": args.batch, "repeats": args.repeats, "create_s_device_loop": t_create}

    def measure(fn, count):
        fn()
        torch.cuda.synchronize()
        ts, out = [], None
        for _ in range(args.repeats):
            t = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
            print(f"  {count / ts[-1]:.1f} per s", file=sys.stderr, flush=True)
        ts.sort()
        return {"s": ts[len(ts) // 2], "s_all": ts, "per_s": count / ts[len(ts) // 2]}, out

    for lanes in (1, 2):
        m, r = measure(lambda: exp.run(args.shots, batch=args.batch, lanes=lanes), args.shots)
        res[f"a_experiment_run_{lanes}_lane_shots_per_s"] = dict(m, logical_errors=r.logical_errors, flagged=r.flagged,
                                                                  window_exit_classes=r.window_exit_classes.tolist())
    det = exp.sampler.sample(args.batch)[0]
    t0 = time.perf_counter()
    host = SlidingWindowDecoder(plan, **kw)  # the fall-back of the default: the host window loop
    res["create_s_host_loop"] = time.perf_counter() - t0
    assert host.window_loop == "host"
    total_dev, total_host = dec.decode(det).copy(), host.decode(det).copy()  # warm-up of both
    stats_dev = dec.last_stats.copy()
    ts = {"device": [], "host": []}
    for _ in range(args.repeats):  # the two alternate: whatever else the machine does hits both
        for name, d in (("device", dec), ("host", host)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            d.decode(det)
            torch.cuda.synchronize()
            ts[name].append(time.perf_counter() - t)
    for name, t in ts.items():
        t.sort()
        res[f"b_decode_{name}_loop_decodes_per_s"] = {"s": t[len(t) // 2], "s_all": t, "per_s": len(det) / t[len(t) // 2]}
    res["same_faults"] = bool(np.array_equal(total_dev, total_host) and np.array_equal(stats_dev[:, :, :2], host.last_stats[:, :, :2]))
    res["device_loop_over_host_loop"] = res["b_decode_device_loop_decodes_per_s"]["per_s"] / res["b_decode_host_loop_decodes_per_s"]["per_s"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
