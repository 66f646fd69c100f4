#!/usr/bin/env python
"""What the device-side code-capacity experiment costs on top of the decoder.

Workload: bench.py's `bp4` -- [[144,12,12]], depolarizing p = 0.02, bp4_osd(max_iter=100, ms_scaling_factor=0.625, osd_cs, 10),
65 536-shot steps.  Timed with HIP events around N steps after a warm-up, with one launch in flight and with four:
  (a) decode only, on device syndromes made beforehand: swd_bp4_decode_batch_dev alone, the figure bench.py reports
  (b) CodeCapacityExperiment.run(): sample + decode + account per step, counters read once at the end
and each new kernel alone on one 65 536-shot batch (Pauli sampler, CSS accounting), next to the decode launch.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3, help="timed windows per figure; the median is reported, all are kept")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "code_capacity_rate.json"))
    args = ap.parse_args()
    import torch
    from slidingwindowdecoder_amd import CodeCapacityExperiment
    from slidingwindowdecoder_amd.codes import bb_code
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    code, _, _ = bb_code(144)
    n, p, B, N = code.N, 0.02, args.batch, args.steps
    pr = np.full(n, p / 3)
    exp = CodeCapacityExperiment(code, decoder="bp4_osd", channel_probs_x=pr, channel_probs_y=pr, channel_probs_z=pr, max_iter=100,
                                 ms_scaling_factor=0.625, osd_method="osd_cs", osd_order=10)
    dec, smp, acct = exp.decoder, exp.sampler, exp._acct
    cur = torch.cuda.current_stream(dev)
    # four distinct batches of syndromes and four sets of output buffers, as bench.py's Bp4Engine keeps them
    data = [smp.sample_device(B, first_shot=k * B) for k in range(4)]
    outs = [torch.empty((B, 2, n), dtype=torch.uint8, device=dev) for _ in range(4)]
    stat = [torch.empty((B, 8), dtype=torch.int32, device=dev) for _ in range(4)]
    lanes = [torch.cuda.Stream(dev, priority=-(i & 1)) for i in range(4)]
    torch.cuda.synchronize()

    def timed(fn, steps):
        """ms of fn(step) for step in range(steps) between two events on the current stream; fn's lanes are fenced by it"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(cur)
        for ln in lanes:
            ln.wait_stream(cur)
        for i in range(steps):
            fn(i)
        for ln in lanes:
            cur.wait_stream(ln)
        e1.record(cur)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def decode_on(nl):
        def fn(i):
            k = i % 4
            dec.decode_batch_device(data[k][1], data[k][2], out=outs[k], stats=stat[k], stream=lanes[i % nl] if nl > 1 else cur)
        return fn

    def measure(fn, steps):
        timed(fn, args.warmup)
        ms = sorted(timed(fn, steps) for _ in range(args.repeats))
        return {"ms_per_step": ms[len(ms) // 2] / steps, "ms_per_step_all": [x / steps for x in ms],
                "shots_per_s": B * steps / (ms[len(ms) // 2] * 1e-3)}

    def run_with(nl):
        def once(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(cur)
            r = exp.run(steps * B, batch=B, lanes=nl)
            e1.record(cur)
            e1.synchronize()
            return e0.elapsed_time(e1), r
        once(args.warmup)
        got = sorted((once(N) for _ in range(args.repeats)), key=lambda t: t[0])
        ms, r = got[len(got) // 2]
        return {"ms_per_step": ms / N, "ms_per_step_all": [t[0] / N for t in got], "shots_per_s": B * N / (ms * 1e-3),
                "shots": r.shots, "logical_errors": r.logical_errors, "not_converged": r.not_converged}

    res = {"workload": "bb144 depolarizing p=0.02 bp4_osd(100, 0.625, osd_cs, 10)", "batch": B, "steps": N, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    res["decode_only_1_in_flight"] = measure(decode_on(1), N)
    res["decode_only_4_in_flight"] = measure(decode_on(4), N)
    res["run_1_lane"] = run_with(1)
    res["run_4_lanes"] = run_with(4)
    # the new kernels alone, back to back on one stream, one 65 536-shot batch
    err, sx, sz = data[0]
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    result = torch.empty((B,), dtype=torch.int32, device=dev)
    dec.decode_batch_device(sx, sz, out=outs[0], stats=stat[0])
    res["kernel_pauli_sampler"] = measure(lambda i: smp.sample_device(B, first_shot=0, out=data[0]), 20)
    res["kernel_css_account"] = measure(lambda i: acct.account(B, outs[0], err, stat[0], result, counters, cur), 20)
    res["kernel_bp4_decode_launch"] = measure(decode_on(1), 20)
    d1, d4 = res["decode_only_1_in_flight"]["ms_per_step"], res["decode_only_4_in_flight"]["ms_per_step"]
    res["run_over_decode_1"] = res["run_1_lane"]["ms_per_step"] / d1
    res["run_over_decode_4"] = res["run_4_lanes"]["ms_per_step"] / d4
    res["sampler_over_decode_launch"] = res["kernel_pauli_sampler"]["ms_per_step"] / res["kernel_bp4_decode_launch"]["ms_per_step"]
    res["account_over_decode_launch"] = res["kernel_css_account"]["ms_per_step"] / res["kernel_bp4_decode_launch"]["ms_per_step"]
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
