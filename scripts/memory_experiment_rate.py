#!/usr/bin/env python
"""What the device-side memory experiment costs on top of the window loop.

Workload: bench.py's headline -- its plan (`build_problem()`), its decoder arguments (`DECODER_KW` at its default OSD order) and its
batch of shots per step.  Timed with HIP events around N steps after a warm-up, the median of three timed windows:
  (a) streamed decode alone on detector data sampled beforehand, two batches in flight (SlidingWindowStream.push_device): the
      figure bench.py reports
  (b) MemoryExperiment.run() with two lanes: sample + window loop + account per step, counters read once at the end
  (a) and (b) also over 4 N steps, which separates what a timed window pays once (filling and draining the two lanes, and for run()
  the zeroed counters and the read-back) from what it pays per step
  (c) MemoryExperiment.run() with one lane, next to decode_device alone on one stream
  (d) the DEM sampler, the accounting kernel and one decode launch, each alone on one batch
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    defaults = bench.parse_args([])
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--batch", type=int, default=defaults.shots)
    ap.add_argument("--repeats", type=int, default=3, help="timed windows per figure; the median is reported, all are kept")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memory_experiment_rate.json"))
    args = ap.parse_args()
    import torch
    from slidingwindowdecoder_amd import MemoryExperiment
    from slidingwindowdecoder_amd import _lib as L
    from slidingwindowdecoder_amd.decoders import shot_account_device
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    plan = bench.build_problem(**bench.WORKLOADS["headline"]["problem"])
    kw = dict(bench.DECODER_KW, osd_order=defaults.osd_order)
    exp = MemoryExperiment(plan, **kw)
    dec, smp = exp.decoder, exp.sampler
    B, N, W = args.batch, args.steps, exp.W
    cur = torch.cuda.current_stream(dev)
    # distinct batches of detector data and one set of output buffers per lane, as bench.py's GpuEngine keeps them
    data = [smp.sample_device(B, first_shot=k * (1 << 24)) for k in range(defaults.distinct_batches)]
    outs = [dict(total=torch.empty((B, dec.num_col), dtype=torch.uint8, device=dev),
                 stats=torch.empty((B, W, 8), dtype=torch.int32, device=dev),
                 shot_result=torch.empty((B, 2), dtype=torch.int32, device=dev)) for _ in range(2)]
    stream = dec.stream(B)
    for k in range(2):  # the first launch on a lane creates its hardware queue
        stream.push_device(data[0][0], min_pm=None, **outs[k])
    stream.wait()
    torch.cuda.synchronize()

    def timed(fn, steps, join=None):
        """ms of fn(step) for step in range(steps) between two events on the current stream"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(cur)
        for i in range(steps):
            fn(i)
        if join is not None:
            join()
        e1.record(cur)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(fn, steps, join=None):
        timed(fn, args.warmup, join)
        ms = sorted(timed(fn, steps, join) for _ in range(args.repeats))
        return {"ms_per_step": ms[len(ms) // 2] / steps, "ms_per_step_all": [x / steps for x in ms],
                "shots_per_s": B * steps / (ms[len(ms) // 2] * 1e-3), "windows_per_s": B * W * steps / (ms[len(ms) // 2] * 1e-3)}

    def run_with(nl, N=N):
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
                "windows_per_s": B * W * N / (ms * 1e-3), "shots": r.shots, "logical_errors": r.logical_errors, "flagged": r.flagged,
                "observable_mismatches": r.observable_mismatches}

    res = {"workload": bench.WORKLOADS["headline"]["desc"] % defaults.osd_order, "batch": B, "steps": N, "warmup": args.warmup,
           "windows_per_shot": W, "device": torch.cuda.get_device_name(0)}
    res["a_stream_decode_2_in_flight"] = measure(lambda i: stream.push_device(data[i % len(data)][0], min_pm=None, **outs[i & 1]), N,
                                                 join=lambda: stream.wait(cur))
    res["a_stream_decode_2_in_flight_4x_steps"] = measure(lambda i: stream.push_device(data[i % len(data)][0], min_pm=None, **outs[i & 1]), 4 * N,
                                                          join=lambda: stream.wait(cur))
    res["b_run_2_lanes"] = run_with(2)
    # the same over four times the steps: what run() pays once (zeroed counters, the drain, the read-back) against what it pays per step
    res["b_run_2_lanes_4x_steps"] = run_with(2, 4 * N)
    res["c_decode_device_1_in_flight"] = measure(lambda i: dec.decode_device(data[i % len(data)][0], want_min_pm=False, **outs[0]), N)
    res["c_run_1_lane"] = run_with(1)
    # (d) each kernel alone, back to back on one stream, one batch
    det, flips = data[0]
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    wc = torch.zeros((W, 10), dtype=torch.int64, device=dev)
    result = torch.empty((B,), dtype=torch.int32, device=dev)
    dec.decode_device(det, want_min_pm=False, **outs[0])

    def sample(i):
        if L.lib().swd_sampler_sample_dev(smp._h, B, 20240318, 0, det.data_ptr(), 0, flips.data_ptr(), None, 0, cur.cuda_stream):
            raise RuntimeError(L.last_error())
    res["d_kernel_dem_sampler"] = measure(sample, 20)
    res["d_kernel_shot_account"] = measure(lambda i: shot_account_device(outs[0]["shot_result"], flips, outs[0]["stats"], 0, result, counters, wc), 20)
    res["d_kernel_decode_launch"] = measure(lambda i: dec.decode_device(det, want_min_pm=False, **outs[0]), 20)
    dec.check_status()
    a, b = res["a_stream_decode_2_in_flight"]["ms_per_step"], res["b_run_2_lanes"]["ms_per_step"]
    small = res["d_kernel_dem_sampler"]["ms_per_step"] + res["d_kernel_shot_account"]["ms_per_step"]
    res["run_2_lanes_over_stream_decode"] = b / a
    res["run_1_lane_over_decode_device"] = res["c_run_1_lane"]["ms_per_step"] / res["c_decode_device_1_in_flight"]["ms_per_step"]
    res["expectation_ms_per_step"] = a + small  # (a) plus the stand-alone times of the two small kernels
    res["run_2_lanes_over_expectation"] = b / (a + small)
    b4 = res["b_run_2_lanes_4x_steps"]["ms_per_step"]
    res["run_2_lanes_ms_per_additional_step"] = (4 * N * b4 - N * b) / (3 * N)
    res["run_2_lanes_ms_once_per_run"] = N * b - N * res["run_2_lanes_ms_per_additional_step"]
    a4 = res["a_stream_decode_2_in_flight_4x_steps"]["ms_per_step"]
    res["stream_decode_ms_per_additional_step"] = (4 * N * a4 - N * a) / (3 * N)
    res["stream_decode_ms_once_per_window"] = N * a - N * res["stream_decode_ms_per_additional_step"]
    res["run_2_lanes_over_stream_decode_per_additional_step"] = res["run_2_lanes_ms_per_additional_step"] / res["stream_decode_ms_per_additional_step"]
    res["sampler_over_decode_launch"] = res["d_kernel_dem_sampler"]["ms_per_step"] / res["d_kernel_decode_launch"]["ms_per_step"]
    res["account_over_decode_launch"] = res["d_kernel_shot_account"]["ms_per_step"] / res["d_kernel_decode_launch"]["ms_per_step"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
