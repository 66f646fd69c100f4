#!/usr/bin/env python
"""What a rolling memory experiment costs per window step.

Workload: bench.py's headline code and decoder arguments -- [[144,12,12]], p = 0.003, (W, F) = (3, 1), `DECODER_KW` at its default OSD
order, its batch of shots -- at the headline's 12 rounds and at one long experiment (--rounds).  One template (the smallest
`RollingMemoryExperiment.bb` accepts) serves both.  Timed with HIP events, the median of --repeats timed regions after a warm-up:
  (a) the BARE loop: one `swd_pipeline_rolling_push_dev` per window (then `finish_dev`) on rows sampled beforehand (`DemSampler` on
      `windows.extend_template`), one lane and two lanes -- a lane is a stream and a `RollingSession`.  It calls nothing this
      feature added to the library, so it is also timed on the parent commit's build: run the script with --bare-only and
      SWD_LIB naming that build, and hand its output to the full run with --parent-bare
  (b) `RollingMemoryExperiment.run()`, one lane and two lanes: per window the sampler call, the window step and its counts
  (c) `MemoryExperiment.run()` on the plan of 12 rounds: the one-launch form of the same experiment
  (d) alone, back to back on one stream: the sampler call of a body step and the accounting of one window's records
  (e) the device bytes the lanes own after the run of each length
Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    defaults = bench.parse_args([])
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, nargs="+", default=[12, 200])
    ap.add_argument("--batch", type=int, default=defaults.shots)
    ap.add_argument("--window-steps", type=int, default=400, help="window steps per timed region at least (whole batches are run)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bare-only", action="store_true", help="(a) alone: what runs on a build that predates the rolling sampler")
    ap.add_argument("--parent-bare", default=None, help="JSON a --bare-only run on the parent commit's build wrote: merged in, ratios against it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rolling_experiment_rate.json"))
    args = ap.parse_args()
    import torch
    from slidingwindowdecoder_amd import DemSampler, SlidingWindowDecoder
    from slidingwindowdecoder_amd import _lib as L
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import extend_template, plan_windows, rolling_schedule, rolling_template
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    cur = torch.cuda.current_stream(dev)
    kw = dict(bench.DECODER_KW, osd_order=defaults.osd_order)
    N, p, W, F, B = 144, 0.003, 3, 1, args.batch
    code, A, Bm = bb_code(N)
    R0 = 5  # head, two body windows, tail: the smallest (3, 1) template rolling_template accepts
    dem = bb_dem(code, A, Bm, p, R0)
    tplan = plan_windows(dem.chk, dem.obs, dem.priors, N // 2, W, F, method=1)
    T = rolling_template(tplan)
    h = T.n_half
    lib = L.lib()

    def region(fn):
        """ms of fn() between two events on the current stream; fn leaves its lanes joined"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(cur)
        fn()
        torch.cuda.synchronize()
        e1.record(cur)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def figure(fn, steps):
        fn()
        ms = sorted(region(fn) for _ in range(args.repeats))
        return {"ms_per_window_step": ms[len(ms) // 2] / steps, "ms_per_window_step_all": [x / steps for x in ms], "window_steps": steps,
                "windows_per_s": B * steps / (ms[len(ms) // 2] * 1e-3)}

    res = {"workload": f"[[144,12,12]] BB, circuit-level p={p}, (W,F)=({W},{F}), template of {R0} rounds, osd_window("
                       f"pre=8, post=200, alpha=1.0, osd_cs order {defaults.osd_order})", "batch": B, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(L.LIB_PATH), "rounds": {}}
    dec = SlidingWindowDecoder(tplan, **kw)
    lanes = [dict(stream=torch.cuda.Stream(dev, priority=-(k & 1)), session=dec.rolling_session(B),
                  stats=torch.empty((B, 8), dtype=torch.int32, device=dev), shot=torch.empty((B, 2), dtype=torch.int32, device=dev)) for k in range(2)]

    def bare_batch(ln, det, sched):
        ses, st = ln["session"], ln["stream"].cuda_stream
        first, count = C.c_int64(), C.c_int32()
        ses.begin(B)
        for b0, n in sched[:-1]:
            rows = det[:, b0 * h:]
            if lib.swd_pipeline_rolling_push_dev(ses._h, n * h, rows.data_ptr(), rows.stride(0), 1, None, ln["stats"].data_ptr(), None,
                                                 C.byref(first), C.byref(count), st) or count.value != 1:
                raise RuntimeError(L.last_error())
        b0, n = sched[-1]
        rows = det[:, b0 * h:]
        if lib.swd_pipeline_rolling_finish_dev(ses._h, n * h, rows.data_ptr(), rows.stride(0), None, ln["stats"].data_ptr(), None,
                                               ln["shot"].data_ptr(), st):
            raise RuntimeError(L.last_error())

    exp = None
    if not args.bare_only:
        from slidingwindowdecoder_amd import MemoryExperiment, RollingMemoryExperiment
        exp = RollingMemoryExperiment(tplan, **kw)
    for R in args.rounds:
        sched = rolling_schedule(T, R)
        nwin = len(sched)
        batches = max(2, -(-args.window_steps // nwin))
        batches += batches & 1  # (both lanes get the same number)
        chk, obs, priors = extend_template(T, R)
        smp = DemSampler(chk, obs, priors)
        data = [smp.sample_device(B, first_shot=k * (1 << 24))[0] for k in range(2)]
        out = {"windows_per_shot": nwin, "batches_per_region": batches}
        for nl in (1, 2):
            def bare(nl=nl):
                for j in range(batches):
                    bare_batch(lanes[j % nl], data[j & 1], sched)
            out[f"a_bare_push_loop_{nl}_lane"] = figure(bare, batches * nwin)
        del smp, data
        if exp is not None:
            for nl in (1, 2):
                cnt = {}

                def run(nl=nl, cnt=cnt):
                    r = exp.run(batches * B, rounds=R, batch=B, lanes=nl)
                    cnt.update(shots=r.shots, logical_errors=r.logical_errors, flagged=r.flagged, observable_mismatches=r.observable_mismatches)
                out[f"b_run_{nl}_lane"] = dict(figure(run, batches * nwin), **cnt)
            out["e_device_bytes_of_the_lanes"] = int(exp.device_bytes)
            for nl in (1, 2):
                out[f"run_over_bare_{nl}_lane"] = out[f"b_run_{nl}_lane"]["ms_per_window_step"] / out[f"a_bare_push_loop_{nl}_lane"]["ms_per_window_step"]
        res["rounds"][str(R)] = out
    dec.check_status()
    if exp is not None:
        # (c) the one-launch form at the headline's 12 rounds
        plan12 = bench.build_problem(**bench.WORKLOADS["headline"]["problem"])
        one = MemoryExperiment(plan12, **kw)
        nb = 24
        cnt = {}

        def one_launch():
            r = one.run(nb * B, batch=B, lanes=2)
            cnt.update(shots=r.shots, logical_errors=r.logical_errors, flagged=r.flagged, observable_mismatches=r.observable_mismatches)
        res["c_memory_experiment_12_rounds_2_lanes"] = dict(figure(one_launch, nb * one.W), **cnt)
        # (d) the two small kernels of a body step alone
        ln = exp._lane(0, B)
        flips, stats, shot = ln["flips"], ln["stats"], ln["shot_result"]
        wc = torch.zeros((3, L.WINDOW_COUNTER_WORDS), dtype=torch.int64, device=dev)
        stats.zero_()
        shot.zero_()
        flips.zero_()
        calls = 200

        def sampler_calls():
            for _ in range(calls):
                if lib.swd_rolling_sampler_rows_dev(exp.sampler._h, B, 20240318, 0, 12, 5, 1, ln["rows"].data_ptr(), ln["rows"].stride(0),
                                                    flips.data_ptr(), None, 0, cur.cuda_stream):
                    raise RuntimeError(L.last_error())

        def account_calls():
            for _ in range(calls):
                if lib.swd_shot_account_dev(0, B, 1, shot.data_ptr(), flips.data_ptr(), stats.data_ptr(), 0, None, None, wc[1].data_ptr(), None, 0,
                                            cur.cuda_stream):
                    raise RuntimeError(L.last_error())
        for name, fn in (("d_kernel_rolling_sampler_body_step", sampler_calls), ("d_kernel_window_account_step", account_calls)):
            f = figure(fn, calls)
            res[name] = {"ms_per_call": f["ms_per_window_step"], "ms_per_call_all": f["ms_per_window_step_all"]}
        res["d_body_step_columns_drawn"] = int(exp.sampler.columns(12, 4, 2)[1])
        r12 = res["rounds"].get("12")
        if r12:
            small = res["d_kernel_rolling_sampler_body_step"]["ms_per_call"] + res["d_kernel_window_account_step"]["ms_per_call"]
            res["small_kernels_over_bare_window_step_1_lane"] = small / r12["a_bare_push_loop_1_lane"]["ms_per_window_step"]
            res["run_12_rounds_over_memory_experiment_windows_per_s"] = r12["b_run_2_lane"]["windows_per_s"] / \
                res["c_memory_experiment_12_rounds_2_lanes"]["windows_per_s"]
        b = [v["e_device_bytes_of_the_lanes"] for v in res["rounds"].values()]
        res["device_bytes_equal_at_every_length"] = len(set(b)) == 1
    if args.parent_bare and os.path.exists(args.parent_bare):
        par = json.load(open(args.parent_bare))
        res["parent_build"] = {"library": par.get("library"), "rounds": par["rounds"]}
        for R, out in res["rounds"].items():
            for nl in (1, 2):
                a = par["rounds"].get(R, {}).get(f"a_bare_push_loop_{nl}_lane")
                if a and f"b_run_{nl}_lane" in out:
                    out[f"run_over_parent_bare_{nl}_lane"] = out[f"b_run_{nl}_lane"]["ms_per_window_step"] / a["ms_per_window_step"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
