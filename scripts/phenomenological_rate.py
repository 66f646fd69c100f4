#!/usr/bin/env python
"""Windows per second of the phenomenological-noise memory experiments.

[[144,12,12]], (W, F) = (3, 1), p = q = 0.01, bench.py's decoder arguments, batches of 4096 shots on two lanes; every figure is the
median of --repeats timed runs after a warm-up run, all of them kept:
  z            MemoryExperiment.phenomenological, basis z, 12 rounds
  depolarizing the both / depolarizing form of the same code (144 detectors a round, 24 observables); it counts its Z and X logical
               errors apart by default, so it is timed with and without that, the runs ALTERNATING in one process: the ratio of the
               medians beside the spread of the ungrouped repeats
  rolling      RollingMemoryExperiment.phenomenological, basis z, at 12 and at 200 rounds
The circuit-level figure of profiles/memory_experiment_rate.json stands beside them for scale.  A construction that the pipeline
refuses is recorded with its message.  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--steps", type=int, default=16, help="batches per timed run")
    ap.add_argument("--long-steps", type=int, default=2, help="batches per timed run of the 200-round experiment")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--p", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phenomenological_rate.json"))
    args = ap.parse_args()
    import torch
    from slidingwindowdecoder_amd import MemoryExperiment, RollingMemoryExperiment
    from slidingwindowdecoder_amd.codes import bb_code
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    cur = torch.cuda.current_stream(dev)
    code = bb_code(144)[0]
    kw = dict(bench.DECODER_KW, osd_order=defaults.osd_order)
    B = args.batch

    def once(exp, steps, **run_kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(cur)
        r = exp.run(steps * B, batch=B, lanes=2, **run_kw)
        e1.record(cur)
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def figure(times, r, steps, windows):
        ms = sorted(times)
        mid = ms[len(ms) // 2]
        out = {"ms_per_step": mid / steps, "ms_per_step_all": [x / steps for x in times], "windows_per_shot": windows,
               "shots_per_s": B * steps / (mid * 1e-3), "windows_per_s": B * windows * steps / (mid * 1e-3),
               "spread": (ms[-1] - ms[0]) / mid, "shots": r.shots, "logical_errors": r.logical_errors, "flagged": r.flagged}
        if r.group_errors:
            out["group_errors"] = r.group_errors
        return out

    def measure(exp, steps, windows, **run_kw):
        once(exp, 2, **run_kw)
        got = [once(exp, steps, **run_kw) for _ in range(args.repeats)]
        return figure([t for t, _ in got], got[0][1], steps, windows)

    def attempt(build):
        try:
            return build(), None
        except (ValueError, RuntimeError) as e:  # a plan outside the pipeline's bounds: the refusal is the finding
            return None, f"{type(e).__name__}: {e}"

    res = {"code": "[[144,12,12]] BB", "p": args.p, "q": args.p, "geometry": [3, 1], "batch": B, "steps": args.steps, "repeats": args.repeats,
           "lanes": 2, "decoder": "osd_window " + json.dumps(kw, sort_keys=True), "device": torch.cuda.get_device_name(0)}
    exp, why = attempt(lambda: MemoryExperiment.phenomenological(code, args.p, 12, 3, 1, basis="z", **kw))
    if exp is None:
        res["z_12_rounds"] = {"refused": why}
    else:
        w = exp.plan.windows[0]
        res["z_12_rounds"] = dict(measure(exp, args.steps, exp.W), window_shape=list(w.mat.shape), threads=exp.decoder.threads)
        exp.close()
    exp, why = attempt(lambda: MemoryExperiment.phenomenological(code, args.p, 12, 3, 1, basis="both", noise="depolarizing", **kw))
    if exp is None:
        res["depolarizing_12_rounds"] = {"refused": why}
    else:
        w = exp.plan.windows[0]
        once(exp, 2)
        once(exp, 2, observable_groups={})
        with_groups, without = [], []
        for _ in range(args.repeats):  # alternating, so that drift lands on both
            without.append(once(exp, args.steps, observable_groups={}))
            with_groups.append(once(exp, args.steps))
        a = figure([t for t, _ in without], without[0][1], args.steps, exp.W)
        b = figure([t for t, _ in with_groups], with_groups[0][1], args.steps, exp.W)
        res["depolarizing_12_rounds"] = dict(a, window_shape=list(w.mat.shape), threads=exp.decoder.threads)
        res["depolarizing_12_rounds_with_groups"] = b
        res["groups_over_no_groups"] = b["ms_per_step"] / a["ms_per_step"]
        res["no_groups_spread"] = a["spread"]
        exp.close()
    exp, why = attempt(lambda: RollingMemoryExperiment.phenomenological(code, args.p, 12, 3, 1, basis="z", **kw))
    if exp is None:
        res["rolling_z"] = {"refused": why}
    else:
        res["rolling_template_rounds"] = exp.template.R0
        res["rolling_z_12_rounds"] = measure(exp, args.steps, 12 + 1 - 3 + 1, rounds=12)
        res["rolling_z_200_rounds"] = measure(exp, args.long_steps, 200 + 1 - 3 + 1, rounds=200)
        res["rolling_device_bytes"] = exp.device_bytes
        exp.close()
    ref = os.path.join(ROOT, "profiles", "memory_experiment_rate.json")
    if os.path.exists(ref):
        with open(ref) as f:
            circuit = json.load(f)
        res["circuit_level_for_scale"] = {"workload": circuit["workload"], "windows_per_s": circuit["b_run_2_lanes"]["windows_per_s"],
                                          "ms_per_step": circuit["b_run_2_lanes"]["ms_per_step"], "source": "profiles/memory_experiment_rate.json"}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
