#!/usr/bin/env python
"""What the circuit sampler costs: [[144,12,12]], 12 rounds, p = 0.003, batches of 4096 and 65 536 shots.

  (a) shots/s of CircuitSampler.sample_device and measure_device (bytes and packed), next to DemSampler.sample_device on the plan of
      the same experiment: each alone on one stream, HIP events around N calls after a warm-up
  (b) shots/s of MemoryExperiment.bb(144, 0.003, 12, 3, 1).run() with the DEM sampler and with sampler="circuit", two lanes
Every figure is the median of --repeats timed windows; all of them are kept, so the spread of the yardstick -- the DEM-sampled
experiment -- shows.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="sampler calls per timed window")
    ap.add_argument("--steps", type=int, default=12, help="batches per timed run() of the 4096-shot experiment (the 65 536-shot one: a quarter)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--osd-order", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "circuit_sampler_rate.json"))
    args = ap.parse_args()
    import torch
    import bench
    from slidingwindowdecoder_amd import CircuitSampler, MemoryExperiment
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    cur = torch.cuda.current_stream(dev)
    kw = dict(bench.DECODER_KW, osd_order=args.osd_order)
    exps = {"dem": MemoryExperiment.bb(144, 0.003, 12, 3, 1, **kw), "circuit": MemoryExperiment.bb(144, 0.003, 12, 3, 1, sampler="circuit", **kw)}
    dem, cir = exps["dem"].sampler, exps["circuit"].sampler
    assert isinstance(cir, CircuitSampler) and cir.num_det == dem.num_det
    info = cir.info()
    res = {"workload": f"[[144,12,12]] 12 rounds p=0.003 (3,1), osd_cs {args.osd_order}", "device": torch.cuda.get_device_name(0),
           "calls": args.calls, "steps": args.steps, "repeats": args.repeats,
           "circuit": {k: int(info[k]) for k in ("qubits", "measurements", "detectors", "observables", "noise_slots", "random_slots")},
           "ops": len(cir.program), "philox_calls_per_shot": (int(info["noise_slots"]) + 3) // 4 + (int(info["random_slots"]) + 127) // 128,
           "dem_columns": dem.num_col}

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(cur)
        for i in range(n):
            fn(i)
        e1.record(cur)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(fn, n, B):
        timed(fn, 2)
        ms = sorted(timed(fn, n) for _ in range(args.repeats))
        return {"ms_per_call": ms[len(ms) // 2] / n, "ms_per_call_all": [x / n for x in ms], "shots_per_s": B * n / (ms[len(ms) // 2] * 1e-3)}

    for B in (4096, 65536):
        det = torch.empty((B, cir.num_det), dtype=torch.uint8, device=dev)
        flips = torch.empty((B,), dtype=torch.int32, device=dev)
        rec = torch.empty((B, cir.num_meas), dtype=torch.uint8, device=dev)
        bits = torch.empty((B, cir.record_bytes(True)), dtype=torch.uint8, device=dev)
        r = {}
        r["dem_sample_device"] = measure(lambda i: dem.sample_device(B, first_shot=i * B, out=(det, flips)), args.calls, B)
        r["circuit_sample_device"] = measure(lambda i: cir.sample_device(B, first_shot=i * B, out=(det, flips)), args.calls, B)
        r["circuit_measure_device"] = measure(lambda i: cir.measure_device(B, first_shot=i * B, out=rec), args.calls, B)
        r["circuit_measure_device_packed"] = measure(lambda i: cir.measure_device(B, first_shot=i * B, packed=True, out=bits), args.calls, B)
        r["circuit_over_dem_sample"] = r["circuit_sample_device"]["ms_per_call"] / r["dem_sample_device"]["ms_per_call"]
        steps = args.steps if B == 4096 else max(2, args.steps // 4)
        for name, exp in exps.items():
            def once():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(cur)
                out = exp.run(steps * B, batch=B, lanes=2)
                e1.record(cur)
                e1.synchronize()
                return e0.elapsed_time(e1), out
            once()
            got = sorted((once() for _ in range(args.repeats)), key=lambda t: t[0])
            ms, out = got[len(got) // 2]
            r[f"run_{name}"] = {"ms_per_step": ms / steps, "ms_per_step_all": [t[0] / steps for t in got], "shots_per_s": B * steps / (ms * 1e-3),
                                "steps": steps, "shots": out.shots, "logical_errors": out.logical_errors, "ler": out.ler}
        r["run_circuit_over_run_dem"] = r["run_circuit"]["ms_per_step"] / r["run_dem"]["ms_per_step"]
        res[f"batch_{B}"] = r
        del det, flips, rec, bits
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
