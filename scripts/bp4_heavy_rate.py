#!/usr/bin/env python3
"""What camel_decode costs on the code Misc.ipynb cell 8 runs.

Workload: the [[362,36,20]] cycle-assembled code of tests/golden/bp4_heavy.npz (its last qubit has weight 171 in Hx and in Hz: the
HEAVY form of the BP kernel), depolarizing p = 0.02 with cell 8's uniform priors and parameters (max_iter=50, ms_scaling_factor=0.8,
osd_method="osd0", osd_order=-1), camel_decode through CodeCapacityExperiment: sample + four BP4 runs per shot + select + account.
Four figures:
  camel_decodes_per_s      shots/s of CodeCapacityExperiment.run (HIP events around the run, median of --repeats after a warm-up)
  not_converged            of 100 000 shots, beside the notebook's recorded 26 / 100 000 (another RNG: a statistical match at best)
  oracle_cpu_shots_per_s   the CPU oracle's camel_decode on syndromes of the same distribution, 16 processes on this machine
  bb144_decodes_per_s      the [[144]] line of scripts/bp4_codes_rate.py in child processes, this build and (--parent-lib, a build
                           of the parent commit next to the package or given by path) the parent's, alternating, --ab-repeats each:
                           graphs without heavy columns must not have become slower
and what an UNDECIDED heavy node costs per iteration (in camel_decode on this code the heavy qubit is the decided one and is never
updated): plain decode, osd_order = -1, on random syndromes -- no shot converges, every shot runs exactly max_iter iterations -- on
the [[362]] graph (HEAVY form: per iteration one lane adds 171 + 171 check messages in order, then a barrier and one edge per thread)
against the same graph without its last column in the generic form (SWD_BP4_GENERIC, a child process): heavy_node_cost.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KW = dict(max_iter=50, ms_scaling_factor=0.8, osd_method="osd0", osd_order=-1)


def load_code():
    f = np.load(os.path.join(ROOT, "tests", "golden", "bp4_heavy.npz"), allow_pickle=False)
    mx, mz, n = (int(x) for x in f["camel362_shape"])
    unpack = lambda a: np.unpackbits(a, axis=-1)[..., :n]
    return unpack(f["camel362_hx"]), unpack(f["camel362_hz"]), n


def _oracle_worker(args):
    seed, shots, p = args
    from oracle import oracle as O
    Hx, Hz, n = load_code()
    pr = np.full(n, p / 3)
    rng = np.random.default_rng(seed)
    pauli = rng.choice(4, size=(shots, n), p=[1 - p, p / 3, p / 3, p / 3])
    ex, ez = ((pauli == 1) | (pauli == 2)).astype(np.uint8), ((pauli == 3) | (pauli == 2)).astype(np.uint8)
    sx, sz = (ez @ Hx.T % 2).astype(np.uint8), (ex @ Hz.T % 2).astype(np.uint8)
    dec = O.bp4_osd(Hx, Hz, channel_probs_x=pr, channel_probs_y=pr, channel_probs_z=pr, **KW)
    t0 = time.perf_counter()
    for k in range(shots):
        dec.camel_decode(sx[k], sz[k])
    return time.perf_counter() - t0


def oracle_rate(procs, shots, p):
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(procs) as pool:
        t0 = time.perf_counter()
        busy = pool.map(_oracle_worker, [(100 + i, shots, p) for i in range(procs)])
        wall = time.perf_counter() - t0
    # (the workers' own decode time: the pool's start-up and the syndrome sampling are not the decoder's)
    return {"processes": procs, "shots_per_process": shots, "shots_per_s": procs * shots / max(busy), "wall_s_with_startup": wall}


def bb144_rate(lib, batch):
    env = dict(os.environ)
    if lib:
        env["SWD_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bp4_codes_rate.py"), str(batch)], capture_output=True, text=True,
                       env=env, cwd=ROOT, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bp4_codes_rate.py failed ({r.returncode}): {r.stdout[-1000:]}{r.stderr[-2000:]}")
    for line in r.stdout.splitlines():
        if line.startswith("{") and json.loads(line)["code"] == "bb144":
            d = json.loads(line)
            return {k: d[k] for k in ("decodes_per_s", "two_streams_decodes_per_s", "checksum")}
    raise RuntimeError("no bb144 line")


def heavy_node_child(batch, launches):
    """(child process, SWD_BP4_GENERIC=1) ms per launch of plain decode on never-converging syndromes: with and without the last column"""
    import torch
    from slidingwindowdecoder_amd import bp4_osd
    dev = torch.device("cuda", 0)
    Hx, Hz, n = load_code()
    out = {}
    for name, hx, hz in (("heavy", Hx, Hz), ("light", Hx[:, :-1], Hz[:, :-1])):
        nn = hx.shape[1]
        pr = np.full(nn, 0.02 / 3)
        dec = bp4_osd(hx, hz, channel_probs_x=pr, channel_probs_y=pr, channel_probs_z=pr, max_iter=50, ms_scaling_factor=0.8,
                      osd_method="osd_cs", osd_order=-1)
        rng = np.random.default_rng(3)
        sx = torch.from_numpy((rng.random((batch, hx.shape[0])) < 0.5).astype(np.uint8)).to(dev)
        sz = torch.from_numpy((rng.random((batch, hz.shape[0])) < 0.5).astype(np.uint8)).to(dev)
        o = torch.empty((batch, 2, nn), dtype=torch.uint8, device=dev)
        st = torch.empty((batch, 8), dtype=torch.int32, device=dev)
        for _ in range(2):
            dec.decode_batch_device(sx, sz, out=o, stats=st)
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                dec.decode_batch_device(sx, sz, out=o, stats=st)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / launches)
        stats = st.cpu().numpy()
        out[name] = {"n": nn, "heavy_columns": list(dec.heavy_columns), "form": dec.last_form, "ms_per_launch_all": ms,
                     "ms_per_launch": sorted(ms)[1], "mean_iterations": float(stats[:, 1].mean()),
                     "converged": int(((stats[:, 0] & 0x100) != 0).sum())}
    h, l = out["heavy"], out["light"]
    out.update(batch=batch, launches=launches,
               us_per_decode_iteration_heavy=h["ms_per_launch"] * 1e3 / batch / h["mean_iterations"],
               us_per_decode_iteration_light=l["ms_per_launch"] * 1e3 / batch / l["mean_iterations"],
               heavy_over_light=h["ms_per_launch"] / l["ms_per_launch"])
    print(json.dumps(out))


def heavy_node_cost(batch, launches):
    env = dict(os.environ, SWD_BP4_GENERIC="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--heavy-node-child", "--batch", str(batch), "--repeats", str(launches)],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"heavy-node child failed ({r.returncode}): {r.stdout[-1000:]}{r.stderr[-2000:]}")
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heavy-node-child", action="store_true", help="(internal) the child process of heavy_node_cost")
    ap.add_argument("--shots", type=int, default=100000)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--oracle-procs", type=int, default=16)
    ap.add_argument("--oracle-shots", type=int, default=150, help="per process")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit (SWD_LIB of the child processes)")
    ap.add_argument("--ab-repeats", type=int, default=2)
    ap.add_argument("--ab-batch", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bp4_heavy_rate.json"))
    args = ap.parse_args()
    if args.heavy_node_child:
        return heavy_node_child(args.batch, args.repeats)
    Hx, Hz, n = load_code()
    p = 0.02
    pr = np.full(n, p / 3)
    res = {"workload": "CAMEL [[362,36,20]] depolarizing p=0.02, camel_decode, bp4_osd(50, 0.8, osd0, -1)", "shots": args.shots,
           "batch": args.batch, "lanes": args.lanes, "notebook_not_converged": "26 / 100000"}
    # everything that runs in child processes first, before this process opens the device: the CPU oracle, then the [[144]] A/B
    res["oracle_cpu"] = oracle_rate(args.oracle_procs, args.oracle_shots, p)
    ab = {"this": [], "parent": []}
    for _ in range(args.ab_repeats):
        ab["this"].append(bb144_rate(None, args.ab_batch))
        if args.parent_lib:
            ab["parent"].append(bb144_rate(args.parent_lib, args.ab_batch))
    res["bb144_decodes_per_s"] = ab
    res["heavy_node_cost"] = heavy_node_cost(16384, 5)
    import torch
    from slidingwindowdecoder_amd import CodeCapacityExperiment
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda", 0)
    res["device"] = torch.cuda.get_device_name(0)
    exp = CodeCapacityExperiment((Hx, Hz), decoder="bp4_osd", method="camel_decode", channel_probs_x=pr, channel_probs_y=pr,
                                 channel_probs_z=pr, **KW)
    res["heavy_columns"] = list(exp.decoder.heavy_columns)
    cur = torch.cuda.current_stream(dev)

    def once(shots):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(cur)
        r = exp.run(shots, batch=args.batch, lanes=args.lanes)
        e1.record(cur)
        e1.synchronize()
        return e0.elapsed_time(e1), r
    once(2 * args.batch * args.lanes)  # warm-up: every buffer and code object of the timed runs
    got = sorted((once(args.shots) for _ in range(args.repeats)), key=lambda t: t[0])
    ms, r = got[len(got) // 2]
    res["camel_decodes_per_s"] = r.shots / (ms * 1e-3)
    res["camel_bp4_runs_per_s"] = 4 * r.shots / (ms * 1e-3)
    res["ms_all"] = [t[0] for t in got]
    res.update(shots_run=r.shots, not_converged=r.not_converged, logical_errors=r.logical_errors, residual_syndromes=r.residual_syndromes)
    res["form"] = exp.decoder.last_form
    res["device_over_oracle_16_processes"] = res["camel_decodes_per_s"] / res["oracle_cpu"]["shots_per_s"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
