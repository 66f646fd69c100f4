#!/usr/bin/env python3
"""Decodes/s of bp4_osd(..., general_osd=True): ``decode`` WITH OSD on the codes whose OSD only the general elimination kernel runs
(huge_bp4_osd_kernel, csrc/swd_huge_bp4.hip).

Workloads: the cycle-assembled [[362,36,20]] at depolarizing p = 0.02 (tuned HEAVY BP kernel + the elimination), EG [[273,111,17]] at
p = 0.06 and EG [[1057,571,33]] at p = 0.04 (general BP form + the elimination); matrices from tests/golden/bp4_heavy.npz /
bp4_general.npz, uniform priors, Misc.ipynb cell 8's BP parameters (max_iter=50, ms_scaling_factor=0.8) -- the workloads of
scripts/bp4_heavy_rate.py / bp4_general_rate.py -- with OSD-0 and with osd_cs 10, --shots syndromes each on device-resident arrays.
Timing: HIP events around one launch (BP kernel + elimination kernel) after a warm-up launch of the same shape; the median of
--repeats launches.  Reported with each figure: the share of shots that reach the OSD, and the CPU oracle's rate on syndromes of the
same distribution in a pool of 16 processes on the same machine (the yardstick of scripts/huge_gdg_rate.py), which runs before this
process opens the device.  The oracle's outputs of those runs (at least 64 shots per code and method) are kept and compared bit for
bit with the device's decode of the same syndromes in the same run.  KERNEL below is the elimination kernel's entry of
``make -C slidingwindowdecoder_amd/csrc resource-usage``.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BP = dict(max_iter=50, ms_scaling_factor=0.8)
METHODS = {"osd0": dict(BP, osd_method="osd0", osd_order=0), "osd_cs10": dict(BP, osd_method="osd_cs", osd_order=10)}
# code: fixture, tag, p, general_form beside general_osd, oracle shots per process
CODES = {"camel362": ("bp4_heavy.npz", "camel362", 0.02, False, 8), "eg273": ("bp4_general.npz", "eg273", 0.06, True, 8),
         "eg1057": ("bp4_general.npz", "eg1057", 0.04, True, 4)}
KERNEL = {"name": "huge_bp4_osd_kernel", "threads": 1024, "vgprs": 128, "sgprs": 106, "scratch_bytes_per_lane": 192, "lds_bytes": 8536}


def load_code(code):
    name, tag, p = CODES[code][:3]
    f = np.load(os.path.join(ROOT, "tests", "golden", name), allow_pickle=False)
    mx, mz, n = (int(x) for x in f[tag + "_shape"])
    unpack = lambda a: np.unpackbits(a, axis=-1)[..., :n]
    Hx = unpack(f[tag + "_hx"])
    Hz = unpack(f[tag + "_hz"]) if tag + "_hz" in f else Hx
    q = np.full(n, p / 3)
    return Hx, Hz, dict(channel_probs_x=q, channel_probs_y=q, channel_probs_z=q), p


def syndromes(Hx, Hz, p, shots, seed):
    rng = np.random.default_rng(seed)
    pauli = rng.choice(4, size=(shots, Hx.shape[1]), p=[1 - p, p / 3, p / 3, p / 3])
    ex, ez = ((pauli == 1) | (pauli == 2)).astype(np.int64), ((pauli == 3) | (pauli == 2)).astype(np.int64)
    return (ez @ Hx.T.astype(np.int64) % 2).astype(np.uint8), (ex @ Hz.T.astype(np.int64) % 2).astype(np.uint8)


def _oracle_worker(args):
    code, method, seed, shots = args
    from oracle import oracle as O
    Hx, Hz, pr, p = load_code(code)
    sx, sz = syndromes(Hx, Hz, p, shots, seed)
    dec = O.bp4_osd(Hx, Hz, **pr, **METHODS[method])
    outs, conv = [], 0
    t0 = time.perf_counter()
    for k in range(shots):
        outs.append(dec.decode(sx[k], sz[k]).astype(np.uint8))
        conv += int(dec.converge)
    return time.perf_counter() - t0, conv, np.array(outs)


def oracle_rate(code, method, procs, shots):
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(procs) as pool:  # fresh processes: none of them has the device open
        got = pool.map(_oracle_worker, [(code, method, 100 + i, shots) for i in range(procs)], chunksize=1)
    # (the workers' own decode time: the pool's start-up and the syndrome sampling are not the decoder's)
    rate = {"processes": procs, "shots_per_process": shots, "decodes_per_s": procs * shots / max(t for t, _, _ in got),
            "converged": sum(c for _, c, _ in got)}
    return rate, np.concatenate([o for _, _, o in got])


def device_rate(code, method, shots, repeats, procs, want):
    import torch
    from slidingwindowdecoder_amd import _lib, bp4_osd
    dev = torch.device("cuda", 0)
    Hx, Hz, pr, p = load_code(code)
    dec = bp4_osd(Hx, Hz, **pr, **METHODS[method], general_osd=True, general_form=CODES[code][3])
    # the oracle's shots, bit for bit (decode keeps no state between shots, so one oracle object per process is a new one per shot)
    per = len(want) // procs
    cs = [syndromes(Hx, Hz, p, per, 100 + i) for i in range(procs)]
    got = dec.decode_batch(np.concatenate([a for a, _ in cs]), np.concatenate([b for _, b in cs]), details=False)
    if not np.array_equal(got, want):
        raise SystemExit(f"{code}/{method}: the device differs from the oracle on {int((got != want).any(axis=(1, 2)).sum())} of {len(want)} shots")
    sx, sz = (torch.from_numpy(a).to(dev) for a in syndromes(Hx, Hz, p, shots, 7))
    out = torch.empty((shots, 2, dec.n), dtype=torch.uint8, device=dev)
    st = torch.empty((shots, _lib.STAT_WORDS), dtype=torch.int32, device=dev)
    cur = torch.cuda.current_stream(dev)
    dec.decode_batch_device(sx, sz, out=out, stats=st)  # warm-up: code objects, the launch slot's scratch areas
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        dec.decode_batch_device(sx, sz, out=out, stats=st)
        e1.record(cur)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    stats = st.cpu().numpy()
    mid = sorted(ms)[len(ms) // 2]
    return {"general_form": bool(dec.general_form), "form": dec.last_form, "ranks": [dec.rank_x, dec.rank_z], "shots": shots, "ms_all": ms,
            "decodes_per_s": shots / (mid * 1e-3), "osd_share": float(((stats[:, 0] & 0xFF) == 2).mean()),
            "mean_iterations": float(stats[:, 1].mean()), "mean_row_additions_per_osd_shot": float(stats[(stats[:, 0] & 0xFF) == 2, 7].mean()),
            "checked_bit_for_bit": len(want), "checksum": int(out.to(torch.int64).sum().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--oracle-procs", type=int, default=16)
    ap.add_argument("--codes", default=",".join(CODES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bp4_general_osd_rate.json"))
    args = ap.parse_args()
    codes = [c for c in args.codes.split(",") if c]
    res = {"shots": args.shots, "repeats": args.repeats, "parameters": "max_iter=50, ms_scaling_factor=0.8", "kernel": KERNEL, "codes": {}}
    want = {}
    for code in codes:  # every child process before this one opens the device
        res["codes"][code] = {"p": CODES[code][2], "oracle_16_processes": {}, "device": {}}
        for method in METHODS:
            res["codes"][code]["oracle_16_processes"][method], want[code, method] = oracle_rate(code, method, args.oracle_procs, CODES[code][4])
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    res["device"] = torch.cuda.get_device_name(0)
    for code in codes:
        r = res["codes"][code]
        for method in METHODS:
            r["device"][method] = device_rate(code, method, args.shots, args.repeats, args.oracle_procs, want[code, method])
            r["device"][method]["over_oracle_16_processes"] = r["device"][method]["decodes_per_s"] / r["oracle_16_processes"][method]["decodes_per_s"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
