#!/usr/bin/env python3
"""Decodes/s of bp4_osd's general form (csrc/swd_huge_bp4.hip) on the two EG codes only it takes.

Workloads: [[273,111,17]] at depolarizing p = 0.06 and [[1057,571,33]] at p = 0.04 (tests/golden/bp4_general.npz holds the matrices),
uniform priors, Misc.ipynb cell 8's parameters (max_iter=50, ms_scaling_factor=0.8, osd_order=-1), --shots syndromes each, ``decode``
and ``camel_decode`` on device-resident arrays.  For context the cycle-assembled [[170]] and [[362]] codes of bp4_heavy.npz at p = 0.04 /
0.02 in both forms -- the HEAVY form of the tuned kernel and general_form=True -- in the same run.
Timing: HIP events around one launch on syndromes already on the device, after a warm-up launch of the same shape; the median of
--repeats launches.  Beside each general-form figure the CPU oracle's rate on syndromes of the same distribution in a pool of 16
processes on the same machine (the yardstick of scripts/huge_gdg_rate.py); the pool runs before this process opens the device.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KW = {"decode": dict(max_iter=50, ms_scaling_factor=0.8, osd_method="osd_cs", osd_order=-1),
      "camel_decode": dict(max_iter=50, ms_scaling_factor=0.8, osd_method="osd0", osd_order=-1)}
# code: fixture, tag, p, forms, oracle shots per process
CODES = {"eg273": ("bp4_general.npz", "eg273", 0.06, (True,), 16), "eg1057": ("bp4_general.npz", "eg1057", 0.04, (True,), 1),
         "camel170": ("bp4_heavy.npz", "camel170", 0.04, (False, True), 0), "camel362": ("bp4_heavy.npz", "camel362", 0.02, (False, True), 0)}


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
    dec = O.bp4_osd(Hx, Hz, **pr, **KW[method])
    t0 = time.perf_counter()
    conv = 0
    for k in range(shots):
        getattr(dec, method)(sx[k], sz[k])
        conv += int(dec.converge)
    return time.perf_counter() - t0, conv


def oracle_rate(code, method, procs, shots):
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(procs) as pool:  # fresh processes: none of them has the device open
        got = pool.map(_oracle_worker, [(code, method, 100 + i, shots) for i in range(procs)], chunksize=1)
    # (the workers' own decode time: the pool's start-up and the syndrome sampling are not the decoder's)
    return {"processes": procs, "shots_per_process": shots, "decodes_per_s": procs * shots / max(t for t, _ in got),
            "converged": sum(c for _, c in got)}


def device_rate(code, method, general, shots, repeats):
    import torch
    from slidingwindowdecoder_amd import _lib, bp4_osd
    dev = torch.device("cuda", 0)
    Hx, Hz, pr, p = load_code(code)
    dec = bp4_osd(Hx, Hz, **pr, **KW[method], general_form=general)
    sx, sz = (torch.from_numpy(a).to(dev) for a in syndromes(Hx, Hz, p, shots, 7))
    out = torch.empty((shots, 2, dec.n), dtype=torch.uint8, device=dev)
    st = torch.empty((shots, _lib.STAT_WORDS), dtype=torch.int32, device=dev)
    cur = torch.cuda.current_stream(dev)

    def launch():
        if method == "decode":
            dec.decode_batch_device(sx, sz, out=out, stats=st)
        elif _lib.lib().swd_bp4_camel_decode_batch_dev(dec._h, shots, sx.data_ptr(), sz.data_ptr(), out.data_ptr(), st.data_ptr(), None,
                                                      cur.cuda_stream):
            raise RuntimeError(_lib.last_error())
    launch()  # warm-up: code objects, the launch slot's scratch area
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        launch()
        e1.record(cur)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    stats = st.cpu().numpy()
    mid = sorted(ms)[len(ms) // 2]
    return {"general_form": bool(dec.general_form), "form": dec.last_form, "shots": shots, "ms_all": ms, "decodes_per_s": shots / (mid * 1e-3),
            "converged": int(((stats[:, 0] & 0x100) != 0).sum()), "mean_iterations": float(stats[:, 1].mean()),
            "checksum": int(out.to(torch.int64).sum().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--oracle-procs", type=int, default=16)
    ap.add_argument("--codes", default=",".join(CODES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bp4_general_rate.json"))
    args = ap.parse_args()
    codes = [c for c in args.codes.split(",") if c]
    res = {"shots": args.shots, "repeats": args.repeats, "parameters": "max_iter=50, ms_scaling_factor=0.8, osd_order=-1", "codes": {}}
    for code in codes:  # every child process before this one opens the device
        res["codes"][code] = {"p": CODES[code][2], "oracle_16_processes": {}, "device": {}}
        for method in KW:
            if CODES[code][4]:
                res["codes"][code]["oracle_16_processes"][method] = oracle_rate(code, method, args.oracle_procs, CODES[code][4])
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    res["device"] = torch.cuda.get_device_name(0)
    for code in codes:
        r = res["codes"][code]
        for method in KW:
            for general in CODES[code][3]:
                key = method + ("/general" if general else "/tuned")
                r["device"][key] = device_rate(code, method, general, args.shots, args.repeats)
                o = r["oracle_16_processes"].get(method)
                if general and o:
                    r["device"][key]["over_oracle_16_processes"] = r["device"][key]["decodes_per_s"] / o["decodes_per_s"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
