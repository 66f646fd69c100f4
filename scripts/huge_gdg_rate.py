#!/usr/bin/env python3
"""Decodes/s of the guessing decoders' general form (csrc/swd_huge_gdg.hip) on the un-windowed [[288,12,18]] detector error model of
an 18-round memory experiment (2736 x 26 208, new_n 5472): bpgdg_decoder(multi_thread=True) with the parameters of the reference's
guessing.py, against the oracle on 64 of the shots in a pool of 16 processes (timed, and checked bit for bit).
python scripts/huge_gdg_rate.py [shots] [p]"""
import json, os, sys, time
import multiprocessing as mp
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench

KW = dict(max_iter=8, max_iter_per_step=6, max_step=25, max_tree_depth=3, max_side_depth=10, max_tree_branch_step=10,
          max_side_branch_step=10, low_error_mode=False, gdg_factor=1.0, ms_scaling_factor=1.0, multi_thread=True)
_ora = _bar = None


def _oracle_init(mat, prior, bar):
    global _ora, _bar
    from oracle import oracle as O
    _ora, _bar = O.bpgdg_decoder(mat, channel_probs=prior, **KW), bar


def _ready(_):
    _bar.wait()  # one warm-up task per process: timing starts once every process has built its object


def _oracle_decode(s):
    _ora.clear_history()
    out = _ora.decode(s)
    return out.astype(np.uint8), float(_ora.min_pm), bool(_ora.converge)


def main():
    shots = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    p = float(sys.argv[2]) if len(sys.argv) > 2 else 0.004
    from slidingwindowdecoder_amd import bpgdg_decoder
    from slidingwindowdecoder_amd.windows import sample_dem
    plan = bench.build_problem(N=288, p=p, rounds=18, W=19, F=1)
    w = plan.windows[0]
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, shots, seed=3)
    synd = np.ascontiguousarray(det[:, w.row0:w.row1])
    dec = bpgdg_decoder(w.mat, channel_probs=w.prior, **KW)
    dec.decode_batch(synd[:8])
    t0 = time.perf_counter()
    out = dec.decode_batch(synd)
    el = time.perf_counter() - t0
    st, pm = dec.last_stats.copy(), dec.last_min_pm.copy()
    k = min(64, shots)
    ctx = mp.get_context("spawn")  # fresh processes: none of them inherits this process's GPU context
    with ctx.Pool(16, initializer=_oracle_init, initargs=(w.mat, w.prior, ctx.Barrier(16))) as pool:
        pool.map(_ready, range(16), chunksize=1)
        t0 = time.perf_counter()
        res = pool.map(_oracle_decode, list(synd[:k]), chunksize=1)
        el_o = time.perf_counter() - t0
    bad = [i for i, (o, opm, cv) in enumerate(res)
           if not (np.array_equal(out[i], o) and bool(st[i, 0] & 0x100) == cv and ((st[i, 0] & 0xFF) != 1 or pm[i] == opm))]
    cls = np.bincount(st[:, 0] & 0xFF, minlength=6)
    post = (st[:, 0] & 0xFF) == 1
    gpu_rate, ora_rate = shots / el, k / el_o
    print(json.dumps({"workload": f"bpgdg_decoder(multi_thread=True, guessing.py parameters) on the un-windowed [[288,12,18]] DEM, "
                                  f"p = {p}, 18 rounds", "shape": list(w.mat.shape), "edges": int(w.mat.nnz), "new_n": int(min(w.mat.shape[1], 2 * w.mat.shape[0])),
                      "shots": shots, "seconds": round(el, 3), "decodes_per_s": round(gpu_rate, 1),
                      "oracle_shots": k, "oracle_processes": 16, "oracle_seconds": round(el_o, 3), "oracle_decodes_per_s": round(ora_rate, 1),
                      "speedup_vs_oracle_pool": round(gpu_rate / ora_rate, 2), "oracle_mismatches": len(bad),
                      "exit_classes_pre_post_x_x_failpeel_noosd": cls[:6].tolist(),
                      "mean_hypotheses_post": float(st[post, 4].mean()) if post.any() else 0.0,
                      "mean_bp_blocks_post": float(st[post, 5].mean()) if post.any() else 0.0}))
    return 0 if not bad else 1


if __name__ == "__main__":
    sys.exit(main())
