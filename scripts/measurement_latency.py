#!/usr/bin/env python3
"""Latency of the measurement sessions (SlidingWindowDecoder.measurement_session): the headline plan of scripts/session_latency.py --
[[144,12,12]], p = 0.003, 12 rounds, (W,F) = (3,1), OSD-CS 10 -- fed one round per push.  For the same shots, HIP-event time of every
push that completes a window, median and p99 over 20 batches after warm-up, for B = 1, 64, 4096:
  (a) session.push_device(det_rows)              detector rows, as scripts/session_latency.py measures them
  (b) measurement_session.push_device(meas)      the round's 144 raw measurement bits: front-end launch, then (a)
  (c) two back-to-back launches of an empty kernel on the same stream (swd_diag_occupy with a zero duration)
  (d) the front end alone through the C ABI: one swd_frontend_push_dev call into a buffer allocated beforehand
  (e) the front end alone through MeasurementFrontEnd.push_device (argument checks, row count and output view in Python, then (d))
Every span starts on an idle stream (the round before has been waited for), so it holds the host's time to issue the work as well as
the device's to do it; (d) and (e) split (b) - (a) into the launch and the Python layer around it.
The front end is one launch in front of the session's merge, so (b) - (a) should stay within (c).  The records are synthesised on the
host from the sampled detectors (measurements.synthesize_measurements_host).  Writes profiles/measurement_latency.json (or the path
given as the first argument)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402
from slidingwindowdecoder_amd import DemSampler, MeasurementFrontEnd, SlidingWindowDecoder, _lib  # noqa: E402
from slidingwindowdecoder_amd.circuit import bb_memory_ops  # noqa: E402
from slidingwindowdecoder_amd.codes import bb_code  # noqa: E402
from slidingwindowdecoder_amd.measurements import measurement_map, synthesize_measurements_host  # noqa: E402

BATCHES, WARMUP = 20, 3
plan = bench.build_problem()
kw = dict(bench.DECODER_KW, osd_order=10)
dec = SlidingWindowDecoder(plan, **kw)
sampler = DemSampler(plan.chk, plan.obs, plan.priors)
code, A, Bm = bb_code(144)
mmap = measurement_map(bb_memory_ops(code, A, Bm, 0.003, 12), plan.n_half)
blk = mmap.blocks()
h, mpr, rounds = plan.n_half, blk.meas_per_round, blk.rounds
stream = torch.cuda.Stream()
L = _lib.lib()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    stream.synchronize()  # the next round arrives after this one has been handled
    return e0.elapsed_time(e1), r


def two_empty_launches():
    for _ in range(2):
        if L.swd_diag_occupy(dec.device, 1, 64, 0, 0, stream.cuda_stream):
            raise RuntimeError(_lib.last_error())


def stats(ms):
    return {"median_ms": float(np.median(ms)), "p99_ms": float(np.percentile(ms, 99)), "samples": len(ms)}


out = {"plan": "[[144,12,12]] p=0.003, 12 rounds, (3,1), osd_cs 10", "windows": dec.W, "rows_per_push": h, "bits_per_push": mpr,
       "batches": BATCHES, "sizes": {}}
for B in (1, 64, 4096):
    ses, mses = dec.session(B), dec.measurement_session(B, mmap)
    fe_c, fe_py = MeasurementFrontEnd(mmap, h, B), MeasurementFrontEnd(mmap, h, B)
    rows_c = torch.empty((B, h), dtype=torch.uint8, device="cuda")
    a_ms, b_ms, c_ms, d_ms, e_ms = [], [], [], [], []
    for k in range(WARMUP + BATCHES):
        det, flips = sampler.sample_device(B, seed=1000 + k)
        torch.cuda.synchronize()
        obs = (flips.cpu().numpy().astype(np.uint32)[:, None] >> np.arange(mmap.obs.shape[0], dtype=np.uint32)) & 1
        meas_host = synthesize_measurements_host(mmap, det.cpu().numpy(), obs, np.random.default_rng(k))
        meas = torch.from_numpy(meas_host).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            ses.begin(B)
            mses.begin(B)
            fe_c.begin(B)
            fe_py.begin(B)
            for r in range(rounds):
                ta, (_, ca) = timed(lambda: ses.push_device(det[:, r * h:(r + 1) * h], stream=stream))
                tb, (_, cb) = timed(lambda: mses.push_device(meas[:, r * mpr:(r + 1) * mpr], stream=stream))
                tc, _ = timed(two_empty_launches)
                bits = meas[:, r * mpr:(r + 1) * mpr]
                td, rc = timed(lambda: L.swd_frontend_push_dev(fe_c._h, mpr, bits.data_ptr(), bits.stride(0), 0, rows_c.data_ptr(), 0, None,
                                                              stream.cuda_stream))
                te, rows_py = timed(lambda: fe_py.push_device(bits, stream=stream))
                assert ca == cb and rc == 0 and torch.equal(rows_c, rows_py) and torch.equal(rows_py, det[:, r * h:(r + 1) * h])
                if k >= WARMUP and ca:
                    for acc, t in zip((a_ms, b_ms, c_ms, d_ms, e_ms), (ta, tb, tc, td, te)):
                        acc.append(t)
            ses.push_device(det[:, rounds * h:], stream=stream)
            stream.synchronize()
            fin = mses.finish(meas_host[:, rounds * mpr:])
        want = ses.finish()
        assert all(np.array_equal(x, y) for x, y in zip(fin[:5], want)), "the measurement session differs from the session"
    for x in (ses, mses, fe_c, fe_py):
        x.close()
    rec = {"a_push_det_rows": stats(a_ms), "b_push_measurements": stats(b_ms), "c_two_empty_launches": stats(c_ms),
           "d_front_end_c_abi": stats(d_ms), "e_front_end_python": stats(e_ms)}
    rec["b_minus_a_median_ms"] = rec["b_push_measurements"]["median_ms"] - rec["a_push_det_rows"]["median_ms"]
    rec["b_minus_a_paired_median_ms"] = float(np.median(np.array(b_ms) - np.array(a_ms)))
    out["sizes"][str(B)] = rec
    print(f"B = {B}: (a) {rec['a_push_det_rows']['median_ms']:.4f} / p99 {rec['a_push_det_rows']['p99_ms']:.4f} ms, (b) "
          f"{rec['b_push_measurements']['median_ms']:.4f} / p99 {rec['b_push_measurements']['p99_ms']:.4f} ms, (c) "
          f"{rec['c_two_empty_launches']['median_ms']:.4f} / p99 {rec['c_two_empty_launches']['p99_ms']:.4f} ms; (b) - (a) = "
          f"{rec['b_minus_a_median_ms']:.4f} ms (paired median {rec['b_minus_a_paired_median_ms']:.4f}); front end alone: (d) C ABI "
          f"{rec['d_front_end_c_abi']['median_ms']:.4f}, (e) Python {rec['e_front_end_python']['median_ms']:.4f} ms", flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "measurement_latency.json")
json.dump(out, open(path, "w"), indent=1)
print("wrote", path)
