#!/usr/bin/env python3
"""Generate tests/golden/bp4_heavy.npz from the REFERENCE ITSELF: bp4_osd on codes with heavy columns, the cycle-assembled
(CAMEL) and Euclidean-geometry codes of Misc.ipynb cells 6-8, H = (H1 | 1), whose last qubit touches every check, plus random
matrices with two heavy columns that are not the last one.

Same recipe as make_golden.py for making the reference importable (ensure_reference() below is that recipe); the reference's
compiled extension and its code constructors are what is recorded -- no reference source is copied.  Everything in the fixture is
data those programs produced or were fed: Hx, Hz (packed bits), priors, packed syndromes, outputs.

Per case ``tag``:
  hx, hz (packed rows), shape = (mx, mz, n), px, py, pz, sx, sz (packed)
  camel_params / decode_params   json of the constructor kwargs
  camel_out, camel_converge, camel_bp_iteration, camel_min_pm
  decode_out, decode_converge, decode_bp_iteration
  decode_lpr_hash    blake2b-64 of the raw bytes of log_prob_ratios (n x 3 doubles) of EVERY shot: equal hashes are equal posteriors
  decode_lpr         the full n x 3 posteriors of the first LPR_FULL shots
  heavy, decode_lpr_heavy   the heavy columns and their posteriors on every shot (the check on the summation order)

A NEW reference object per shot, so a camel_decode shot with no converged run records the zero vectors and min_pm = 10000.0 of
a new object -- what a device shot returns -- and every shot is comparable.

camel_params are Misc.ipynb cell 8's: max_iter=50, ms_scaling_factor=0.8, osd_method="osd0", osd_order=-1.  With "osd0" the
reference resets osd_order to 0 (bp4_osd.pyx:74-76), which camel_decode never looks at; ``decode`` is recorded with
osd_method="osd_cs", osd_order=-1, the spelling under which the reference keeps -1 and returns the BP decisions of a shot that
did not converge (bp4_osd.pyx:213-221).

Shots 0, 4, 8, .. draw their error at SCALE[0] times the priors and shots 2, 6, 10, .. at SCALE[1] times (inputs only; the decoder's
priors stay): both exits of BP are then present at the notebook's noise rates, and the 40 shots of the largest code hold enough
errors on its last qubit.  The issue's plain sampling alone does not reach the coverage asserted below on every case (camel_decode
on EG [[73]] at p = 0.04 leaves 0-3 of 200 shots unconverged under any seed tried), hence the scaled shots; the assertions are the
issue's, unrelaxed.  A scaled probability is simply compared with the uniform draw, so where SCALE * (px + py) of the last qubit
exceeds 1 (SCALE[0] = 8 with its raised priors 0.10 / 0.06 / 0.08) that qubit is never I or Z in those shots: always X or Y.
Seeds are fixed below; SWD_HEAVY_SEARCH=1 walks on from them until the assertions hold
(at least 5 converged and 5 unconverged shots in both methods, at least 3 camel winners of each of X, Z, Y on the last qubit)
and prints the seed to write down here.
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFBUILD = os.environ.get("SWD_REFBUILD", "/tmp/refbuild")
sys.path.insert(0, ROOT)

LPR_FULL = 12
SWD_DMAX = 10
LAST_PRIORS = (0.10, 0.06, 0.08)
CAMEL_KW = dict(max_iter=50, ms_scaling_factor=0.8, osd_method="osd0", osd_order=-1)
DECODE_KW = dict(max_iter=50, ms_scaling_factor=0.8, osd_method="osd_cs", osd_order=-1)


def ensure_reference():
    if not os.path.exists(os.path.join(REFBUILD, "src")) or not any(
            f.startswith("osd_window.") and f.endswith(".so") for f in os.listdir(os.path.join(REFBUILD, "src"))):
        sh = f"""
        set -e
        rm -rf {REFBUILD} && cp -r /root/reference {REFBUILD} && chmod -R u+w {REFBUILD} && cd {REFBUILD}
        sed -i 's/np\\.int_t/np.int64_t/g' src/*.pyx src/*.pxd
        sed -i 's/= long(/= int(/g' src/bp4_osd.pyx src/osd_window.pyx
        rm -f src/bp4_osd.cpp src/osd_window.cpp src/bp_guessing_decoder.cpp src/mod2sparse.c
        python3 setup.py build_ext --inplace > build.log 2>&1
        """
        subprocess.check_call(["bash", "-c", sh])
    sys.path.insert(0, REFBUILD)


def h64(a):
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=8).digest(), dtype=np.uint64)[0]


def pack(a):
    return np.packbits(np.asarray(a, dtype=np.uint8), axis=-1)


def two_heavy_matrices(seed):
    """24 x 60 and 20 x 60, every column of weight 3 except columns 0 and 31: weights 13 and 20 in Hx, 11 and 20 in Hz."""
    rng = np.random.default_rng(seed)
    n = 60

    def rand_h(m, w0, w31):
        H = np.zeros((m, n), np.uint8)
        for c in range(n):
            H[rng.choice(m, size={0: w0, 31: w31}.get(c, 3), replace=False), c] = 1
        return H
    return rand_h(24, 13, 20), rand_h(20, 11, 20)


def record_case(ref, tag, Hx, Hz, p, shots, seed, scale):
    Hx, Hz = np.asarray(Hx).astype(np.uint8), np.asarray(Hz).astype(np.uint8)
    n = Hx.shape[1]
    rng = np.random.default_rng(seed)
    px, py, pz = (p / 3 * rng.uniform(0.5, 1.5, n) for _ in range(3))
    px[-1], py[-1], pz[-1] = LAST_PRIORS
    wx, wz = Hx.sum(0), Hz.sum(0)
    heavy = np.flatnonzero((wx > SWD_DMAX) | (wz > SWD_DMAX)).astype(np.int32)

    def new(kw):
        return ref.bp4_osd(Hx.astype(int), Hz.astype(int), channel_probs_x=px, channel_probs_y=py, channel_probs_z=pz, **kw)
    sxs, szs = [], []
    c_out, c_conv, c_it, c_pm = [], [], [], []
    d_out, d_conv, d_it, d_hash, d_lpr, d_hv = [], [], [], [], [], []
    for k in range(shots):
        sc = scale[0] if k % 4 == 0 else (scale[1] if k % 4 == 2 else 1.0)
        noise = rng.uniform(0, 1, n)
        err_z = np.logical_and(noise > sc * px, noise < sc * (px + py + pz))
        err_x = noise < sc * (px + py)
        sx, sz = (err_z @ Hx.T) % 2, (err_x @ Hz.T) % 2
        sxs.append(sx); szs.append(sz)
        dec = new(CAMEL_KW)
        out = dec.camel_decode(sx, sz)
        c_out.append(np.asarray(out, np.uint8)); c_conv.append(int(dec.converge)); c_it.append(int(dec.bp_iteration))
        c_pm.append(float(dec.min_pm))
        dec = new(DECODE_KW)
        out = dec.decode(sx, sz)
        lp = np.asarray(dec.log_prob_ratios, dtype=np.float64)
        assert lp.shape == (n, 3)
        d_out.append(np.asarray(out, np.uint8)); d_conv.append(int(dec.converge)); d_it.append(int(dec.bp_iteration))
        d_hash.append(h64(lp)); d_hv.append(lp[heavy].copy())
        if k < LPR_FULL:
            d_lpr.append(lp.copy())
    c_conv, d_conv, c_out = np.array(c_conv, np.uint8), np.array(d_conv, np.uint8), np.array(c_out)
    win = (c_out[:, 0, -1] + 2 * c_out[:, 1, -1])[c_conv == 1]
    counts = dict(camel_conv=int(c_conv.sum()), camel_unconv=int((c_conv == 0).sum()), decode_conv=int(d_conv.sum()),
                  decode_unconv=int((d_conv == 0).sum()), win_x=int((win == 1).sum()), win_z=int((win == 2).sum()),
                  win_y=int((win == 3).sum()))
    print(f"  bp4_heavy/{tag}: seed {seed} n {n} heavy {heavy.tolist()} weights {wx[heavy].tolist()} / {wz[heavy].tolist()} {counts}")
    ok = min(counts["camel_conv"], counts["camel_unconv"], counts["decode_conv"], counts["decode_unconv"]) >= 5 and \
        min(counts["win_x"], counts["win_z"], counts["win_y"]) >= 3
    arrs = {"hx": pack(Hx), "hz": pack(Hz), "shape": np.array([Hx.shape[0], Hz.shape[0], n], np.int32),
            "px": px, "py": py, "pz": pz, "sx": pack(np.array(sxs)), "sz": pack(np.array(szs)),
            "camel_params": json.dumps(CAMEL_KW), "decode_params": json.dumps(DECODE_KW),
            "camel_out": pack(c_out), "camel_converge": c_conv, "camel_bp_iteration": np.array(c_it, np.int32),
            "camel_min_pm": np.array(c_pm, np.float64),
            "decode_out": pack(np.array(d_out)), "decode_converge": d_conv, "decode_bp_iteration": np.array(d_it, np.int32),
            "decode_lpr_hash": np.array(d_hash, np.uint64), "decode_lpr": np.array(d_lpr),
            "heavy": heavy, "decode_lpr_heavy": np.array(d_hv)}
    return ok, {f"{tag}_{k}": v for k, v in arrs.items()}


def main():
    ensure_reference()
    import src as ref
    from src.codes_q import create_cycle_assemble_codes, create_EG_codes
    search = bool(os.environ.get("SWD_HEAVY_SEARCH"))
    # tag, (Hx, Hz), p, shots, seed, SCALE
    cases = [("camel50", lambda: create_cycle_assemble_codes(7, 3), 0.03, 300, 5001, (3.0, 1.0)),
             ("eg73", lambda: create_EG_codes(3), 0.04, 200, 7306, (8.0, 1.0)),
             ("camel170", lambda: create_cycle_assemble_codes(13, 2), 0.04, 120, 17001, (4.0, 1.0)),
             ("two_heavy", lambda: two_heavy_matrices(6031), 0.03, 200, 6001, (3.0, 1.0)),
             ("camel362", lambda: create_cycle_assemble_codes(19, 3), 0.02, 40, 36402, (8.0, 2.4))]
    which = sys.argv[1:] or [c[0] for c in cases]
    path = os.path.join(HERE, "bp4_heavy.npz")
    arrs = dict(np.load(path)) if (os.path.exists(path) and len(which) < len(cases)) else {}
    for tag, make, p, shots, seed, scale in cases:
        if tag not in which:
            continue
        code = make()
        Hx, Hz = (code.hx, code.hz) if hasattr(code, "hx") else code
        while True:
            ok, a = record_case(ref, tag, Hx, Hz, p, shots, seed, scale)
            if ok or not search:
                break
            seed += 1
        assert ok, f"{tag}: seed {seed} misses the coverage the fixture promises; run with SWD_HEAVY_SEARCH=1 and write the seed down"
        arrs = {k: v for k, v in arrs.items() if not k.startswith(tag + "_")}
        arrs.update(a)
    arrs["tags"] = json.dumps([c[0] for c in cases])
    np.savez_compressed(path, **arrs)
    print(f"wrote bp4_heavy.npz: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
