#!/usr/bin/env python3
"""Generate tests/golden/bp4_general.npz from the REFERENCE ITSELF: bp4_osd on the two Euclidean-geometry codes of Misc.ipynb
cell 8 that only the general form of the device decoder takes (bp4_osd(..., general_form=True)):

  eg273    create_EG_codes(4), [[273,111,17]]: H 256 x 273, every column of weight 16 (above the bound of the tuned kernels), the last
           one of weight 256, rows of weight 18; p = 0.06, 40 shots
  eg1057   create_EG_codes(5), [[1057,571,33]]: H 1024 x 1057, columns of weight 32, the last one 1024, rows of weight 34 -- 544 KB of
           messages; p = 0.04, 4 shots (a shot costs seconds in the oracle that replays it); Hz equals Hx and is stored once

The recipe of make_golden_heavy.py (its ensure_reference, pack and h64 are imported, not copied): the reference's compiled extension
and its code constructor are what is recorded, no reference source is copied, and everything in the fixture is data those programs
produced or were fed.  Same fields per case as bp4_heavy.npz (see make_golden_heavy.py), with ``heavy`` = the last qubit.  Priors are
uniform, p / 3 each, and the errors are the reference's own sampling (Misc.ipynb cell 8: one uniform draw per qubit against the
priors), with no scaled shots.  A NEW reference object per shot, so every shot is comparable with a device shot.

The generator asserts at least 5 converged and 5 unconverged shots per method on eg273, and at least one of each in ``decode`` on
eg1057 (seed 105701 leaves all four unconverged, 105702 meets it).  Seeds are fixed below; SWD_GENERAL_SEARCH=1 walks on from them until the assertions hold and prints the seed to write down.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_heavy import CAMEL_KW, DECODE_KW, ensure_reference, h64, pack  # noqa: E402

# tag, s of create_EG_codes(s), p, shots, seed, posteriors kept in full, least count of each BP exit (camel, decode)
CASES = [("eg273", 4, 0.06, 40, 27301, 4, (5, 5)),
         ("eg1057", 5, 0.04, 4, 105702, 1, (0, 1))]


def record_case(ref, tag, Hx, Hz, p, shots, seed, lpr_full, least):
    Hx, Hz = np.asarray(Hx).astype(np.uint8), np.asarray(Hz).astype(np.uint8)
    n = Hx.shape[1]
    rng = np.random.default_rng(seed)
    px = py = pz = np.full(n, p / 3)
    heavy = np.array([n - 1], np.int32)
    # With "osd0" the reference resets osd_order to 0 and its constructor prepares OSD-0, which takes more than five minutes per object
    # at 1057 qubits -- and a new object is built per shot.  camel_decode never looks at the OSD settings, so on eg1057 the reference
    # object of the camel run is built with osd_method="osd_cs" (order -1 kept); camel_params in the fixture stay cell 8's.
    camel_ref_kw = CAMEL_KW if tag != "eg1057" else dict(CAMEL_KW, osd_method="osd_cs")

    def new(kw):
        return ref.bp4_osd(Hx.astype(int), Hz.astype(int), channel_probs_x=px, channel_probs_y=py, channel_probs_z=pz, **kw)
    sxs, szs = [], []
    c_out, c_conv, c_it, c_pm = [], [], [], []
    d_out, d_conv, d_it, d_hash, d_lpr, d_hv = [], [], [], [], [], []
    for k in range(shots):
        noise = rng.uniform(0, 1, n)
        err_z = np.logical_and(noise > px, noise < px + py + pz)
        err_x = noise < px + py
        sx, sz = (err_z @ Hx.T) % 2, (err_x @ Hz.T) % 2
        sxs.append(sx); szs.append(sz)
        dec = new(camel_ref_kw)
        out = dec.camel_decode(sx, sz)
        c_out.append(np.asarray(out, np.uint8)); c_conv.append(int(dec.converge)); c_it.append(int(dec.bp_iteration))
        c_pm.append(float(dec.min_pm))
        dec = new(DECODE_KW)
        out = dec.decode(sx, sz)
        lp = np.asarray(dec.log_prob_ratios, dtype=np.float64)
        assert lp.shape == (n, 3)
        d_out.append(np.asarray(out, np.uint8)); d_conv.append(int(dec.converge)); d_it.append(int(dec.bp_iteration))
        d_hash.append(h64(lp)); d_hv.append(lp[heavy].copy())
        if k < lpr_full:
            d_lpr.append(lp.copy())
    c_conv, d_conv = np.array(c_conv, np.uint8), np.array(d_conv, np.uint8)
    counts = dict(camel_conv=int(c_conv.sum()), camel_unconv=int((c_conv == 0).sum()), decode_conv=int(d_conv.sum()),
                  decode_unconv=int((d_conv == 0).sum()))
    print(f"  bp4_general/{tag}: seed {seed} n {n} column weights {sorted(set(Hx.sum(0).tolist()))} row weights "
          f"{sorted(set(Hx.sum(1).tolist()))} {counts}")
    ok = min(counts["camel_conv"], counts["camel_unconv"]) >= least[0] and min(counts["decode_conv"], counts["decode_unconv"]) >= least[1]
    arrs = {"hx": pack(Hx), "shape": np.array([Hx.shape[0], Hz.shape[0], n], np.int32),
            "px": px, "py": py, "pz": pz, "sx": pack(np.array(sxs)), "sz": pack(np.array(szs)),
            "camel_params": json.dumps(CAMEL_KW), "decode_params": json.dumps(DECODE_KW),
            "camel_out": pack(np.array(c_out)), "camel_converge": c_conv, "camel_bp_iteration": np.array(c_it, np.int32),
            "camel_min_pm": np.array(c_pm, np.float64),
            "decode_out": pack(np.array(d_out)), "decode_converge": d_conv, "decode_bp_iteration": np.array(d_it, np.int32),
            "decode_lpr_hash": np.array(d_hash, np.uint64), "decode_lpr": np.array(d_lpr),
            "heavy": heavy, "decode_lpr_heavy": np.array(d_hv)}
    if tag != "eg1057":  # (Hz of the EG codes equals Hx: the large one stores it once)
        arrs["hz"] = pack(Hz)
    else:
        assert np.array_equal(Hx, Hz)
    return ok, {f"{tag}_{k}": v for k, v in arrs.items()}


def main():
    ensure_reference()
    import types
    import src as ref
    from src import codes_q
    # create_EG_codes ends in css_code(hx, hz, check_css=True), whose kernels and logical operators in pure Python take hours at 1057
    # qubits and are not recorded: a holder of the two matrices stands in for that class.  The matrices are the constructor's own.
    codes_q.css_code = lambda hx, hz, **kw: types.SimpleNamespace(hx=hx, hz=hz)
    create_EG_codes = codes_q.create_EG_codes
    search = bool(os.environ.get("SWD_GENERAL_SEARCH"))
    which = sys.argv[1:] or [c[0] for c in CASES]
    path = os.path.join(HERE, "bp4_general.npz")
    arrs = dict(np.load(path)) if (os.path.exists(path) and len(which) < len(CASES)) else {}
    for tag, s, p, shots, seed, lpr_full, least in CASES:
        if tag not in which:
            continue
        code = create_EG_codes(s)
        while True:
            ok, a = record_case(ref, tag, code.hx, code.hz, p, shots, seed, lpr_full, least)
            if ok or not search:
                break
            seed += 1
        assert ok, f"{tag}: seed {seed} misses the coverage the fixture promises; run with SWD_GENERAL_SEARCH=1 and write the seed down"
        arrs = {k: v for k, v in arrs.items() if not k.startswith(tag + "_")}
        arrs.update(a)
    arrs["tags"] = json.dumps([c[0] for c in CASES])
    np.savez_compressed(path, **arrs)
    print(f"wrote bp4_general.npz: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
