#!/usr/bin/env python3
"""Generate tests/golden/bp4_general_osd.npz from the REFERENCE ITSELF: bp4_osd.decode WITH OSD on the graphs the device decoder
takes with ``general_osd=True`` only -- graphs with heavy columns (the CAMEL and EG codes of Misc.ipynb cells 6-8) and the EG code
[[273,111,17]] of the general form.

The recipe of make_golden_heavy.py (its ensure_reference, pack and h64 are imported, not copied): the reference's compiled extension
is what is recorded, no reference source is copied.  The matrices, priors and syndromes are the ones bp4_heavy.npz / bp4_general.npz
already store, so this fixture holds OUTPUTS only, per case ``tag``:

  params          json of the constructor kwargs
  out             decode's return value (packed), [shots][2][n]
  osd0            osd0_decoding_x / osd0_decoding_z after the call (packed)
  converge, bp_iteration
  out_hash        blake2b-64 of the unpacked ``out`` of the case (a check on the packing)

A NEW reference object per shot, so every shot is comparable with a device shot (osd0_decoding of a shot the OSD did not reach is
BP's converged decision, as the reference leaves it).

  camel50    ("osd0", -1)   cell 8's own spelling, which the reference turns into OSD-0 (bp4_osd.pyx:74-76)
  eg73       osd_cs 10
  camel170   osd_e 5
  two_heavy  osd_cs 6       rank 24 against 20: the unequal-rank sweep (kz = n - rank_x)
  camel362   osd_cs 10
  eg273      osd_cs 10      (bp4_general.npz)

EG [[1057,571,33]] is not recorded: the reference's constructor alone takes minutes per object there (make_golden_general.py).
The generator asserts at least 5 shots per case that reach the OSD and at least 5 that converge.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_heavy import ensure_reference, h64, pack  # noqa: E402

BASE = dict(max_iter=50, ms_scaling_factor=0.8)
# tag, source fixture, constructor kwargs
CASES = [("camel50", "bp4_heavy.npz", dict(BASE, osd_method="osd0", osd_order=-1)),
         ("eg73", "bp4_heavy.npz", dict(BASE, osd_method="osd_cs", osd_order=10)),
         ("camel170", "bp4_heavy.npz", dict(BASE, osd_method="osd_e", osd_order=5)),
         ("two_heavy", "bp4_heavy.npz", dict(BASE, osd_method="osd_cs", osd_order=6)),
         ("camel362", "bp4_heavy.npz", dict(BASE, osd_method="osd_cs", osd_order=10)),
         ("eg273", "bp4_general.npz", dict(BASE, osd_method="osd_cs", osd_order=10))]


def unpack(a, n):
    return np.unpackbits(a, axis=-1)[..., :n]


def record_case(ref, tag, src, kw):
    f = np.load(os.path.join(HERE, src))
    mx, mz, n = (int(x) for x in f[f"{tag}_shape"])
    Hx, Hz = unpack(f[f"{tag}_hx"], n), unpack(f[f"{tag}_hz"], n)
    px, py, pz = f[f"{tag}_px"], f[f"{tag}_py"], f[f"{tag}_pz"]
    sx, sz = unpack(f[f"{tag}_sx"], mx), unpack(f[f"{tag}_sz"], mz)
    outs, o0, conv, its = [], [], [], []
    for k in range(len(sx)):
        dec = ref.bp4_osd(Hx.astype(int), Hz.astype(int), channel_probs_x=px, channel_probs_y=py, channel_probs_z=pz, **kw)
        out = dec.decode(sx[k].astype(int), sz[k].astype(int))
        outs.append(np.asarray(out, np.uint8))
        o0.append(np.stack([dec.osd0_decoding_x, dec.osd0_decoding_z]).astype(np.uint8))
        conv.append(int(dec.converge)); its.append(int(dec.bp_iteration))
    outs, conv = np.array(outs), np.array(conv, np.uint8)
    # BP does not depend on the OSD settings: the exits are those of the BP-only recording
    assert np.array_equal(conv, f[f"{tag}_decode_converge"]) and np.array_equal(its, f[f"{tag}_decode_bp_iteration"])
    osd = conv == 0
    for k in np.flatnonzero(osd):  # every correction the OSD returns satisfies both syndromes
        assert np.array_equal((Hx.astype(np.int64) @ outs[k, 1]) % 2, sx[k]) and np.array_equal((Hz.astype(np.int64) @ outs[k, 0]) % 2, sz[k])
    print(f"  bp4_general_osd/{tag}: {kw['osd_method']} {kw['osd_order']}: {int(osd.sum())} of {len(sx)} shots reach the OSD")
    assert osd.sum() >= 5 and (~osd).sum() >= 5
    arrs = {"params": json.dumps(kw), "out": pack(outs), "osd0": pack(np.array(o0)), "converge": conv,
            "bp_iteration": np.array(its, np.int32), "out_hash": h64(outs)}
    return {f"{tag}_{k}": v for k, v in arrs.items()}


def main():
    ensure_reference()
    import src as ref
    which = sys.argv[1:] or [c[0] for c in CASES]
    path = os.path.join(HERE, "bp4_general_osd.npz")
    arrs = dict(np.load(path)) if (os.path.exists(path) and len(which) < len(CASES)) else {}
    for tag, src, kw in CASES:
        if tag not in which:
            continue
        arrs = {k: v for k, v in arrs.items() if not k.startswith(tag + "_")}
        arrs.update(record_case(ref, tag, src, kw))
    arrs["tags"] = json.dumps([c[0] for c in CASES])
    np.savez_compressed(path, **arrs)
    print(f"wrote bp4_general_osd.npz: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
