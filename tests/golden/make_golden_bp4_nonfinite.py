#!/usr/bin/env python3
"""Generate tests/golden/bp4_nonfinite.npz from the REFERENCE ITSELF: bp4_osd.decode where the posteriors are not finite.

A qubit under several degree-1 checks collects their +-1e308 sentinels (the minimum over "the other edges" of a check with one
edge): two of one sign sum to +-inf, two of opposite signs leave the rest, and inf - inf is NaN.  The construction: random Hx and
Hz (rand_h of tests/fuzz_bp4.py at density 2.2 / m), and appended to BOTH, for chosen qubits q, k rows that are the single entry q
("twins").  Errors are drawn at twice the priors; on odd shots the syndrome bits of the appended rows are replaced by random bits,
so that twins disagree (no error explains such a syndrome: BP cannot converge, and the sentinels of disagreeing twins cancel or
add up).  Priors uniform in [0.005, 0.03] per component, ms_scaling_factor 0.625.

Same recipe as make_golden_heavy.py for making the reference importable (its ensure_reference, pack and h64 are imported, not
copied): the reference's compiled extension is what is recorded, no reference source is copied.  A NEW reference object per shot.

Matrix groups and the runs recorded on each (tag = group + "_" + run):
  n24   n = 24, m = 8, twins (0, 2), (5, 3)                       osd0: max_iter 3, osd_0;  cs3: max_iter 12, osd_cs order 3
  n70   n = 70, m = 20, twins (0, 2), (33, 2), (69, 4)            osd0, cs3 as above;
                                                                  general: max_iter 12, (osd_cs, -1), device general_form=True;
                                                                  gosd: cs3 with device general_osd=True
  h71   n70's construction plus a qubit that touches every one    heavy: max_iter 12, (osd_cs, -1) -- the HEAVY instantiation;
        of the 20 random checks of Hx and of Hz (weight 20 > 10)  hgosd: cs3 with device general_osd=True
(osd_cs with order -1 is the spelling under which the reference keeps -1 and returns the BP decisions of an unconverged shot.)

Per tag:
  hx, hz (packed rows), shape = (mx, mz, n), px, py, pz, sx, sz (packed)
  params          json of the reference's constructor kwargs;  device_params  json of the device decoder's extra kwargs
  out             decode's return value (packed) [shots][2][n];  converge, bp_iteration
  bp_dec          bp_decoding_x / bp_decoding_z after the call (packed);  osd0  osd0_decoding_x / _z (packed)
  lpr             the full n x 3 posteriors (log_prob_ratios) of the first LPR_FULL shots
  lpr_hash        blake2b-64 of every shot's posteriors after every NaN has been set to the one pattern of numpy.nan
  key_nan         1 where an OSD ordering key of the shot (either basis) is NaN: std::stable_sort then leaves the reference's vector
                  and OSD-0 vectors undefined, and nothing compares them
  nan_lpr         1 where the shot's posteriors hold a NaN

Conditions, asserted here and again by tests/test_oracle_bp4_nonfinite.py: every tag has at least 24 shots that are not converged,
have non-finite posteriors and NaN-free keys in both bases (keys by _log1pexp / _logaddexp of tests/test_oracle_bp4.py), and at
least 3 shots with NaN posteriors.  The seeds in GROUPS are the first from 9001 / 9101 / 9201 on at which every run of the group
holds them (9001, 9102, 9205: 25-29 such shots and 3-4 NaN shots of 48); SWD_NONFINITE_SEARCH=1 walks on from them and prints the
seed to write down here.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden_heavy import ensure_reference, h64, pack  # noqa: E402

SHOTS = 48
LPR_FULL = 16
BASE = dict(ms_scaling_factor=0.625)
OSD0 = dict(BASE, max_iter=3, osd_method="osd_0", osd_order=0)
CS3 = dict(BASE, max_iter=12, osd_method="osd_cs", osd_order=3)
BP_ONLY = dict(BASE, max_iter=12, osd_method="osd_cs", osd_order=-1)
# group: n, m, twins, heavy column, seed, runs (name, reference kwargs, device kwargs)
GROUPS = {
    "n24": (24, 8, ((0, 2), (5, 3)), False, 9001, (("osd0", OSD0, {}), ("cs3", CS3, {}))),
    "n70": (70, 20, ((0, 2), (33, 2), (69, 4)), False, 9102,
            (("osd0", OSD0, {}), ("cs3", CS3, {}), ("general", BP_ONLY, dict(general_form=True)), ("gosd", CS3, dict(general_osd=True)))),
    "h71": (70, 20, ((0, 2), (33, 2), (69, 4)), True, 9205, (("heavy", BP_ONLY, {}), ("hgosd", CS3, dict(general_osd=True)))),
}
TAGS = [f"{g}_{run[0]}" for g, v in GROUPS.items() for run in v[5]]


def rand_h(rng, m, n):
    """rand_h of tests/fuzz_bp4.py at density 2.2 / m"""
    H = (rng.random((m, n)) < 2.2 / m).astype(np.uint8)
    for r in range(m):
        if H[r].sum() == 0:
            H[r, rng.integers(n)] = 1
    for c in range(n):
        if H[:, c].sum() == 0:
            H[rng.integers(m), c] = 1
    return H


def construct(n, m, twins, heavy, seed):
    """Hx, Hz, priors, syndromes of one group"""
    rng = np.random.default_rng(seed)
    Hx, Hz = rand_h(rng, m, n), rand_h(rng, m, n)
    if heavy:  # one more qubit, on every random check of both matrices
        Hx, Hz = (np.concatenate([H, np.ones((m, 1), np.uint8)], axis=1) for H in (Hx, Hz))
        n += 1
    extra = np.zeros((sum(k for _, k in twins), n), np.uint8)
    r = 0
    for q, k in twins:
        extra[r:r + k, q] = 1
        r += k
    Hx, Hz = np.concatenate([Hx, extra]), np.concatenate([Hz, extra])
    px, py, pz = (rng.uniform(0.005, 0.03, size=n) for _ in range(3))
    u = rng.random((SHOTS, n))
    ex = (u < 2 * (px + py)).astype(np.uint8)                              # X or Y component
    ez = ((u >= 2 * px) & (u < 2 * (px + py + pz))).astype(np.uint8)       # Y or Z component
    sx, sz = (ez @ Hx.T) % 2, (ex @ Hz.T) % 2
    for s in (sx, sz):
        s[1::2, m:] = rng.integers(0, 2, size=s[1::2, m:].shape)
    return Hx, Hz, (px, py, pz), sx.astype(np.uint8), sz.astype(np.uint8)


def canonical(lp):
    lp = np.array(lp, dtype=np.float64)
    lp[np.isnan(lp)] = np.nan
    return lp


def keys_have_nan(lp):
    from tests.test_oracle_bp4 import _log1pexp, _logaddexp
    kx = [_log1pexp(-1. * x) - _logaddexp(-1. * y, -1. * z) for x, y, z in lp.tolist()]
    kz = [_log1pexp(-1. * z) - _logaddexp(-1. * y, -1. * x) for x, y, z in lp.tolist()]
    return bool(np.isnan(kx).any() or np.isnan(kz).any())


def coverage(conv, lpr_finite, key_nan, nan_lpr):
    """(shots that are not converged, not finite and have NaN-free keys; shots with NaN posteriors)"""
    return int(((conv == 0) & ~lpr_finite & (key_nan == 0)).sum()), int(nan_lpr.sum())


def record_run(ref, Hx, Hz, pr, sx, sz, kw, dev_kw):
    n = Hx.shape[1]
    outs, conv, its, bpd, o0, hashes, lprs, knan, lnan, fin = [], [], [], [], [], [], [], [], [], []
    for k in range(SHOTS):
        dec = ref.bp4_osd(Hx.astype(int), Hz.astype(int), channel_probs_x=pr[0], channel_probs_y=pr[1], channel_probs_z=pr[2], **kw)
        out = dec.decode(sx[k].astype(int), sz[k].astype(int))
        lp = canonical(dec.log_prob_ratios)
        assert lp.shape == (n, 3)
        outs.append(np.asarray(out, np.uint8)); conv.append(int(dec.converge)); its.append(int(dec.bp_iteration))
        bpd.append(np.stack([dec.bp_decoding_x, dec.bp_decoding_z]).astype(np.uint8))
        o0.append(np.stack([dec.osd0_decoding_x, dec.osd0_decoding_z]).astype(np.uint8))
        hashes.append(h64(lp)); knan.append(keys_have_nan(lp)); lnan.append(bool(np.isnan(lp).any())); fin.append(bool(np.isfinite(lp).all()))
        if k < LPR_FULL:
            lprs.append(lp)
    conv, knan, lnan = np.array(conv, np.uint8), np.array(knan, np.uint8), np.array(lnan, np.uint8)
    cov = coverage(conv, np.array(fin), knan, lnan)
    arrs = {"hx": pack(Hx), "hz": pack(Hz), "shape": np.array([Hx.shape[0], Hz.shape[0], n], np.int32), "px": pr[0], "py": pr[1], "pz": pr[2],
            "sx": pack(sx), "sz": pack(sz), "params": json.dumps(kw), "device_params": json.dumps(dev_kw), "out": pack(np.array(outs)),
            "converge": conv, "bp_iteration": np.array(its, np.int32), "bp_dec": pack(np.array(bpd)), "osd0": pack(np.array(o0)),
            "lpr": np.array(lprs), "lpr_hash": np.array(hashes, np.uint64), "key_nan": knan, "nan_lpr": lnan}
    return cov, arrs


def main():
    ensure_reference()
    import src as ref
    search = bool(os.environ.get("SWD_NONFINITE_SEARCH"))
    arrs = {}
    for g, (n, m, twins, heavy, seed, runs) in GROUPS.items():
        while True:
            Hx, Hz, pr, sx, sz = construct(n, m, twins, heavy, seed)
            from slidingwindowdecoder_amd import gf2
            if gf2.rank(Hx) < gf2.rank(Hz):  # the reference's higher-order z sweep reads past its column array there: undefined
                print(f"  bp4_nonfinite/{g}: seed {seed}: rank(Hx) < rank(Hz)")
                assert search, f"{g}: seed {seed} gives rank(Hx) < rank(Hz)"
                seed += 1
                continue
            try:
                res = [(name, record_run(ref, Hx, Hz, pr, sx, sz, kw, dev_kw)) for name, kw, dev_kw in runs]
            except ValueError as ex:  # (the reference's constructor refuses an OSD order beyond n - rank)
                res, why = None, str(ex)
            ok = res is not None and all(cov[0] >= 24 and cov[1] >= 3 for _, (cov, _) in res)
            print(f"  bp4_nonfinite/{g}: seed {seed}: " + (", ".join(f"{name} {cov}" for name, (cov, _) in res) if res else why))
            if ok or not search:
                break
            seed += 1
        assert ok, f"{g}: seed {seed} misses the coverage the fixture promises; run with SWD_NONFINITE_SEARCH=1 and write the seed down"
        for name, (_, a) in res:
            arrs.update({f"{g}_{name}_{k}": v for k, v in a.items()})
    arrs["tags"] = json.dumps(TAGS)
    path = os.path.join(HERE, "bp4_nonfinite.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote bp4_nonfinite.npz: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
