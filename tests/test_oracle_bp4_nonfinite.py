"""bp4_osd where the posteriors are NOT finite, in the oracle against the run recorded from the reference extension
(tests/golden/make_golden_bp4_nonfinite.py): a qubit under several degree-1 checks sums their +-1e308 sentinels to +-inf, and
inf - inf gives NaN.  BP is defined there and pinned on EVERY shot: posteriors bit for bit (NaN at the same positions), converge
flag, iteration count, BP decisions.  The OSD is defined as long as its ordering keys are NaN-free -- infinite keys sort well -- and
on those shots the returned vector and the OSD-0 vectors are pinned too; a NaN key goes through std::stable_sort in the reference
(bpgd.cpp:384-389), which leaves the order undefined: the vector and the OSD-0 vectors of such a shot are the only things outside
parity.  A new reference object per shot was recorded, so a new oracle object per shot equals it."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import fixtures as fx
from tests.test_oracle_bp4 import _log1pexp, _logaddexp

TAGS = ["n24_osd0", "n24_cs3", "n70_osd0", "n70_cs3", "n70_general", "n70_gosd", "h71_heavy", "h71_hgosd"]
SHOTS, LPR_FULL = 48, 16


@functools.lru_cache(maxsize=None)
def load_nonfinite(tag):
    f = fx.load("bp4_nonfinite.npz")
    mx, mz, n = (int(x) for x in f[tag + "_shape"])
    return dict(Hx=fx.unpack(f[tag + "_hx"], n), Hz=fx.unpack(f[tag + "_hz"], n), n=n, mx=mx, mz=mz,
                pr=dict(channel_probs_x=f[tag + "_px"], channel_probs_y=f[tag + "_py"], channel_probs_z=f[tag + "_pz"]),
                kw=fx.params(f, tag + "_params"), dev_kw=fx.params(f, tag + "_device_params"),
                sx=fx.unpack(f[tag + "_sx"], mx), sz=fx.unpack(f[tag + "_sz"], mz), out=fx.unpack(f[tag + "_out"], n),
                bp_dec=fx.unpack(f[tag + "_bp_dec"], n), osd0=fx.unpack(f[tag + "_osd0"], n), converge=f[tag + "_converge"],
                its=f[tag + "_bp_iteration"], lpr=f[tag + "_lpr"], lpr_hash=f[tag + "_lpr_hash"], key_nan=f[tag + "_key_nan"],
                nan_lpr=f[tag + "_nan_lpr"])


def canonical(lp):
    """the posteriors [n, 3] with every NaN set to one bit pattern: what the fixture hashes"""
    lp = np.array(lp, dtype=np.float64)
    lp[np.isnan(lp)] = np.nan
    return lp


def keys_have_nan(lp):
    """an OSD ordering key of either basis (swd_oracle.c bp4_osd_basis) is NaN"""
    rows = np.asarray(lp).tolist()
    kx = [_log1pexp(-1. * x) - _logaddexp(-1. * y, -1. * z) for x, y, z in rows]
    kz = [_log1pexp(-1. * z) - _logaddexp(-1. * y, -1. * x) for x, y, z in rows]
    return bool(np.isnan(kx).any() or np.isnan(kz).any())


def same_posteriors(got, want):
    """bit for bit, two NaNs equal whatever their payload"""
    return canonical(got).tobytes() == canonical(want).tobytes()


def test_fixture_lists_its_cases():
    f = fx.load("bp4_nonfinite.npz")
    assert fx.params(f, "tags") == TAGS
    # the matrix pairs are shared as the generator says
    for a, b in (("n24_osd0", "n24_cs3"), ("n70_osd0", "n70_cs3"), ("n70_cs3", "n70_general"), ("n70_cs3", "n70_gosd"), ("h71_heavy", "h71_hgosd")):
        ca, cb = load_nonfinite(a), load_nonfinite(b)
        assert np.array_equal(ca["Hx"], cb["Hx"]) and np.array_equal(ca["Hz"], cb["Hz"]) and np.array_equal(ca["sx"], cb["sx"])
    c = load_nonfinite("n24_osd0")
    assert (c["n"], c["mx"], c["mz"]) == (24, 13, 13) and c["Hx"][8:].sum(1).tolist() == [1] * 5 and c["Hx"][8:, 0].sum() == 2 and c["Hx"][8:, 5].sum() == 3
    c = load_nonfinite("n70_cs3")
    assert (c["n"], c["mx"], c["mz"]) == (70, 28, 28) and [int(c["Hz"][20:, q].sum()) for q in (0, 33, 69)] == [2, 2, 4]
    assert c["kw"] == dict(ms_scaling_factor=0.625, max_iter=12, osd_method="osd_cs", osd_order=3)
    assert load_nonfinite("n70_osd0")["kw"] == dict(ms_scaling_factor=0.625, max_iter=3, osd_method="osd_0", osd_order=0)
    c = load_nonfinite("h71_heavy")
    assert c["n"] == 71 and c["Hx"][:20, 70].all() and c["Hz"][:20, 70].all() and c["kw"]["osd_order"] == -1
    assert max(c["Hx"][:, :70].sum(0).max(), c["Hz"][:, :70].sum(0).max()) <= 10
    assert load_nonfinite("n70_general")["dev_kw"] == dict(general_form=True) and load_nonfinite("n70_gosd")["dev_kw"] == dict(general_osd=True)
    for tag in TAGS:
        c = load_nonfinite(tag)
        assert ((c["pr"]["channel_probs_x"] >= 0.005) & (c["pr"]["channel_probs_x"] <= 0.03)).all()
        assert c["out"].shape == c["bp_dec"].shape == c["osd0"].shape == (SHOTS, 2, c["n"]) and c["lpr"].shape == (LPR_FULL, c["n"], 3)


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_equals_the_reference_on_every_shot(tag):
    c = load_nonfinite(tag)
    good = nan_shots = 0
    for k in range(SHOTS):
        dec = O.bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c["kw"])
        out = dec.decode(c["sx"][k], c["sz"][k])
        lp = dec.log_prob_ratios
        assert fx.h64(canonical(lp)) == c["lpr_hash"][k], f"shot {k}: posteriors"
        if k < LPR_FULL:
            assert same_posteriors(lp, c["lpr"][k]) and np.array_equal(np.isnan(lp), np.isnan(c["lpr"][k])), f"shot {k}: posteriors"
        assert (dec.converge, dec.bp_iteration) == (c["converge"][k], c["its"][k]), f"shot {k}"
        assert np.array_equal(np.stack([dec.bp_decoding_x, dec.bp_decoding_z]), c["bp_dec"][k]), f"shot {k}: BP decisions"
        key_nan = keys_have_nan(lp)
        assert key_nan == bool(c["key_nan"][k]) and bool(np.isnan(lp).any()) == bool(c["nan_lpr"][k]), f"shot {k}"
        if not key_nan:
            assert np.array_equal(out, c["out"][k]), f"shot {k}: vector"
            assert np.array_equal(np.stack([dec.osd0_decoding_x, dec.osd0_decoding_z]), c["osd0"][k]), f"shot {k}: OSD-0"
        good += (not dec.converge) and (not np.isfinite(lp).all()) and not key_nan
        nan_shots += bool(np.isnan(lp).any())
    # the conditions of the fixture (the generator asserts the same on the reference's posteriors)
    print(f"{tag}: {good} unconverged non-finite shots with NaN-free keys, {nan_shots} shots with NaN posteriors")
    assert good >= 24 and nan_shots >= 3
