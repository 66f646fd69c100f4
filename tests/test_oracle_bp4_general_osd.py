"""bp4_osd.decode WITH OSD on the graphs the device takes with ``general_osd=True`` only -- the CAMEL and EG codes with a column that
touches every check, the EG code [[273,111,17]] -- in the oracle against the run recorded from the reference extension
(tests/golden/make_golden_bp4_general_osd.py).  The recording holds outputs only: the matrices, priors and syndromes are those of
bp4_heavy.npz / bp4_general.npz.  A new reference object per shot was recorded, so a new oracle object per shot equals it on EVERY
shot: vectors, the OSD-0 vectors, converge, iterations."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import fixtures as fx
from tests.test_oracle_bp4_general import load_general
from tests.test_oracle_bp4_heavy import load_heavy

OSD_TAGS = ["camel50", "eg73", "camel170", "two_heavy", "camel362", "eg273"]
BASE = dict(max_iter=50, ms_scaling_factor=0.8)
# constructor kwargs, shots, shots that reach the OSD
CASES = {"camel50": (dict(BASE, osd_method="osd0", osd_order=-1), 300, 42), "eg73": (dict(BASE, osd_method="osd_cs", osd_order=10), 200, 57),
         "camel170": (dict(BASE, osd_method="osd_e", osd_order=5), 120, 44), "two_heavy": (dict(BASE, osd_method="osd_cs", osd_order=6), 200, 48),
         "camel362": (dict(BASE, osd_method="osd_cs", osd_order=10), 40, 17), "eg273": (dict(BASE, osd_method="osd_cs", osd_order=10), 40, 15)}


@functools.lru_cache(maxsize=None)
def load_osd(tag):
    """the BP-only case of bp4_heavy.npz / bp4_general.npz (its fields as they are) with the OSD recording beside it: kw, out, osd0,
    converge, its"""
    f = fx.load("bp4_general_osd.npz")
    base = load_general(tag) if tag == "eg273" else load_heavy(tag)
    n = base["n"]
    return dict(base, kw=fx.params(f, tag + "_params"), out=fx.unpack(f[tag + "_out"], n), osd0=fx.unpack(f[tag + "_osd0"], n),
                converge=f[tag + "_converge"], its=f[tag + "_bp_iteration"], out_hash=f[tag + "_out_hash"])


@pytest.mark.parametrize("tag", OSD_TAGS)
def test_fixture_is_what_it_promises(tag):
    c = load_osd(tag)
    kw, shots, osd_shots = CASES[tag]
    assert c["kw"] == kw and c["out"].shape == c["osd0"].shape == (shots, 2, c["n"]) and len(c["sx"]) == shots
    assert fx.h64(c["out"]) == c["out_hash"]
    osd = c["converge"] == 0
    assert osd.sum() == osd_shots >= 5 and (~osd).sum() >= 5
    # BP does not depend on the OSD settings
    assert np.array_equal(c["converge"], c["decode_converge"]) and np.array_equal(c["its"], c["decode_its"])
    assert np.array_equal(c["out"][~osd], c["decode_out"][~osd]) and np.array_equal(c["osd0"][~osd], c["out"][~osd])
    # every correction the OSD returns satisfies both syndromes (the BP decisions of those shots do not)
    hx, hz = c["Hx"].astype(np.int64), c["Hz"].astype(np.int64)
    for vec in (c["out"], c["osd0"]):
        assert np.array_equal((vec[osd, 1] @ hx.T) % 2, c["sx"][osd]) and np.array_equal((vec[osd, 0] @ hz.T) % 2, c["sz"][osd])
    if kw["osd_order"] > 0:
        assert (c["out"][osd] != c["osd0"][osd]).any()  # the sweep found something better than OSD-0 on some shot


@pytest.mark.parametrize("tag", OSD_TAGS)
def test_decode_oracle_equals_the_reference_on_every_shot(tag):
    c = load_osd(tag)
    for k in range(len(c["sx"])):
        dec = O.bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c["kw"])
        out = dec.decode(c["sx"][k], c["sz"][k])
        assert (out == c["out"][k]).all(), f"shot {k}"
        assert (np.stack([dec.osd0_decoding_x, dec.osd0_decoding_z]) == c["osd0"][k]).all(), f"shot {k}: OSD-0"
        assert (dec.converge, dec.bp_iteration) == (c["converge"][k], c["its"][k]), f"shot {k}"
