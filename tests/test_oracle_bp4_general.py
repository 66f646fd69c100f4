"""bp4_osd on the graphs only the general form of the device decoder takes -- the Euclidean-geometry codes [[273,111,17]] and
[[1057,571,33]] of Misc.ipynb cell 8, H = (H1 | 1): every column above the weight bound of the tuned kernels, the last one touching
every check -- in the oracle against the run recorded from the reference extension (tests/golden/make_golden_general.py).  A new
reference object per shot was recorded, so a new oracle object per shot equals it on EVERY shot, in both methods, posteriors exactly.
The large code costs about 1.5 s per oracle shot, hence its 4 shots."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import fixtures as fx

GENERAL_TAGS = ["eg273", "eg1057"]
# n, checks per matrix, weight of every column but the last, weight of the last column, row weight, p, shots
SHAPES = {"eg273": (273, 256, 16, 256, 18, 0.06, 40), "eg1057": (1057, 1024, 32, 1024, 34, 0.04, 4)}


@functools.lru_cache(maxsize=None)
def load_general(tag):
    f = fx.load("bp4_general.npz")
    g = lambda k: f[f"{tag}_{k}"]
    mx, mz, n = (int(x) for x in g("shape"))
    Hx = fx.unpack(g("hx"), n)
    Hz = fx.unpack(g("hz"), n) if f"{tag}_hz" in f else Hx  # (stored once where Hz equals Hx)
    return dict(Hx=Hx, Hz=Hz, mx=mx, mz=mz, n=n, heavy=g("heavy"),
                pr=dict(channel_probs_x=g("px"), channel_probs_y=g("py"), channel_probs_z=g("pz")),
                camel_kw=fx.params(f, tag + "_camel_params"), decode_kw=fx.params(f, tag + "_decode_params"),
                sx=fx.unpack(g("sx"), mx), sz=fx.unpack(g("sz"), mz),
                camel_out=fx.unpack(g("camel_out"), n), camel_converge=g("camel_converge"), camel_its=g("camel_bp_iteration"),
                camel_min_pm=g("camel_min_pm"),
                decode_out=fx.unpack(g("decode_out"), n), decode_converge=g("decode_converge"), decode_its=g("decode_bp_iteration"),
                lpr_hash=g("decode_lpr_hash"), lpr=g("decode_lpr"), lpr_heavy=g("decode_lpr_heavy"))


@pytest.mark.parametrize("tag", GENERAL_TAGS)
def test_fixture_is_what_it_promises(tag):
    """the measured shapes of the two codes, cell 8's parameters, uniform priors, and the coverage the generator asserts"""
    c = load_general(tag)
    n, m, w, w_last, row_w, p, shots = SHAPES[tag]
    assert (c["n"], c["mx"], c["mz"]) == (n, m, m) and c["Hx"].shape == c["Hz"].shape == (m, n)
    assert np.array_equal(c["Hx"], c["Hz"]) and c["heavy"].tolist() == [n - 1]
    assert (c["Hx"].sum(0)[:-1] == w).all() and c["Hx"].sum(0)[-1] == w_last and (c["Hx"].sum(1) == row_w).all()
    assert c["camel_kw"] == dict(max_iter=50, ms_scaling_factor=0.8, osd_method="osd0", osd_order=-1)
    assert c["decode_kw"] == dict(max_iter=50, ms_scaling_factor=0.8, osd_method="osd_cs", osd_order=-1)
    for q in c["pr"].values():
        assert (q == p / 3).all()
    assert len(c["sx"]) == len(c["sz"]) == shots
    least = 5 if tag == "eg273" else 1
    for conv in ((c["camel_converge"], c["decode_converge"]) if tag == "eg273" else (c["decode_converge"],)):
        assert (conv == 1).sum() >= least and (conv == 0).sum() >= least
    dead = c["camel_converge"] == 0  # a shot without a converged run: the state of a new object
    assert not c["camel_out"][dead].any() and (c["camel_min_pm"][dead] == 10000.0).all()
    assert len(c["lpr"]) >= 1 and len(c["lpr_heavy"]) == len(c["lpr_hash"]) == shots


@pytest.mark.parametrize("tag", GENERAL_TAGS)
def test_camel_decode_oracle_equals_the_reference_on_every_shot(tag):
    c = load_general(tag)
    for k in range(len(c["sx"])):
        dec = O.bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c["camel_kw"])
        out = dec.camel_decode(c["sx"][k], c["sz"][k])
        assert (out == c["camel_out"][k]).all(), f"shot {k}"
        assert (dec.converge, dec.bp_iteration, dec.min_pm) == (c["camel_converge"][k], c["camel_its"][k], c["camel_min_pm"][k]), f"shot {k}"


@pytest.mark.parametrize("tag", GENERAL_TAGS)
def test_decode_oracle_equals_the_reference_on_every_shot(tag):
    """decode with osd_order = -1: vectors, converge, iterations, and the three posteriors of every qubit -- by hash on every shot, in
    full on the first shots and on the last qubit (the order in which its 2 x m check messages are added)"""
    c = load_general(tag)
    for k in range(len(c["sx"])):
        dec = O.bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c["decode_kw"])
        out = dec.decode(c["sx"][k], c["sz"][k])
        assert (out == c["decode_out"][k]).all(), f"shot {k}"
        assert (dec.converge, dec.bp_iteration) == (c["decode_converge"][k], c["decode_its"][k]), f"shot {k}"
        lpr = dec.log_prob_ratios
        assert np.array_equal(lpr[c["heavy"]], c["lpr_heavy"][k]), f"shot {k}: posteriors of the last qubit"
        assert fx.h64(lpr) == c["lpr_hash"][k], f"shot {k}: posteriors"
        if k < len(c["lpr"]):
            assert np.array_equal(lpr, c["lpr"][k]), f"shot {k}"
