"""bp4_osd on graphs with heavy columns -- the cycle-assembled (CAMEL) and EG codes of Misc.ipynb cells 6-8, H = (H1 | 1), whose last
qubit touches every check, and random matrices with two heavy columns elsewhere -- in the oracle against the run recorded from the
reference extension (tests/golden/make_golden_heavy.py).  The recording used a new reference object per shot, so a new oracle object
per shot equals it on EVERY shot, in both methods; posteriors exactly (oracle and reference call the same libm here, and the oracle
adds the check messages of a column in the reference's order whatever its weight)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import fixtures as fx

HEAVY_TAGS = ["camel50", "eg73", "camel170", "two_heavy", "camel362"]
# (n, heavy columns, their weights in Hx, in Hz)
SHAPES = {"camel50": (50, [49], [21], [21]), "eg73": (73, [72], [64], [64]), "camel170": (170, [169], [78], [78]),
          "two_heavy": (60, [0, 31], [13, 20], [11, 20]), "camel362": (362, [361], [171], [171])}


@functools.lru_cache(maxsize=None)
def load_heavy(tag):
    f = fx.load("bp4_heavy.npz")
    g = lambda k: f[f"{tag}_{k}"]
    mx, mz, n = (int(x) for x in g("shape"))
    Hx, Hz = fx.unpack(g("hx"), n), fx.unpack(g("hz"), n)
    return dict(Hx=Hx, Hz=Hz, mx=mx, mz=mz, n=n, heavy=g("heavy"),
                pr=dict(channel_probs_x=g("px"), channel_probs_y=g("py"), channel_probs_z=g("pz")),
                camel_kw=fx.params(f, tag + "_camel_params"), decode_kw=fx.params(f, tag + "_decode_params"),
                sx=fx.unpack(g("sx"), mx), sz=fx.unpack(g("sz"), mz),
                camel_out=fx.unpack(g("camel_out"), n), camel_converge=g("camel_converge"), camel_its=g("camel_bp_iteration"),
                camel_min_pm=g("camel_min_pm"),
                decode_out=fx.unpack(g("decode_out"), n), decode_converge=g("decode_converge"), decode_its=g("decode_bp_iteration"),
                lpr_hash=g("decode_lpr_hash"), lpr=g("decode_lpr"), lpr_heavy=g("decode_lpr_heavy"))


@pytest.mark.parametrize("tag", HEAVY_TAGS)
def test_fixture_is_what_it_promises(tag):
    """The shapes the cases were chosen for, cell 8's parameters, and the coverage the generator asserts: both exits of BP in both
    methods, every Pauli of the last qubit among the camel winners."""
    c = load_heavy(tag)
    n, heavy, wx, wz = SHAPES[tag]
    assert c["n"] == n and c["heavy"].tolist() == heavy
    assert c["Hx"].sum(0)[heavy].tolist() == wx and c["Hz"].sum(0)[heavy].tolist() == wz
    light = np.setdiff1d(np.arange(n), heavy)
    assert max(c["Hx"].sum(0)[light].max(), c["Hz"].sum(0)[light].max()) <= 10
    assert c["camel_kw"] == dict(max_iter=50, ms_scaling_factor=0.8, osd_method="osd0", osd_order=-1)
    assert c["decode_kw"] == dict(max_iter=50, ms_scaling_factor=0.8, osd_method="osd_cs", osd_order=-1)
    assert (c["pr"]["channel_probs_x"][-1], c["pr"]["channel_probs_y"][-1], c["pr"]["channel_probs_z"][-1]) == (0.10, 0.06, 0.08)
    for conv in (c["camel_converge"], c["decode_converge"]):
        assert (conv == 1).sum() >= 5 and (conv == 0).sum() >= 5
    win = (c["camel_out"][:, 0, -1] + 2 * c["camel_out"][:, 1, -1])[c["camel_converge"] == 1]
    assert min((win == 1).sum(), (win == 2).sum(), (win == 3).sum()) >= 3
    dead = c["camel_converge"] == 0  # a shot without a converged run: the state of a new object
    assert not c["camel_out"][dead].any() and (c["camel_min_pm"][dead] == 10000.0).all()


@pytest.mark.parametrize("tag", HEAVY_TAGS)
def test_camel_decode_oracle_equals_the_reference_on_every_shot(tag):
    c = load_heavy(tag)
    for k in range(len(c["sx"])):
        dec = O.bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c["camel_kw"])
        out = dec.camel_decode(c["sx"][k], c["sz"][k])
        assert (out == c["camel_out"][k]).all(), f"shot {k}"
        assert (dec.converge, dec.bp_iteration, dec.min_pm) == (c["camel_converge"][k], c["camel_its"][k], c["camel_min_pm"][k]), f"shot {k}"


@pytest.mark.parametrize("tag", HEAVY_TAGS)
def test_decode_oracle_equals_the_reference_on_every_shot(tag):
    """decode with osd_order = -1: vectors, converge, iterations, and the three posteriors of every qubit -- by hash on every shot, in
    full on the first shots and on the heavy qubits (the check on the order their 2 x weight check messages are added in)."""
    c = load_heavy(tag)
    for k in range(len(c["sx"])):
        dec = O.bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c["decode_kw"])
        out = dec.decode(c["sx"][k], c["sz"][k])
        assert (out == c["decode_out"][k]).all(), f"shot {k}"
        assert (dec.converge, dec.bp_iteration) == (c["decode_converge"][k], c["decode_its"][k]), f"shot {k}"
        lpr = dec.log_prob_ratios
        assert np.array_equal(lpr[c["heavy"]], c["lpr_heavy"][k]), f"shot {k}: posteriors of the heavy qubits"
        assert fx.h64(lpr) == c["lpr_hash"][k], f"shot {k}: posteriors"
        if k < len(c["lpr"]):
            assert np.array_equal(lpr, c["lpr"][k]), f"shot {k}"
