"""bp4_osd(..., general_osd=True) on the device: the elimination kernel that keeps its arrays in HBM (huge_bp4_osd_kernel,
csrc/swd_huge_bp4.hip) behind the tuned BP kernels (graphs with heavy columns, and light graphs forced through it) and behind the
general BP form (``general_form=True`` beside it).  Against the runs recorded from the reference (tests/golden/bp4_general_osd.npz and
the OSD fixtures of the tuned path) and against a new oracle object per shot.  Every comparison is exact, on every shot: the ordering
keys come from bit-identical posteriors, the elimination is GF(2), and the path metrics are added in the reference's order."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import fixtures as fx
from tests.test_gpu_bp4_general import SEED, _rand_h, _syndromes, _uniform
from tests.test_oracle_bp4 import load_case, load_prefix
from tests.test_oracle_bp4_general import load_general
from tests.test_oracle_bp4_general_osd import OSD_TAGS, load_osd
from tests.test_oracle_bp4_heavy import load_heavy

pytestmark = pytest.mark.gpu
KW = dict(max_iter=50, ms_scaling_factor=0.8)
MODES = {"osd": dict(general_osd=True), "both": dict(general_osd=True, general_form=True)}
GENERAL_FORM = dict(split=0, lazy=0, fast=0, wmax=0, dm=0, threads=1024, skew=0, overlapped=0)
RANKS = {"camel50": (19, 19), "eg73": (27, 27), "camel170": (73, 73), "two_heavy": (24, 20), "camel362": (163, 163), "eg273": (81, 81)}


def _new(Hx, Hz, pr, kw, mode):
    from slidingwindowdecoder_amd import bp4_osd
    dec = bp4_osd(Hx, Hz, **pr, **kw, **MODES[mode])
    assert dec.general_osd is True and dec.general_form is (mode == "both")
    return dec


def _check_form(dec, mode, heavy):
    if mode == "both":
        assert dec.last_form == GENERAL_FORM and dec.heavy_columns == (0, 0)
    else:
        assert dec.last_form != GENERAL_FORM and dec.last_form["wmax"] > 0  # a tuned BP kernel ran
        assert (dec.heavy_columns[0] > 0) == heavy


# ---- the recording of the reference on the graphs only this path takes -------------------------------------------------------------
@pytest.mark.parametrize("mode", ["osd", "both"])
@pytest.mark.parametrize("tag", OSD_TAGS)
def test_recorded_cases_equal_the_reference_on_every_shot(tag, mode):
    """camel50 is cell 8's own spelling ("osd0", -1), which runs OSD-0 like the reference under the flag; two_heavy has rank 24
    against 20, the unequal-rank sweep; eg273 (every column heavy) only runs with the general BP form beside the elimination"""
    from slidingwindowdecoder_amd import bp4_osd
    c = load_osd(tag)
    if tag == "eg273" and mode == "osd":
        with pytest.raises(ValueError, match=r"column weight \d+ exceeds this build's bound 10 .*general_form=True"):
            bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c["kw"], general_osd=True)
        return
    dec = _new(c["Hx"], c["Hz"], c["pr"], c["kw"], mode)
    assert (dec.rank_x, dec.rank_z) == RANKS[tag]
    out = dec.decode_batch(c["sx"], c["sz"])
    _check_form(dec, mode, heavy=True)
    assert np.array_equal(out, c["out"])
    assert np.array_equal(dec.last_osd0, c["osd0"])
    assert np.array_equal((dec.last_status & 0x100) != 0, c["converge"] != 0)
    assert np.array_equal(dec.last_iterations, c["its"])
    assert np.array_equal((dec.last_status & 0xFF) == 2, c["converge"] == 0)  # exit class OSD on exactly the unconverged shots
    assert np.array_equal((dec.last_status & 0xFF) == 0, c["converge"] != 0)
    assert np.array_equal(dec.last_bp_decoding, c["decode_out"])  # the BP-only recording of bp4_heavy.npz / bp4_general.npz


def test_single_call_surface():
    """decode and the properties around it on one converged and one OSD shot of camel170 (osd_e 5), as on the tuned path"""
    c = load_osd("camel170")
    dec = _new(c["Hx"], c["Hz"], c["pr"], c["kw"], "osd")
    for want in (1, 0):
        k = int(np.flatnonzero(c["converge"] == want)[0])
        one = dec.decode(c["sx"][k], c["sz"][k])
        assert one.dtype == np.int64 and np.array_equal(one, c["out"][k])
        assert (dec.converge, dec.bp_iteration) == (want, c["its"][k])
        assert np.array_equal(np.stack([dec.osd0_decoding_x, dec.osd0_decoding_z]), c["osd0"][k])
        assert np.array_equal(np.stack([dec.bp_decoding_x, dec.bp_decoding_z]), c["decode_out"][k])
        if not want:
            assert np.array_equal(np.stack([dec.osdw_decoding_x, dec.osdw_decoding_z]), c["out"][k])
        assert fx.h64(dec.log_prob_ratios) == c["lpr_hash"][k]


# ---- the OSD fixtures of the tuned path, forced through the new kernel --------------------------------------------------------------
@pytest.mark.parametrize("mode", ["osd", "both"])
@pytest.mark.parametrize("tag", ["bb72_cs10", "bb72_e5", "bb144_osd0", "bb144_cs10"])
def test_recorded_light_fixtures_in_the_forced_kernel(tag, mode):
    c = load_case(tag)
    pr = dict(channel_probs_x=c["pr"], channel_probs_y=c["pr"], channel_probs_z=c["pr"])
    dec = _new(c["code"].hx, c["code"].hz, pr, c["kw"], mode)
    out = dec.decode_batch(c["sx"], c["sz"])
    _check_form(dec, mode, heavy=False)
    assert (c["converge"] == 0).sum() >= 5
    assert np.array_equal(out, c["out"]) and np.array_equal(dec.last_osd0, c["osd0"])
    assert np.array_equal((dec.last_status & 0xFF) == 2, c["converge"] == 0)


@pytest.mark.parametrize("mode", ["osd", "both"])
@pytest.mark.parametrize("tag", ["cs3", "e4"])
def test_recorded_unequal_ranks_in_the_forced_kernel(tag, mode):
    """rank(Hx) > rank(Hz): the z-basis sweep walks kx = n - rank_x candidates"""
    f = fx.load("bp4_unequal_ranks.npz")
    Hx, Hz = f[tag + "_hx"], f[tag + "_hz"]
    pr = dict(channel_probs_x=f[tag + "_px"], channel_probs_y=f[tag + "_py"], channel_probs_z=f[tag + "_pz"])
    dec = _new(Hx, Hz, pr, fx.params(f, tag + "_params"), mode)
    assert dec.rank_x > dec.rank_z
    sx, sz = fx.unpack(f[tag + "_sx"], Hx.shape[0]), fx.unpack(f[tag + "_sz"], Hz.shape[0])
    out = dec.decode_batch(sx, sz)
    assert np.array_equal(out, fx.unpack(f[tag + "_out"], Hx.shape[1]))
    if tag + "_osd0" in f:
        assert np.array_equal(dec.last_osd0, fx.unpack(f[tag + "_osd0"], Hx.shape[1]))
    assert np.array_equal((dec.last_status & 0xFF) == 2, f[tag + "_converge"] == 0)


@pytest.mark.parametrize("mode", ["osd", "both"])
@pytest.mark.parametrize("tag", ["cs4", "e3"])
def test_recorded_unequal_prefix_in_the_forced_kernel(tag, mode):
    """a rank-deficient sweep prefix on every OSD shot: the elimination must run over all n sorted columns"""
    c = load_prefix(tag)
    dec = _new(c["Hx"], c["Hz"], c["pr"], c["kw"], mode)
    out = dec.decode_batch(c["sx"], c["sz"])
    assert np.array_equal(out, c["out"]) and np.array_equal(dec.last_osd0, c["osd0"])
    assert np.array_equal((dec.last_status & 0xFF) == 2, c["converge"] == 0)


# ---- against a new oracle object per shot ---------------------------------------------------------------------------------------
def _oracle(Hx, Hz, pr, kw, sx, sz):
    from oracle import oracle as O
    r = dict(out=[], osd0=[], converge=[], its=[])
    for k in range(len(sx)):
        o = O.bp4_osd(Hx, Hz, **pr, **kw)
        r["out"].append(np.asarray(o.decode(sx[k], sz[k]), np.uint8))
        r["osd0"].append(np.stack([o.osd0_decoding_x, o.osd0_decoding_z]).astype(np.uint8))
        r["converge"].append(o.converge); r["its"].append(o.bp_iteration)
    return {k: np.array(v) for k, v in r.items()}


def _check_vs_oracle(dec, sx, sz, want):
    out = dec.decode_batch(sx, sz)
    assert np.array_equal(out, want["out"]) and np.array_equal(dec.last_osd0, want["osd0"])
    assert np.array_equal((dec.last_status & 0x100) != 0, want["converge"] != 0)
    assert np.array_equal((dec.last_status & 0xFF) == 2, want["converge"] == 0)
    assert np.array_equal(dec.last_iterations, want["its"])


@pytest.mark.parametrize("osd", [("osd0", 0), ("osd_cs", 10)])
def test_eg1057_equals_the_oracle(osd):
    """[[1057,571,33]]: 1024 checks of rank 243 (16 words per column of T, long runs of dependent columns in the pivot scan), 544 KB
    of messages; the 3 shots of the recorded 4 that BP leaves unconverged"""
    c = load_general("eg1057")
    kw = dict(KW, osd_method=osd[0], osd_order=osd[1])
    sel = np.flatnonzero(c["decode_converge"] == 0)
    assert len(sel) == 3
    sx, sz = c["sx"][sel], c["sz"][sel]
    want = _oracle(c["Hx"], c["Hz"], c["pr"], kw, sx, sz)
    assert not want["converge"].any() and np.array_equal(want["its"], c["decode_its"][sel])
    dec = _new(c["Hx"], c["Hz"], c["pr"], kw, "both")
    assert (dec.rank_x, dec.rank_z) == (243, 243)
    _check_vs_oracle(dec, sx, sz, want)
    assert np.array_equal(dec.last_bp_decoding, c["decode_out"][sel])


# tag: mx, mz, n, column weights lo..hi, p
RANDOM = {"dense": (65, 63, 150, 11, 16, 0.02), "tall": (1100, 1060, 1300, 3, 3, 0.02)}


@functools.lru_cache(maxsize=None)
def _random_case(tag, shots=16):
    mx, mz, n, lo, hi, p = RANDOM[tag]
    rng = np.random.default_rng(SEED)
    Hx, Hz = _rand_h(rng, mx, n, lo, hi), _rand_h(rng, mz, n, lo, hi)
    pr = _uniform(n, p)
    sx, sz = _syndromes(Hx, Hz, pr, shots)
    return dict(Hx=Hx, Hz=Hz, pr=pr, sx=sx, sz=sz, n=n)


@pytest.mark.parametrize("osd", [("osd_cs", 4), ("osd_e", 3)])
@pytest.mark.parametrize("tag", ["dense", "tall"])
def test_random_graphs_equal_the_oracle(tag, osd):
    """dense: 65 and 63 checks (two words and one word per column of T), every column of weight 11..16.  tall: 1100 and 1060 checks
    (18 and 17 words, past the tuned kernels' 1024), ranks 1062 > 1024 -- the unequal-rank sweep.  16 shots, at least 4 of them
    unconverged and at least one converged."""
    c = _random_case(tag)
    kw = dict(KW, osd_method=osd[0], osd_order=osd[1])
    want = _oracle(c["Hx"], c["Hz"], c["pr"], kw, c["sx"], c["sz"])
    assert 4 <= (want["converge"] == 0).sum() < 16
    dec = _new(c["Hx"], c["Hz"], c["pr"], kw, "both")
    _check_vs_oracle(dec, c["sx"], c["sz"], want)


def test_arbitrary_syndrome_bits_equal_the_oracle():
    """Syndromes that are random bits: the reference ignores an inconsistent system (it solves on the pivot rows alone), and so does
    the device.  The dense case has full row rank (65 of 65, 63 of 63), where every syndrome is consistent, so its last five rows of
    Hx are repeated here: rank 65 of 70 checks, and the random bits disagree on the repeated rows."""
    c = _random_case("dense")
    Hx = np.vstack([c["Hx"], c["Hx"][-5:]])
    rng = np.random.default_rng(SEED + 1)
    sx, sz = rng.integers(0, 2, (16, Hx.shape[0]), dtype=np.uint8), rng.integers(0, 2, (16, c["Hz"].shape[0]), dtype=np.uint8)
    assert (sx[:, -5:] != sx[:, -10:-5]).any()  # inconsistent on the repeated rows
    kw = dict(KW, osd_method="osd_cs", osd_order=4)
    want = _oracle(Hx, c["Hz"], c["pr"], kw, sx, sz)
    assert (want["converge"] == 0).sum() >= 4
    dec = _new(Hx, c["Hz"], c["pr"], kw, "both")
    assert (dec.rank_x, dec.rank_z) == (65, 63)
    _check_vs_oracle(dec, sx, sz, want)


# ---- surfaces -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["osd", "both"])
def test_two_launches_in_flight_equal_one_at_a_time(mode):
    """one handle, two streams, two launches in flight through decode_batch_device (each launch slot has its own elimination area):
    the results of one launch at a time, which are the recording's; and decode_batch(details=False)"""
    import torch
    from slidingwindowdecoder_amd import _lib
    c = load_osd("eg73")
    dec = _new(c["Hx"], c["Hz"], c["pr"], c["kw"], mode)
    dev = torch.device("cuda", 0)
    B, h = len(c["sx"]), len(c["sx"]) // 2 + 1
    t_sx, t_sz = torch.from_numpy(np.ascontiguousarray(c["sx"])).to(dev), torch.from_numpy(np.ascontiguousarray(c["sz"])).to(dev)
    out = torch.zeros((B, 2, c["n"]), dtype=torch.uint8, device=dev)
    st = torch.zeros((B, _lib.STAT_WORDS), dtype=torch.int32, device=dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    for s, (a, b) in zip(streams, ((0, h), (h, B))):
        with torch.cuda.stream(s):
            dec.decode_batch_device(t_sx[a:b], t_sz[a:b], out=out[a:b], stats=st[a:b], stream=s)
    torch.cuda.synchronize()
    single = _new(c["Hx"], c["Hz"], c["pr"], c["kw"], mode)
    want = np.concatenate([single.decode_batch(c["sx"][a:b], c["sz"][a:b]) for a, b in ((0, h), (h, B))])
    assert np.array_equal(want, c["out"])
    assert np.array_equal(out.cpu().numpy(), want)
    stats = st.cpu().numpy()
    assert np.array_equal((stats[:, 0] & 0xFF) == 2, c["converge"] == 0) and np.array_equal(stats[:, 1], c["its"])
    lean = single.decode_batch(c["sx"], c["sz"], details=False)
    assert np.array_equal(lean, c["out"]) and single.last_osd0 is None and single.last_llr is None
    assert np.array_equal(single.last_stats[:, :2], stats[:, :2])


def test_experiment_on_eg73_equals_the_oracle():
    """CodeCapacityExperiment passes general_osd through: the estimates of a batch are the oracle's decode of the batch's own
    syndromes, and the totals do not depend on batch size or lane count"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import CodeCapacityExperiment
    c = load_osd("eg73")
    kw = dict(KW, osd_method="osd_cs", osd_order=4)
    exp = CodeCapacityExperiment((c["Hx"], c["Hz"]), decoder="bp4_osd", method="decode", general_osd=True, **c["pr"], **kw)
    assert exp.decoder.general_osd and exp.decoder.heavy_columns[0] == 1
    shots = 64
    b = exp.run_batch(shots, seed=SEED)
    osd = 0
    for i in range(shots):
        o = O.bp4_osd(c["Hx"], c["Hz"], **c["pr"], **kw)
        assert np.array_equal(o.decode(b["sx"][i], b["sz"][i]), b["est"][i]), f"shot {i}"
        osd += 1 - o.converge
    print(f"eg73 experiment: {osd} of {shots} shots reach the OSD")
    a = exp.run(1024, batch=65536, lanes=4, seed=SEED)
    assert a.shots == 1024 and a == exp.run(1024, batch=200, lanes=3, seed=SEED)
    assert a.residual_syndromes == 0  # (the OSD always reproduces the syndrome)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_under_the_flag():
    from slidingwindowdecoder_amd import bp4_osd
    n = 4200
    rows = np.repeat(np.arange(4097), 2)
    H = sp.csr_matrix((np.ones(2 * 4097, np.uint8), (rows, (rows + np.tile([0, 1], 4097)) % n)), shape=(4097, n))
    with pytest.raises(ValueError, match=r"m=4097 exceeds the general OSD's limit of 4096 checks per matrix"):
        bp4_osd(H, H, **_uniform(n, 0.03), **KW, osd_method="osd0", osd_order=0, general_osd=True, general_form=True)
    t = load_heavy("two_heavy")  # rank 24 against 20, swapped: rank(Hx) < rank(Hz)
    for mode in MODES.values():
        with pytest.raises((ValueError, RuntimeError), match=r"rank\(Hx\) < rank\(Hz\)"):
            bp4_osd(t["Hz"], t["Hx"], **t["pr"], **KW, osd_method="osd_cs", osd_order=3, **mode)
        assert bp4_osd(t["Hz"], t["Hx"], **t["pr"], **KW, osd_method="osd0", osd_order=0, **mode).rank_z == 24  # (OSD-0 is defined)
        c = load_heavy("camel170")
        with pytest.raises((ValueError, RuntimeError), match=r"osd_e supports osd_order <= 15"):
            bp4_osd(c["Hx"], c["Hz"], **c["pr"], **KW, osd_method="osd_e", osd_order=16, **mode)
        with pytest.raises(ValueError, match=r"OSD order should be set in the range 0<=osd_oder<=97"):
            bp4_osd(c["Hx"], c["Hz"], **c["pr"], **KW, osd_method="osd_cs", osd_order=98, **mode)
        dec = bp4_osd(c["Hx"], c["Hz"], **c["pr"], **KW, osd_method="osd_cs", osd_order=-1, **mode)  # -1 stays "no OSD"
        out = dec.decode_batch(c["sx"][:32], c["sz"][:32])
        assert np.array_equal(out, c["decode_out"][:32]) and ((dec.last_status & 0xFF) != 2).all()


def test_without_the_flag_the_constructor_refuses_as_before():
    from slidingwindowdecoder_amd import bp4_osd
    c = load_heavy("camel50")
    for kw in (dict(osd_method="osd0", osd_order=0), dict(osd_method="osd_cs", osd_order=3)):
        with pytest.raises(ValueError, match=r"OSD on a graph with heavy columns \(1 of weight above 10, up to 21\) is not supported: create "
                                             r"the decoder with osd_order=-1 \(decode then returns the BP decisions\) or use camel_decode.*general_osd=True"):
            bp4_osd(c["Hx"], c["Hz"], **c["pr"], **KW, **kw)
        with pytest.raises(ValueError, match=r"OSD in the general form is not supported: create the decoder with osd_order=-1 \(decode then "
                                             r"returns the BP decisions\) or use camel_decode.*general_osd=True"):
            bp4_osd(c["Hx"], c["Hz"], **c["pr"], **KW, **kw, general_form=True)
    dec = bp4_osd(c["Hx"], c["Hz"], **c["pr"], **KW, osd_method="osd0", osd_order=-1)  # cell 8's spelling: the -1 stands
    assert dec.general_osd is False
    out = dec.decode_batch(c["sx"][:64], c["sz"][:64])
    assert np.array_equal(out, c["decode_out"][:64]) and ((dec.last_status & 0xFF) != 2).all()
