"""bp4_osd(..., general_form=True) on the device (csrc/swd_huge_bp4.hip): the BP4 kernel without degree or size bounds, against
the runs recorded from the reference (tests/golden/bp4_heavy.npz, forced into this form; tests/golden/bp4_general.npz, the EG codes
only this form takes) and against a new oracle object per shot on graphs past each bound of the tuned kernels.  Everything is
compared exactly on every shot: exp / log1p are the reference's libm algorithms and a node's check messages are added in the
reference's order, so there is no tolerance and no shot is left out."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import fixtures as fx
from tests.test_gpu_bp4_heavy import _check_decode, _with_heavy_columns
from tests.test_oracle_bp4_general import load_general
from tests.test_oracle_bp4_heavy import load_heavy

pytestmark = pytest.mark.gpu
SEED = 20240318
GENERAL_FORM = dict(split=0, lazy=0, fast=0, wmax=0, dm=0, threads=1024, skew=0, overlapped=0)
KW = dict(max_iter=50, ms_scaling_factor=0.8)
CAMEL_KW = dict(KW, osd_method="osd0", osd_order=-1)
DECODE_KW = dict(KW, osd_method="osd_cs", osd_order=-1)


def _new(Hx, Hz, pr, kw, **more):
    from slidingwindowdecoder_amd import bp4_osd
    return bp4_osd(Hx, Hz, **pr, **kw, general_form=True, **more)


def _check_camel(dec, out, c, sel=slice(None)):
    """_check_camel of test_gpu_bp4_heavy.py without its first line: that one asserts heavy_columns[0] > 0, and the general form
    reports (0, 0) -- no column is special here.  The four comparisons are the same."""
    assert dec.heavy_columns == (0, 0)
    assert np.array_equal(out, c["camel_out"][sel])
    assert np.array_equal((dec.last_status & 0x100) != 0, c["camel_converge"][sel] != 0)
    assert np.array_equal(dec.last_iterations, c["camel_its"][sel])
    assert np.array_equal(dec.last_min_pm, c["camel_min_pm"][sel])


def _is_general(dec):
    assert dec.general_form is True and dec.heavy_columns == (0, 0)
    assert dec.last_form == GENERAL_FORM


# ---- recorded fixtures --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["camel50", "eg73", "two_heavy", "camel170"])
def test_recorded_heavy_fixtures_in_the_forced_form(tag):
    """graphs the HEAVY form takes, forced into the general form: vectors, converge, iterations, min_pm, the heavy qubits'
    posteriors and the posterior hashes of every shot equal the recording"""
    c = load_heavy(tag)
    dec = _new(c["Hx"], c["Hz"], c["pr"], c["decode_kw"])
    assert dec.last_form is None and (dec.mx, dec.mz, dec.n) == (c["mx"], c["mz"], c["n"])
    out = dec.decode_batch(c["sx"], c["sz"], return_llr=True)
    _is_general(dec)
    _check_decode(dec, out, c, dec.last_llr)
    assert ((dec.last_status & 0xFF) != 2).all()  # no OSD exit
    conv = c["decode_converge"] != 0
    assert np.array_equal(dec.last_osd0[conv], out[conv]) and not dec.last_osd0[~conv].any()
    assert np.array_equal(dec.last_bp_decoding, out)
    cam = _new(c["Hx"], c["Hz"], c["pr"], c["camel_kw"])  # (cell 8's spelling: osd0 with -1, which stands)
    _check_camel(cam, cam.camel_decode_batch(c["sx"], c["sz"]), c)
    _is_general(cam)


@pytest.mark.parametrize("tag", ["eg273", "eg1057"])
def test_eg_codes_equal_the_recording(tag):
    """create_EG_codes(4) and (5): every column above the weight bound, the last one of weight m; (5) has 544 KB of messages"""
    from slidingwindowdecoder_amd import bp4_osd
    c = load_general(tag)
    with pytest.raises(ValueError, match=r"column weight \d+ exceeds this build's bound 10 .*general_form=True"):
        bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c["decode_kw"])
    dec = _new(c["Hx"], c["Hz"], c["pr"], c["decode_kw"])
    out = dec.decode_batch(c["sx"], c["sz"], return_llr=True)
    _is_general(dec)
    _check_decode(dec, out, c, dec.last_llr)
    cam = _new(c["Hx"], c["Hz"], c["pr"], c["camel_kw"])
    _check_camel(cam, cam.camel_decode_batch(c["sx"], c["sz"]), c)
    out = cam.decode_batch(c["sx"], c["sz"], return_llr=True)  # decode under cell 8's spelling: the BP decisions
    _check_decode(cam, out, c, cam.last_llr)


# ---- graphs only this form takes, against the oracle ----------------------------------------------------------------------------
def _rand_h(rng, m, n, lo, hi):
    H = np.zeros((m, n), np.uint8)
    for col in range(n):
        w = int(rng.integers(lo, hi + 1))
        H[rng.choice(m, size=w, replace=False), col] = 1
    return H


def _uniform(n, p):
    return dict(channel_probs_x=np.full(n, p / 3), channel_probs_y=np.full(n, p / 3), channel_probs_z=np.full(n, p / 3))


def _syndromes(Hx, Hz, pr, shots, seed=7):
    rng = np.random.default_rng(seed)
    px, py, pz = pr["channel_probs_x"], pr["channel_probs_y"], pr["channel_probs_z"]
    noise = rng.uniform(0, 1, (shots, Hx.shape[1]))
    err_z = (noise > px) & (noise < px + py + pz)
    err_x = noise < px + py
    return ((err_z.astype(np.int64) @ Hx.T.astype(np.int64)) % 2).astype(np.uint8), \
        ((err_x.astype(np.int64) @ Hz.T.astype(np.int64)) % 2).astype(np.uint8)


def _oracle_runs(Hx, Hz, pr, sx, sz):
    """a new oracle object per shot, both methods: the recording's fields"""
    from oracle import oracle as O
    r = dict(decode_out=[], decode_converge=[], decode_its=[], lpr=[], camel_out=[], camel_converge=[], camel_its=[], camel_min_pm=[])
    for k in range(len(sx)):
        o = O.bp4_osd(Hx, Hz, **pr, **DECODE_KW)
        r["decode_out"].append(np.asarray(o.decode(sx[k], sz[k]), np.uint8))
        r["decode_converge"].append(o.converge); r["decode_its"].append(o.bp_iteration); r["lpr"].append(o.log_prob_ratios.copy())
        o = O.bp4_osd(Hx, Hz, **pr, **CAMEL_KW)
        r["camel_out"].append(np.asarray(o.camel_decode(sx[k], sz[k]), np.uint8))
        r["camel_converge"].append(o.converge); r["camel_its"].append(o.bp_iteration); r["camel_min_pm"].append(o.min_pm)
    return {k: np.array(v) for k, v in r.items()}


# tag: mx, mz, n, column weights lo..hi, p -- the bound each crosses is in the test's docstring
RANDOM = {"dense": (40, 36, 96, 11, 16, 0.02), "wide": (48, 44, 1100, 3, 3, 0.004), "tall": (1100, 1060, 1300, 3, 3, 0.02),
          "lds": (1000, 960, 3600, 3, 3, 0.06)}  # (lds: the oracle converges on 5 of its 8 shots in both methods at this rate)


@functools.lru_cache(maxsize=None)
def _random_case(tag, shots=32):
    mx, mz, n, lo, hi, p = RANDOM[tag]
    rng = np.random.default_rng(SEED)
    Hx = _rand_h(rng, mx, n, lo, hi)
    Hz = _rand_h(rng, mz, n, lo, hi)
    pr = _uniform(n, p)
    sx, sz = _syndromes(Hx, Hz, pr, shots)
    return dict(Hx=Hx, Hz=Hz, pr=pr, sx=sx, sz=sz, n=n, **_oracle_runs(Hx, Hz, pr, sx, sz))


def _check_vs_oracle(c, sel=slice(None)):
    dec = _new(c["Hx"], c["Hz"], c["pr"], DECODE_KW)
    out = dec.decode_batch(c["sx"][sel], c["sz"][sel], return_llr=True)
    _is_general(dec)
    assert np.array_equal(out, c["decode_out"][sel])
    assert np.array_equal((dec.last_status & 0x100) != 0, c["decode_converge"][sel] != 0)
    assert np.array_equal(dec.last_iterations, c["decode_its"][sel])
    bad = [k for k, (g, w) in enumerate(zip(np.transpose(dec.last_llr, (0, 2, 1)), c["lpr"][sel])) if not np.array_equal(g, w)]
    assert not bad, f"posteriors differ on shots {bad[:10]}"
    cam = _new(c["Hx"], c["Hz"], c["pr"], CAMEL_KW)
    _check_camel(cam, cam.camel_decode_batch(c["sx"][sel], c["sz"][sel]), c, sel)
    _is_general(cam)


@pytest.mark.parametrize("tag", ["dense", "wide", "tall"])
def test_graphs_past_a_bound_equal_the_oracle(tag):
    """dense: every column above the weight bound (11..16).  wide: rows up to weight 94, more nodes than threads.  tall: more than
    1024 checks, more edges than threads.  32 shots, both methods, posteriors included, with both exits of BP among them."""
    from slidingwindowdecoder_amd import bp4_osd
    c = _random_case(tag)
    with pytest.raises((ValueError, RuntimeError), match="general_form=True"):
        bp4_osd(c["Hx"], c["Hz"], **c["pr"], **DECODE_KW)
    if tag == "dense":
        assert min(c["Hx"].sum(0).min(), c["Hz"].sum(0).min()) >= 11
    if tag == "wide":
        assert c["Hx"].sum(1).max() > 64 and c["n"] > 1024
    if tag == "tall":
        assert min(c["Hx"].shape[0], c["Hz"].shape[0]) > 1024 and c["Hx"].sum() > 1024
    for conv in (c["decode_converge"], c["camel_converge"]):
        assert 0 < conv.sum() < 32
    _check_vs_oracle(c)


@functools.lru_cache(maxsize=None)
def _refused_case(which):
    """the two matrices test_refusals (tests/test_gpu_bp4_heavy.py) builds on two_heavy: a ninth heavy column, and a light column of
    weight 11 beside eight heavy ones -- 64 shots of two_heavy"""
    t = load_heavy("two_heavy")
    rng = np.random.default_rng(9)
    eight = [0, 31, 5, 12, 20, 40, 50, 59]
    Hx8 = _with_heavy_columns(t["Hx"], eight[2:], rng)
    if which == "nine":
        Hx = _with_heavy_columns(Hx8, [45], rng)
    else:
        Hx = Hx8.copy()
        Hx[:, 46] = 0
        Hx[:11, 46] = 1
    sx, sz = t["sx"][:64], t["sz"][:64]
    return dict(Hx=Hx, Hz=t["Hz"], pr=t["pr"], sx=sx, sz=sz, n=t["n"], **_oracle_runs(Hx, t["Hz"], t["pr"], sx, sz))


@pytest.mark.parametrize("which", ["nine", "weight11"])
def test_the_matrices_the_default_constructor_refuses(which):
    from slidingwindowdecoder_amd import bp4_osd
    c = _refused_case(which)
    with pytest.raises(ValueError, match=r"column weight 1[12] exceeds this build's bound 10"):
        bp4_osd(c["Hx"], c["Hz"], **c["pr"], **DECODE_KW)
    assert 0 < c["decode_converge"].sum() < 64
    _check_vs_oracle(c)


def test_a_light_graph_past_the_lds_bound():
    """1000 x 3600 and 960 x 3600 of column weight 3: 21 600 edges, 173 KB of messages -- refused with the LDS text by default"""
    from slidingwindowdecoder_amd import bp4_osd
    c = _random_case("lds", 8)
    assert (c["Hx"].sum() + c["Hz"].sum() + 2) * 8 > 160 * 1024
    assert 0 < c["decode_converge"].sum() < 8 and 0 < c["camel_converge"].sum() < 8
    with pytest.raises(RuntimeError, match=r"code needs \d+ bytes of LDS per shot \(> 163840\).*general_form=True"):
        bp4_osd(c["Hx"], c["Hz"], **c["pr"], **DECODE_KW)
    _check_vs_oracle(c)


# ---- surfaces -----------------------------------------------------------------------------------------------------------------
def _surface_case(tag):
    return _random_case(tag) if tag == "dense" else load_general(tag)


@pytest.mark.parametrize("tag", ["dense", "eg273"])
def test_batch_surfaces_agree(tag):
    """one batch as two launches on two streams through decode_batch_device (posteriors included), and the same halves through
    camel_decode_batch: the results of the single launch"""
    import torch
    from slidingwindowdecoder_amd import _lib
    c = _surface_case(tag)
    kw = c.get("decode_kw", DECODE_KW)
    dec = _new(c["Hx"], c["Hz"], c["pr"], kw)
    dev = torch.device("cuda", 0)
    B, h = len(c["sx"]), len(c["sx"]) // 2 + 1
    t_sx, t_sz = torch.from_numpy(np.ascontiguousarray(c["sx"])).to(dev), torch.from_numpy(np.ascontiguousarray(c["sz"])).to(dev)
    out = torch.zeros((B, 2, c["n"]), dtype=torch.uint8, device=dev)
    st = torch.zeros((B, _lib.STAT_WORDS), dtype=torch.int32, device=dev)
    llr = torch.zeros((B, 3, c["n"]), dtype=torch.float64, device=dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    for s, (a, b) in zip(streams, ((0, h), (h, B))):
        with torch.cuda.stream(s):
            dec.decode_batch_device(t_sx[a:b], t_sz[a:b], out=out[a:b], stats=st[a:b], llr=llr[a:b], stream=s)
    torch.cuda.synchronize()
    stats = st.cpu().numpy()
    single = _new(c["Hx"], c["Hz"], c["pr"], kw)
    want = single.decode_batch(c["sx"], c["sz"], return_llr=True)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(want, c["decode_out"])
    assert np.array_equal(stats[:, :2], single.last_stats[:, :2])
    assert np.array_equal(llr.cpu().numpy(), single.last_llr)
    cam = _new(c["Hx"], c["Hz"], c["pr"], c.get("camel_kw", CAMEL_KW))
    for a, b in ((0, h), (h, B)):
        _check_camel(cam, cam.camel_decode_batch(c["sx"][a:b], c["sz"][a:b]), c, slice(a, b))


def test_single_call_surface():
    """camel_decode / decode on one converged and one unconverged shot of eg273"""
    c = load_general("eg273")
    cam, dec = _new(c["Hx"], c["Hz"], c["pr"], c["camel_kw"]), _new(c["Hx"], c["Hz"], c["pr"], c["decode_kw"])
    for want in (1, 0):
        k = int(np.flatnonzero(c["camel_converge"] == want)[0])
        one = cam.camel_decode(c["sx"][k], c["sz"][k])
        assert one.dtype == np.int64 and np.array_equal(one, c["camel_out"][k])
        assert (cam.converge, cam.bp_iteration, cam.min_pm) == (want, c["camel_its"][k], c["camel_min_pm"][k])
        k = int(np.flatnonzero(c["decode_converge"] == want)[0])
        one = dec.decode(c["sx"][k], c["sz"][k])
        assert one.dtype == np.int64 and np.array_equal(one, c["decode_out"][k])
        assert (dec.converge, dec.bp_iteration) == (want, c["decode_its"][k])
        assert np.array_equal(dec.log_prob_ratios[c["heavy"]], c["lpr_heavy"][k])
        assert fx.h64(dec.log_prob_ratios) == c["lpr_hash"][k]


def test_empty_and_one_shot_batches():
    c = _random_case("dense")
    dec, cam = _new(c["Hx"], c["Hz"], c["pr"], DECODE_KW), _new(c["Hx"], c["Hz"], c["pr"], CAMEL_KW)
    assert dec.decode_batch(c["sx"][:0], c["sz"][:0]).shape == (0, 2, c["n"])
    assert cam.camel_decode_batch(c["sx"][:0], c["sz"][:0]).shape == (0, 2, c["n"])
    for k in (0, 31):
        _check_vs_oracle(c, slice(k, k + 1))


# ---- the experiment -------------------------------------------------------------------------------------------------------------
class _Code:
    def __init__(self, hx, hz):
        self.hx, self.hz, self.N = hx, hz, hx.shape[1]


def test_camel_experiment_on_eg273_equals_the_host_loop():
    """Misc.ipynb cell 8 on the [[273,111,17]] code through CodeCapacityExperiment with general_form=True: result words of a batch
    against a host loop over the oracle, and totals that do not depend on batch size or lane count (four launches in flight)."""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import CodeCapacityExperiment, gf2
    from tests import pauli_ref as P
    c = load_general("eg273")
    code, shots = _Code(c["Hx"], c["Hz"]), 48
    hx_perp, hz_perp = gf2.nullspace(code.hx), gf2.nullspace(code.hz)
    kw = dict(**c["pr"], **c["camel_kw"])
    pr = c["pr"]
    err, sx, sz = P.sample(code.hx, code.hz, pr["channel_probs_x"], pr["channel_probs_y"], pr["channel_probs_z"], shots, SEED)
    est, words = np.zeros_like(err), np.zeros(shots, np.int32)
    hx64, hz64 = code.hx.astype(np.int64), code.hz.astype(np.int64)
    for i in range(shots):
        dec = O.bp4_osd(code.hx, code.hz, **kw)
        est[i] = dec.camel_decode(sx[i], sz[i])
        dx, dz = est[i, 0] ^ err[i, 0], est[i, 1] ^ err[i, 1]
        residual = bool(((hz64 @ dx) % 2).any() or ((hx64 @ dz) % 2).any())
        words[i] = int(P.reference_logical_error(dx, dz, hx_perp, hz_perp)) | (2 if residual else 0) | (0 if dec.converge else 4)
    exp = CodeCapacityExperiment((code.hx, code.hz), decoder="bp4_osd", method="camel_decode", general_form=True, **kw)
    assert exp.decoder.general_form and exp.decoder.heavy_columns == (0, 0)
    b = exp.run_batch(shots, seed=SEED)
    assert (b["err"] == err).all() and (b["est"] == est).all() and (b["result"] == words).all()
    assert 0 < (words & 4 != 0).sum() < shots
    a = exp.run(2048, batch=65536, lanes=4, seed=SEED)
    assert a.shots == 2048 and a == exp.run(2048, batch=300, lanes=3, seed=SEED)
    r = exp.run(shots, batch=20, lanes=4, seed=SEED)
    assert (r.shots, r.logical_errors, r.not_converged) == (shots, int((words & 1).sum()), int((words & 4 != 0).sum()))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from slidingwindowdecoder_amd import bp4_osd
    c = _random_case("dense")
    with pytest.raises(ValueError, match=r"osd_order=-1.*camel_decode"):  # the form runs no OSD
        bp4_osd(c["Hx"], c["Hz"], **c["pr"], **KW, osd_method="osd0", osd_order=0, general_form=True)
    with pytest.raises(ValueError, match=r"osd_order=-1.*camel_decode"):
        bp4_osd(c["Hx"], c["Hz"], **c["pr"], **KW, osd_method="osd_cs", osd_order=3, general_form=True)
    assert bp4_osd(load_heavy("camel50")["Hx"], load_heavy("camel50")["Hz"], **load_heavy("camel50")["pr"], **DECODE_KW).general_form is False


def test_a_graph_beyond_the_bounds_of_the_form():
    """1 048 577 qubits: one past the documented bound of the form (include/swd.h)"""
    from slidingwindowdecoder_amd import bp4_osd
    n = (1 << 20) + 1
    H = sp.csr_matrix((np.ones(4, np.uint8), ([0, 0, 1, 1], [0, 1, 1, n - 1])), shape=(2, n))
    with pytest.raises(ValueError, match=r"n=1048577 exceeds bp4_osd's general form limit of 1048576 qubits"):
        bp4_osd(H, H, **_uniform(n, 0.03), **DECODE_KW, general_form=True)
