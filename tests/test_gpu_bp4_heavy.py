"""bp4_osd on the device for graphs with heavy columns (the HEAVY form of the BP kernel, csrc/swd_bp4_kernel.h) against the run
recorded from the reference (tests/golden/bp4_heavy.npz; tests/test_oracle_bp4_heavy.py pins the fixture against the oracle).
Everything is compared exactly on every shot: the device evaluates exp / log1p with the reference's libm algorithms and adds a heavy
qubit's check messages in the reference's order, so there is no tolerance and no shot is left out."""
import functools

import numpy as np
import pytest

from tests import fixtures as fx
from tests.test_oracle_bp4_heavy import HEAVY_TAGS, SHAPES, load_heavy

pytestmark = pytest.mark.gpu
SEED = 20240318


@functools.lru_cache(maxsize=None)
def _dec(tag, which):
    from slidingwindowdecoder_amd import bp4_osd
    c = load_heavy(tag)
    return bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c[which + "_kw"])


def _expected_info(tag):
    _, _, wx, wz = SHAPES[tag]
    return len(wx), max(wx + wz)


@pytest.mark.parametrize("tag", HEAVY_TAGS)
def test_construction_reports_the_heavy_columns(tag):
    """cell 8's parameters (osd_method="osd0", osd_order=-1) and decode's (osd_cs, -1) both construct; the decoder found the
    fixture's heavy columns"""
    for which in ("camel", "decode"):
        dec = _dec(tag, which)
        assert dec.heavy_columns == _expected_info(tag)
        assert (dec.mx, dec.mz, dec.n) == (load_heavy(tag)["mx"], load_heavy(tag)["mz"], load_heavy(tag)["n"])


def _check_camel(dec, out, c, sel=slice(None)):
    assert dec.heavy_columns[0] > 0
    assert np.array_equal(out, c["camel_out"][sel])
    assert np.array_equal((dec.last_status & 0x100) != 0, c["camel_converge"][sel] != 0)
    assert np.array_equal(dec.last_iterations, c["camel_its"][sel])
    assert np.array_equal(dec.last_min_pm, c["camel_min_pm"][sel])


@pytest.mark.parametrize("tag", HEAVY_TAGS)
def test_camel_decode_batch_equals_the_reference_on_every_shot(tag):
    c = load_heavy(tag)
    dec = _dec(tag, "camel")
    out = dec.camel_decode_batch(c["sx"], c["sz"])
    _check_camel(dec, out, c)
    f = dec.last_form
    assert (f["split"], f["lazy"], f["fast"], f["dm"]) == (0, 0, 0, 10) and f["threads"] == (c["n"] + 63) // 64 * 64


def _check_decode(dec, out, c, lpr):
    assert np.array_equal(out, c["decode_out"])
    assert np.array_equal((dec.last_status & 0x100) != 0, c["decode_converge"] != 0)
    assert np.array_equal(dec.last_iterations, c["decode_its"])
    got = np.ascontiguousarray(np.transpose(lpr, (0, 2, 1)))  # [B, n, 3] like log_prob_ratios
    assert np.array_equal(got[:, c["heavy"]], c["lpr_heavy"]), "posteriors of the heavy qubits: the order of their sums"
    assert np.array_equal(got[: len(c["lpr"])], c["lpr"])
    bad = [k for k in range(len(got)) if fx.h64(got[k]) != c["lpr_hash"][k]]
    assert not bad, f"posteriors differ on shots {bad[:10]}"


@pytest.mark.parametrize("tag", HEAVY_TAGS)
def test_decode_batch_equals_the_reference_on_every_shot(tag):
    """osd_order = -1: vectors, converge, iterations, and the three posteriors of every qubit"""
    c = load_heavy(tag)
    dec = _dec(tag, "decode")
    out = dec.decode_batch(c["sx"], c["sz"], return_llr=True)
    assert dec.heavy_columns[0] > 0
    _check_decode(dec, out, c, dec.last_llr)
    assert ((dec.last_status & 0xFF) != 2).all()  # no OSD exit


@pytest.mark.parametrize("tag", HEAVY_TAGS)
def test_decode_with_cell8_spelling_returns_the_bp_decisions(tag):
    """The documented deviation: on a graph with heavy columns osd_method="osd0", osd_order=-1 keeps the caller's -1 (the reference
    resets it to 0 and would run OSD-0), so ``decode`` on that handle equals the run recorded with osd_cs / -1 on every shot."""
    c = load_heavy(tag)
    dec = _dec(tag, "camel")
    assert c["camel_kw"]["osd_method"] == "osd0" and c["camel_kw"]["osd_order"] == -1
    out = dec.decode_batch(c["sx"], c["sz"], return_llr=True)
    _check_decode(dec, out, c, dec.last_llr)
    assert ((dec.last_status & 0xFF) != 2).all()  # no OSD exit


@pytest.mark.parametrize("tag", ["eg73", "camel170"])
def test_fewer_threads_than_qubits(tag, monkeypatch):
    """SWD_BP4_NT=64 (read at create): n > 64, so a thread serves several nodes and finds the heavy ones by looking them up, the
    posteriors go straight to the output, and the checks have no thread of their own -- same results on every shot"""
    from slidingwindowdecoder_amd import bp4_osd
    c = load_heavy(tag)
    monkeypatch.setenv("SWD_BP4_NT", "64")
    dec = bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c["decode_kw"])
    cam = bp4_osd(c["Hx"], c["Hz"], **c["pr"], **c["camel_kw"])
    monkeypatch.delenv("SWD_BP4_NT")
    out = dec.decode_batch(c["sx"], c["sz"], return_llr=True)
    assert dec.last_form["threads"] == 64 < c["n"] and c["mx"] + c["mz"] > 64
    _check_decode(dec, out, c, dec.last_llr)
    _check_camel(cam, cam.camel_decode_batch(c["sx"], c["sz"]), c)
    assert cam.last_form["threads"] == 64


def test_eight_heavy_columns_equal_the_oracle():
    """eight heavy columns at any position, six of them heavy in Hx only (weight 12 there, 3 in Hz): decode with posteriors and
    camel_decode against a new oracle object per shot"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import bp4_osd
    t = load_heavy("two_heavy")
    Hx8 = _with_heavy_columns(t["Hx"], [5, 12, 20, 40, 50, 59], np.random.default_rng(9))
    heavy = [0, 5, 12, 20, 31, 40, 50, 59]
    assert Hx8.sum(0)[heavy].tolist() == [13, 12, 12, 12, 20, 12, 12, 12] and t["Hz"].sum(0)[heavy].tolist() == [11, 3, 3, 3, 20, 3, 3, 3]
    sx, sz = t["sx"][:64], t["sz"][:64]
    dec = bp4_osd(Hx8, t["Hz"], **t["pr"], **t["decode_kw"])
    assert dec.heavy_columns == (8, 20)
    out = dec.decode_batch(sx, sz, return_llr=True)
    cam = bp4_osd(Hx8, t["Hz"], **t["pr"], **t["camel_kw"])  # (the decided qubit 59 is one of the heavy ones)
    cout = cam.camel_decode_batch(sx, sz)
    conv = 0
    for k in range(len(sx)):
        o = O.bp4_osd(Hx8, t["Hz"], **t["pr"], **t["decode_kw"])
        assert np.array_equal(o.decode(sx[k], sz[k]), out[k]), f"shot {k}"
        assert (o.converge, o.bp_iteration) == (int((dec.last_status[k] & 0x100) != 0), dec.last_iterations[k]), f"shot {k}"
        assert np.array_equal(o.log_prob_ratios, dec.last_llr[k].T), f"shot {k}: posteriors"
        conv += o.converge
        o = O.bp4_osd(Hx8, t["Hz"], **t["pr"], **t["camel_kw"])
        assert np.array_equal(o.camel_decode(sx[k], sz[k]), cout[k]), f"shot {k}"
        assert (o.converge, o.bp_iteration, o.min_pm) == (int((cam.last_status[k] & 0x100) != 0), cam.last_iterations[k], cam.last_min_pm[k])
    assert 0 < conv < len(sx)


@pytest.mark.parametrize("tag", ["camel50", "two_heavy", "camel170"])
def test_batch_surfaces_agree(tag):
    """one batch as two launches on two streams through decode_batch_device (posteriors included), and the same halves through
    camel_decode_batch: the results of the single launch"""
    import torch
    from slidingwindowdecoder_amd import _lib
    c = load_heavy(tag)
    dec = _dec(tag, "decode")
    dev = torch.device("cuda", 0)
    B, h = len(c["sx"]), len(c["sx"]) // 2 + 1
    t_sx, t_sz = torch.from_numpy(c["sx"]).to(dev), torch.from_numpy(c["sz"]).to(dev)
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
    dec.last_status, dec.last_iterations = stats[:, 0], stats[:, 1]
    _check_decode(dec, out.cpu().numpy(), c, llr.cpu().numpy())
    cam = _dec(tag, "camel")
    for a, b in ((0, h), (h, B)):
        _check_camel(cam, cam.camel_decode_batch(c["sx"][a:b], c["sz"][a:b]), c, slice(a, b))


@pytest.mark.parametrize("tag", HEAVY_TAGS)
def test_single_call_surface(tag):
    """camel_decode / decode on one converged and one unconverged shot per case"""
    c = load_heavy(tag)
    cam, dec = _dec(tag, "camel"), _dec(tag, "decode")
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


class _Code:
    def __init__(self, hx, hz):
        self.hx, self.hz, self.N = hx, hz, hx.shape[1]


def test_camel_experiment_on_camel50_equals_the_host_loop():
    """Misc.ipynb cell 8 on the [[50,12,6]] code through CodeCapacityExperiment: result words of a batch against a host loop over
    the oracle (a new object per shot, as on the device), and totals that do not depend on batch size or lane count."""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import CodeCapacityExperiment, gf2
    from tests import pauli_ref as P
    c = load_heavy("camel50")
    code, shots = _Code(c["Hx"], c["Hz"]), 384
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
    exp = CodeCapacityExperiment((code.hx, code.hz), decoder="bp4_osd", method="camel_decode", **kw)
    assert exp.decoder.heavy_columns == (1, 21)
    b = exp.run_batch(shots, seed=SEED)
    assert (b["err"] == err).all() and (b["est"] == est).all() and (b["result"] == words).all()
    a = exp.run(4096, seed=SEED)
    assert a.shots == 4096 and a == exp.run(4096, batch=500, lanes=3, seed=SEED)
    r = exp.run(shots, batch=200, lanes=2, seed=SEED)
    assert (r.shots, r.logical_errors, r.not_converged) == (shots, int((words & 1).sum()), int((words & 4 != 0).sum()))


def _with_heavy_columns(H, cols, rng):
    H = H.copy()
    for v in cols:
        H[:, v] = 0
        H[rng.choice(H.shape[0], size=12, replace=False), v] = 1
    return H


def test_refusals():
    from slidingwindowdecoder_amd import bp4_osd
    c = load_heavy("camel50")
    with pytest.raises(ValueError, match=r"osd_order=-1.*camel_decode"):  # OSD on a graph with heavy columns
        bp4_osd(c["Hx"], c["Hz"], **c["pr"], max_iter=50, ms_scaling_factor=0.8, osd_method="osd0", osd_order=0)
    with pytest.raises(ValueError, match=r"osd_order=-1.*camel_decode"):
        bp4_osd(c["Hx"], c["Hz"], **c["pr"], max_iter=50, ms_scaling_factor=0.8, osd_method="osd_cs", osd_order=3)
    t = load_heavy("two_heavy")
    rng = np.random.default_rng(9)
    kw = dict(**t["pr"], **t["decode_kw"])
    eight = [0, 31, 5, 12, 20, 40, 50, 59]
    Hx8 = _with_heavy_columns(t["Hx"], eight[2:], rng)
    assert bp4_osd(Hx8, t["Hz"], **kw).heavy_columns == (8, 20)  # eight heavy columns, at any position: accepted
    with pytest.raises(ValueError, match=r"column weight 12 exceeds this build's bound 10 .*up to 8 heavy columns"):
        bp4_osd(_with_heavy_columns(Hx8, [45], rng), t["Hz"], **kw)  # a ninth
    Hx9 = Hx8.copy()  # a light column of weight 11 next to the eight heavy ones: beyond the bound of the ELL tables
    Hx9[:, 46] = 0
    Hx9[:11, 46] = 1
    with pytest.raises(ValueError, match=r"column weight 11 exceeds this build's bound 10"):
        bp4_osd(Hx9, t["Hz"], **kw)


@pytest.mark.parametrize("tag", ["bb72", "bb144"])
def test_graphs_without_heavy_columns_take_the_forms_they_took(tag):
    """the BB-code cases of bp4_camel.npz: no heavy column, and the forms of the launcher's rules for them -- camel runs the generic
    form on ceil(n / 64) waves, decode the specialised one (two threads per qubit for [[72]], the two-half update for [[144]])"""
    from slidingwindowdecoder_amd import bp4_osd
    from tests.test_oracle_bp4 import load_camel
    c = load_camel(tag)
    dec = bp4_osd(c["code"].hx, c["code"].hz, channel_probs_x=c["px"], channel_probs_y=c["py"], channel_probs_z=c["pz"], **c["kw"])
    assert dec.heavy_columns == (0, 0)
    dec.camel_decode_batch(c["sx"][:16], c["sz"][:16])
    n = c["code"].N
    assert dec.last_form == dict(split=0, lazy=0, fast=0, wmax=4, dm=4, threads=(n + 63) // 64 * 64, skew=0, overlapped=0)
    dec.decode_batch(c["sx"][:16], c["sz"][:16])
    want = dict(split=1, lazy=0, fast=1, wmax=4, dm=4, threads=192, skew=0, overlapped=0) if tag == "bb72" else \
        dict(split=0, lazy=1, fast=1, wmax=4, dm=4, threads=192, skew=0, overlapped=0)
    assert dec.last_form == want
