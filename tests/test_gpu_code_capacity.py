"""Code-capacity experiments on the device: the Pauli sampler against its numpy restatement (tests/pauli_ref.py) bit for bit, the
CSS accounting against numpy, and CodeCapacityExperiment end to end against a host loop that takes the restated errors, decodes them
with the oracle shot by shot and applies the reference's criterion (/root/reference/Misc.ipynb cells 2 and 8, src/simulation.py)."""
import functools

import numpy as np
import pytest

from slidingwindowdecoder_amd import gf2
from slidingwindowdecoder_amd.codes import bb_code
from tests import pauli_ref as P
from tests import philox_ref

pytestmark = pytest.mark.gpu
SEED = 20240318


@functools.lru_cache(maxsize=None)
def _bb(N):
    code, _, _ = bb_code(N)
    return code


@functools.lru_cache(maxsize=None)
def _perps(N):
    code = _bb(N)
    return gf2.nullspace(code.hx), gf2.nullspace(code.hz)


def _random_probs(n, seed):
    """per-qubit px, py, pz; qubit 1 never errs, qubit 2 always does (sum exactly 1)"""
    rng = np.random.default_rng(seed)
    px, py, pz = rng.uniform(0.0, 0.3, n), rng.uniform(0.0, 0.3, n), rng.uniform(0.0, 0.3, n)
    px[1] = py[1] = pz[1] = 0.0
    px[2], py[2], pz[2] = 0.25, 0.25, 0.5
    return px, py, pz


def _random_sparse(m, n, w, seed):
    rng = np.random.default_rng(seed)
    H = np.zeros((m, n), np.uint8)
    for r in range(m):
        H[r, rng.choice(n, size=w, replace=False)] = 1
    return H


def _sampler_matrices(name):
    if name == "bb72":
        return _bb(72).hx, _bb(72).hz
    if name == "shyps3":  # n = 49: not a multiple of 4
        from slidingwindowdecoder_amd import shyps
        return shyps.shyps_stabilizers(3)
    if name == "bb288":  # n > 256: more than one stride of a wave
        return _bb(288).hx, _bb(288).hz
    # n = 601 > 512: a shot takes the whole workgroup; the sampler does not need the matrices to commute
    return _random_sparse(150, 601, 7, 1), _random_sparse(131, 601, 5, 2)


@pytest.mark.parametrize("name", ["bb72", "shyps3", "bb288", "random601"])
def test_sampler_equals_the_restatement(name):
    """err, sx, sz bit for bit; 257 shots (not a multiple of the shots per workgroup) from shot 2^32 - 100 on, so that the high
    counter word changes inside the batch; the host and the device entry point; any cut into calls."""
    from slidingwindowdecoder_amd import PauliSampler
    Hx, Hz = _sampler_matrices(name)
    n = Hx.shape[1]
    px, py, pz = _random_probs(n, 40 + n)
    smp = PauliSampler(Hx, Hz, px, py, pz)
    assert (smp.mx, smp.mz, smp.n) == (Hx.shape[0], Hz.shape[0], n)
    first = 2 ** 32 - 100
    want = P.sample(Hx, Hz, px, py, pz, 257, SEED, first)
    got = smp.sample(257, seed=SEED, first_shot=first)
    for g, w, what in zip(got, want, ("err", "sx", "sz")):
        assert g.dtype == np.uint8 and g.shape == w.shape and (g == w).all(), f"{name}: {what} differs from the restatement"
    assert not got[0][:, :, 1].any() and (got[0][:, :, 2].sum(axis=1) >= 1).all()
    assert got[0][:, 0].any() and got[0][:, 1].any() and got[1].any() and got[2].any()
    dev = [t.cpu().numpy() for t in smp.sample_device(257, seed=SEED, first_shot=first)]
    assert all((d == w).all() for d, w in zip(dev, want))
    # a key of more than 32 bits, and the default first shot
    big = (0xABCDEF12 << 32) | 77
    assert all((g == w).all() for g, w in zip(smp.sample(9, seed=big), P.sample(Hx, Hz, px, py, pz, 9, big)))
    whole, a, b = smp.sample(300), smp.sample(100), smp.sample(200, first_shot=100)
    assert all((np.concatenate([x, y]) == w).all() for x, y, w in zip(a, b, whole))


def _result_words(cx, stab_x, cz, stab_z, d, stats=None):
    """numpy accounting: d [B, 2, n] with both matrices, [B, n] with one"""
    B = d.shape[0]
    odd = np.zeros(B, bool)
    stab = np.zeros(B, bool)
    for mat, s, string in ((cx, stab_x, d[:, 1] if d.ndim == 3 else d), (cz, stab_z, d[:, 0] if d.ndim == 3 else d)):
        if mat is None:
            continue
        par = (string.astype(np.int64) @ np.asarray(mat, np.int64).T) % 2
        odd |= par.any(axis=1)
        stab |= par[:, :s].any(axis=1)
    w = odd.astype(np.int32) | (stab.astype(np.int32) << 1)
    if stats is not None:
        w |= ((stats[:, 0] & 0x100) == 0).astype(np.int32) << 2
    return w


def _account(acct, est, err, stats=None, counters=None, est_pad=0):
    """run the device accounting on numpy arrays; est_pad > 0 puts the estimate into rows of a wider buffer (a byte stride)"""
    import torch
    B = est.shape[0]
    dev = torch.device("cuda", 0)
    e = torch.from_numpy(np.ascontiguousarray(est)).to(dev)
    if est_pad:
        wide = torch.zeros((B, est[0].size + est_pad), dtype=torch.uint8, device=dev)
        wide[:, :est[0].size] = e.reshape(B, -1)
        e = wide[:, :est[0].size]
    r = torch.from_numpy(np.ascontiguousarray(err)).to(dev)
    s = torch.from_numpy(np.ascontiguousarray(stats)).to(dev) if stats is not None else None
    res = torch.full((B,), -1, dtype=torch.int32, device=dev)
    acct.account(B, e, r, s, res, counters, torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    return res.cpu().numpy()


def test_accounting_equals_numpy_bb72():
    import torch
    from slidingwindowdecoder_amd.decoders import _CssAccount
    code = _bb(72)
    hx, hz, lx, lz = code.hx, code.hz, code.lx, code.lz
    cx, cz = np.vstack([hx, lx]), np.vstack([hz, lz])
    acct = _CssAccount(cx, hx.shape[0], cz, hz.shape[0], 0)
    rng = np.random.default_rng(23)
    zero = np.zeros(72, np.uint8)
    one = zero.copy(); one[17] = 1
    # crafted differences (X string, Z string) and the word each must give
    crafted = [((zero, zero), 0), ((hx[3], hz[5]), 0), ((hx[1] ^ hx[7], zero), 0),          # nothing, stabilisers
               ((lx[0], zero), 1), ((zero, lz[4]), 1), ((lx[2] ^ hx[9], lz[1] ^ hz[30]), 1),  # logical operators: bit 0 only
               ((one, zero), 3), ((zero, one), 3),                                          # one qubit: a residual syndrome
               ((lz[0], zero), 3), ((zero, lx[0]), 3)]                                      # a logical in the other string is detected
    B = 301
    err = rng.integers(0, 2, (B, 2, 72)).astype(np.uint8)
    d = rng.integers(0, 2, (B, 2, 72)).astype(np.uint8)
    d[100:] = (rng.random((B - 100, 2, 72)) < 0.01)  # sparse differences: some shots give 0
    for k, ((dx, dz), _) in enumerate(crafted):
        d[k, 0], d[k, 1] = dx, dz
    est = d ^ err
    want = _result_words(cx, hx.shape[0], cz, hz.shape[0], d)
    assert [int(w) for w in want[:len(crafted)]] == [w for _, w in crafted]
    assert set(np.unique(want)) == {0, 1, 3}
    got = _account(acct, est, err)
    assert (got == want).all()
    assert (_account(acct, est, err, est_pad=5) == want).all()  # an odd byte stride
    # the stats column: bit 2 where the converge bit of word 0 is clear; counters add up over two calls
    stats = rng.integers(0, 6, (B, 8)).astype(np.int32)
    stats[::3, 0] |= 0x100
    want_s = _result_words(cx, hx.shape[0], cz, hz.shape[0], d, stats)
    counters = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    assert (_account(acct, est, err, stats=stats, counters=counters) == want_s).all()
    assert ((want_s & 4) != 0).sum() == B - len(range(0, B, 3))
    tally = lambda w: [len(w), int((w & 1 != 0).sum()), int((w & 2 != 0).sum()), int((w & 4 != 0).sum())]  # noqa: E731
    assert counters.cpu().tolist() == tally(want_s)
    assert (_account(acct, est[:77], err[:77], counters=counters) == want[:77]).all()
    assert counters.cpu().tolist() == [a + b for a, b in zip(tally(want_s), tally(want[:77]))]
    # single-string forms: one matrix, n bytes per shot (the binary decoders' case), either basis
    for kw, mat, s in ((dict(cx=cx, stab_x=36, cz=None, stab_z=0), cx, 36), (dict(cx=None, stab_x=0, cz=cz, stab_z=36), cz, 36)):
        one_acct = _CssAccount(kw["cx"], kw["stab_x"], kw["cz"], kw["stab_z"], 0)
        d1 = d[:, 1].copy()
        d1[0], d1[1], d1[2], d1[3] = zero, (hz if kw["cz"] is None else hx)[4], (lz if kw["cz"] is None else lx)[3], one
        w1 = _result_words(mat, s, None, 0, d1)
        assert w1[:4].tolist() == [0, 0, 1, 3]
        assert (_account(one_acct, d1 ^ err[:, 0], err[:, 0]) == w1).all()


def test_accounting_large_code_and_many_logicals():
    """n = 601 > 512 takes a workgroup per shot; 40 logical rows (no 32-observable limit); 5000 shots make every workgroup of the
    launch walk more than one group of shots."""
    import torch
    from slidingwindowdecoder_amd.decoders import _CssAccount
    rng = np.random.default_rng(29)
    for n, B in ((601, 700), (72, 9001)):
        cx = np.vstack([_random_sparse(150, n, 7, 3), _random_sparse(40, n, 31, 4)])
        cz = np.vstack([_random_sparse(131, n, 5, 5), _random_sparse(40, n, 29, 6)])
        cx[:150, 0], cx[150, 0] = 0, 1  # qubit 0 of the Z string: seen by a logical row only
        acct = _CssAccount(cx, 150, cz, 131, 0)
        err = rng.integers(0, 2, (B, 2, n)).astype(np.uint8)
        d = (rng.random((B, 2, n)) < 0.002).astype(np.uint8)
        d[::7] = 0
        d[7, 1, 0] = 1
        want = _result_words(cx, 150, cz, 131, d)
        assert want[0] == 0 and want[7] == 1 and {0, 1, 3} == set(np.unique(want))
        counters = torch.zeros(4, dtype=torch.int64, device="cuda:0")
        assert (_account(acct, d ^ err, err, counters=counters) == want).all()
        assert counters.cpu().tolist() == [B, int((want & 1 != 0).sum()), int((want & 2 != 0).sum()), 0]


BP4_KW = dict(max_iter=32, ms_scaling_factor=0.625, osd_method="osd_cs", osd_order=10)


@functools.lru_cache(maxsize=None)
def _bp4_host_loop(case):
    """restated errors -> oracle.bp4_osd shot by shot -> the reference's criterion.  Computed once per case, never modified."""
    from oracle import oracle as O
    code = _bb(72)
    hx_perp, hz_perp = _perps(72)
    if case == "depolarizing":
        pr = np.full(72, 0.06 / 3)
        probs, shots, first = (pr, pr, pr), 2048, 0
    else:  # per-qubit biased noise; the high counter word changes inside the batch
        rng = np.random.default_rng(77)
        probs = (rng.uniform(0.002, 0.02, 72), rng.uniform(0.001, 0.01, 72), rng.uniform(0.02, 0.07, 72))
        shots, first = 1024, 2 ** 32 - 500
    kw = dict(channel_probs_x=probs[0], channel_probs_y=probs[1], channel_probs_z=probs[2], **BP4_KW)
    err, sx, sz = P.sample(code.hx, code.hz, *probs, shots, SEED, first)
    dec = O.bp4_osd(code.hx, code.hz, **kw)
    est, osd0 = np.zeros_like(err), np.zeros_like(err)
    words, words0 = np.zeros(shots, np.int32), np.zeros(shots, np.int32)
    for i in range(shots):
        est[i] = dec.decode(sx[i], sz[i])
        osd0[i, 0], osd0[i, 1] = dec.osd0_decoding_x, dec.osd0_decoding_z
        for e, w in ((est[i], words), (osd0[i], words0)):
            dx, dz = e[0] ^ err[i, 0], e[1] ^ err[i, 1]
            residual = bool(((code.hz.astype(np.int64) @ dx) % 2).any() or ((code.hx.astype(np.int64) @ dz) % 2).any())
            w[i] = int(P.reference_logical_error(dx, dz, hx_perp, hz_perp)) | (2 if residual else 0) | (0 if dec.converge else 4)
    for a in (err, sx, sz, est, osd0, words, words0):
        a.setflags(write=False)
    return dict(kw=kw, shots=shots, first=first, err=err, sx=sx, sz=sz, est=est, osd0=osd0, words=words, words0=words0)


@pytest.mark.parametrize("case", ["depolarizing", "biased"])
def test_bp4_experiment_equals_the_host_loop(case):
    """[[72,12,6]], bp4_osd(max_iter=32, 0.625, osd_cs, 10): depolarizing p = 0.06, 2048 shots from shot 0 (the loop gives 83 logical
    errors, 95 with OSD-0, 68 not converged) and biased per-qubit noise, 1024 shots from shot 2^32 - 500."""
    from slidingwindowdecoder_amd import CodeCapacityExperiment
    h = _bp4_host_loop(case)
    shots, first = h["shots"], h["first"]
    exp = CodeCapacityExperiment(_bb(72), decoder="bp4_osd", method="decode", **h["kw"])
    b = exp.run_batch(shots, seed=SEED, first_shot=first, osd0=True)
    for key in ("err", "sx", "sz", "est", "osd0"):
        assert (b[key] == h[key]).all(), key
    assert (b["result"] == h["words"]).all() and (b["result_osd0"] == (h["words0"] & 3)).all()
    assert (((b["stats"][:, 0] & 0x100) == 0) == ((h["words"] & 4) != 0)).all()
    r = exp.run(shots, seed=SEED, first_shot=first, osd0=True)
    n_log, n_log0, n_nc = int((h["words"] & 1).sum()), int((h["words0"] & 1).sum()), int((h["words"] & 4 != 0).sum())
    print(f"{case}: {n_log} logical errors, {n_log0} with OSD-0, {n_nc} not converged of {shots}")
    assert (r.shots, r.logical_errors, r.osd0_logical_errors, r.not_converged) == (shots, n_log, n_log0, n_nc)
    assert r.residual_syndromes == int((h["words"] & 2 != 0).sum()) == 0  # (the OSD always reproduces the syndrome)
    assert 0 < r.logical_errors < shots
    assert r.ler == n_log / shots and r.ler_stderr == pytest.approx(np.sqrt(r.ler * (1 - r.ler) / shots), rel=1e-12)
    if case == "depolarizing":
        assert (n_log, n_log0, n_nc) == (83, 95, 68)
    assert exp.run(shots, seed=SEED, first_shot=first).osd0_logical_errors is None


def test_run_does_not_depend_on_batching_or_lanes():
    from slidingwindowdecoder_amd import CodeCapacityExperiment
    pr = np.full(72, 0.06 / 3)
    exp = CodeCapacityExperiment((_bb(72).hx, _bb(72).hz), channel_probs_x=pr, channel_probs_y=pr, channel_probs_z=pr, **BP4_KW)
    a = exp.run(3000, batch=1024, lanes=2, osd0=True)
    b = exp.run(3000, batch=3000, lanes=1, osd0=True)
    assert a == b and a.shots == 3000 and 0 < a.logical_errors < 3000
    for f in ("shots", "logical_errors", "residual_syndromes", "not_converged", "osd0_logical_errors", "ler", "ler_stderr"):
        assert getattr(a, f) == getattr(b, f), f
    # the first 2048 shots of the stream are the end-to-end test's
    assert exp.run(2048, batch=500, lanes=3).logical_errors == 83
    # max_errors stops at batch granularity: whole rounds of lanes
    c = exp.run(3000, batch=256, lanes=2, max_errors=5)
    assert c.logical_errors >= 5 and c.shots % 512 == 0 and c.shots < 3000
    assert c == exp.run(c.shots, batch=c.shots, lanes=1)


@pytest.mark.parametrize("tag", ["bb72", "bb144"])
def test_camel_experiment_equals_the_host_loop(tag):
    """Misc.ipynb cell 8 on the recorded camel_decode configurations: every shot a newly built object, as on the device; a shot
    without a converged run returns zeros, so residual syndromes occur."""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import CodeCapacityExperiment
    from tests.test_oracle_bp4 import load_camel
    c = load_camel(tag)
    code, shots = c["code"], 512
    N = code.N
    hx_perp, hz_perp = _perps(N)
    kw = dict(channel_probs_x=c["px"], channel_probs_y=c["py"], channel_probs_z=c["pz"], **c["kw"])
    err, sx, sz = P.sample(code.hx, code.hz, c["px"], c["py"], c["pz"], shots, SEED)
    est, words = np.zeros_like(err), np.zeros(shots, np.int32)
    hx64, hz64 = code.hx.astype(np.int64), code.hz.astype(np.int64)
    for i in range(shots):
        dec = O.bp4_osd(code.hx, code.hz, **kw)
        est[i] = dec.camel_decode(sx[i], sz[i])
        dx, dz = est[i, 0] ^ err[i, 0], est[i, 1] ^ err[i, 1]
        residual = bool(((hz64 @ dx) % 2).any() or ((hx64 @ dz) % 2).any())
        words[i] = int(P.reference_logical_error(dx, dz, hx_perp, hz_perp)) | (2 if residual else 0) | (0 if dec.converge else 4)
    exp = CodeCapacityExperiment(code, decoder="bp4_osd", method="camel_decode", **kw)
    b = exp.run_batch(shots, seed=SEED)
    assert (b["err"] == err).all() and (b["est"] == est).all() and (b["result"] == words).all()
    r = exp.run(shots, batch=200, lanes=2, seed=SEED)
    n_res = int((words & 2 != 0).sum())
    print(f"camel {tag}: {int((words & 1).sum())} logical errors, {n_res} residual syndromes, {int((words & 4 != 0).sum())} not converged")
    assert n_res > 0 and r.residual_syndromes == n_res
    assert (r.shots, r.logical_errors, r.not_converged) == (shots, int((words & 1).sum()), int((words & 4 != 0).sum()))


@pytest.mark.parametrize("name", ["osd_window", "bpgdg_decoder"])
def test_binary_harness_equals_the_host_loop(name):
    """simulation.py's single-basis harness on [[72,12,6]] hx, iid p = 0.05, 1024 shots: errors of the DEM sampler's stream,
    syndrome err @ hx.T, the oracle class shot by shot, criterion ((e_hat + err) @ hz_perp.T % 2).any()."""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import CodeCapacityExperiment
    code, shots = _bb(72), 1024
    _, hz_perp = _perps(72)
    pr = np.full(72, 0.05)
    if name == "osd_window":
        kw = dict(channel_probs=pr, pre_max_iter=8, post_max_iter=100, ms_scaling_factor=0.625, osd_method="osd_cs", osd_order=10)
    else:
        kw = dict(channel_probs=pr, max_iter=8, ms_scaling_factor=0.625, max_iter_per_step=6, max_step=25, max_tree_depth=3,
                  max_side_depth=10, max_side_branch_step=10, gdg_factor=0.625, multi_thread=False)
    err = philox_ref.sample_faults(pr, shots, SEED)
    hx64 = code.hx.astype(np.int64)
    synd = ((err.astype(np.int64) @ hx64.T) % 2).astype(np.uint8)
    ora = getattr(O, name)(code.hx, **kw)
    est, words = np.zeros_like(err), np.zeros(shots, np.int32)
    if name == "osd_window":
        est[:], res = ora.decode_batch(synd)
        conv = res["converge"] != 0
    else:
        conv = np.zeros(shots, bool)
        for i in range(shots):
            est[i], conv[i] = ora.decode(synd[i]), bool(ora.converge)
    d = (est ^ err).astype(np.int64)
    logical = ((d @ hz_perp.T.astype(np.int64)) % 2).any(axis=1)
    residual = ((d @ hx64.T) % 2).any(axis=1)
    words = logical.astype(np.int32) | (residual.astype(np.int32) << 1) | ((~conv).astype(np.int32) << 2)
    exp = CodeCapacityExperiment(code, decoder=name, **kw)
    b = exp.run_batch(shots, seed=SEED)
    assert (b["err"] == err).all() and (b["sx"] == synd).all() and (b["est"] == est).all() and (b["result"] == words).all()
    r = exp.run(shots, batch=300, lanes=2, seed=SEED)
    print(f"{name}: {int(logical.sum())} logical errors, {int(residual.sum())} residual syndromes, {int((~conv).sum())} not converged")
    assert (r.shots, r.logical_errors, r.residual_syndromes, r.not_converged) == (shots, int(logical.sum()), int(residual.sum()), int((~conv).sum()))
    assert 0 < r.logical_errors < shots


def test_bad_arguments_raise_value_error():
    from slidingwindowdecoder_amd import CodeCapacityExperiment, PauliSampler
    code = _bb(72)
    pr = np.full(72, 0.02)
    with pytest.raises(ValueError):
        PauliSampler(code.hx, code.hz, pr[:71], pr, pr)
    with pytest.raises(ValueError):
        PauliSampler(code.hx, code.hz, np.full(72, 0.5), np.full(72, 0.3), np.full(72, 0.3))
    with pytest.raises(ValueError):
        PauliSampler(code.hx, code.hz, np.full(72, -0.1), pr, pr)
    with pytest.raises(ValueError):
        CodeCapacityExperiment(code, decoder="union_find", channel_probs_x=pr, channel_probs_y=pr, channel_probs_z=pr)
    exp = CodeCapacityExperiment(code, decoder="bp_history_decoder", channel_probs=pr, max_iter=8)
    with pytest.raises(ValueError):
        exp.run(10, osd0=True)
    assert exp.run(0).shots == 0
