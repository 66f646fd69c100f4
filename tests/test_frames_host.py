"""The Pauli-frame rule on the host (``frames.simulate_frames_host``, the statement the device circuit sampler is held against in
tests/test_gpu_circuit_sampler.py): the FORWARD propagation of every single fault of an op list gives exactly the columns and
priors that ``circuit.dem_from_ops`` derives BACKWARDS from the same list; a noiseless run with random frames has random records
and no detector; ``compile_ops`` refuses malformed lists; tests/frame_ref.py draws the documented Philox words.
Circuits: [[72,12,6]] z- and x-basis with 3 rounds, SHYPS r = 3 with 2 rounds."""
import functools

import numpy as np
import pytest

from tests import frame_ref
from tests.philox_ref import philox4x32_10

CIRCUITS = ["bb72z", "bb72x", "shyps3"]


@functools.lru_cache(maxsize=None)
def circuit_ops(tag, p=0.01):
    from slidingwindowdecoder_amd.circuit import bb_memory_ops
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.shyps import shyps_memory_ops
    if tag == "shyps3":
        return shyps_memory_ops(3, p, 2)
    code, A, B = bb_code(72)
    return bb_memory_ops(code, A, B, p, 3, z_basis=tag == "bb72z")


def symptoms(ops, codes=None, rbits=None):
    """-> uint8 [shots, num_det + num_obs] of a host run, and its record"""
    from slidingwindowdecoder_amd import measurements as ms
    from slidingwindowdecoder_amd.frames import simulate_frames_host
    rec = simulate_frames_host(ops, codes, rbits)
    det, obs = ms.detectors_from_measurements_host(ms.measurement_map(ops), rec)
    return np.concatenate([det, obs], axis=1), rec


@pytest.mark.parametrize("tag", CIRCUITS)
def test_forward_single_faults_equal_the_backward_dem(tag):
    from slidingwindowdecoder_amd.circuit import dem_from_ops
    from slidingwindowdecoder_amd.frames import compile_ops, single_faults
    ops = circuit_ops(tag)
    prog = compile_ops(ops)
    slot, code, prob = single_faults(prog)
    folded = {}
    for lo in range(0, len(slot), 8192):  # one fault per "shot", randomisation off
        n = min(8192, len(slot) - lo)
        codes = np.zeros((n, prog.num_noise), np.uint8)
        codes[np.arange(n), slot[lo:lo + n]] = code[lo:lo + n]
        sym, _ = symptoms(ops, codes)
        keys = np.packbits(sym, axis=1)
        for i in np.flatnonzero(sym.any(axis=1)):
            k, q = keys[i].tobytes(), prob[lo + i]
            pp = folded.get(k)
            folded[k] = q if pp is None else pp * (1.0 - q) + q * (1.0 - pp)
    dem = dem_from_ops(ops)
    cols = np.packbits(np.concatenate([dem.chk.toarray(), dem.obs.toarray()], axis=0).T.astype(np.uint8), axis=1)
    want = {cols[j].tobytes(): dem.priors[j] for j in range(cols.shape[0])}
    assert len(want) == cols.shape[0] == {"bb72z": 1152, "bb72x": 1152, "shyps3": 441}[tag]
    assert set(folded) == set(want)
    rel = max(abs(folded[k] - want[k]) / want[k] for k in want)
    print(f"{tag}: {len(slot)} single faults, {len(want)} columns, priors differ by {rel:.3g} relative at most")
    assert rel <= 1e-12  # a fold of a few hundred terms in another order


@pytest.mark.parametrize("tag", CIRCUITS)
def test_noiseless_run_with_random_frames(tag):
    from slidingwindowdecoder_amd.frames import compile_ops
    ops = circuit_ops(tag, 0.0)
    prog = compile_ops(ops)
    assert not prog.thr.any()
    rbits = np.random.default_rng(3).integers(0, 2, (64, prog.num_rand)).astype(np.uint8)
    sym, rec = symptoms(ops, None, rbits)
    assert not sym.any()
    assert rec.any()
    if tag == "bb72z":  # a round measures 36 Z ancillas, then 36 X ancillas: the X outcomes are random and repeat
        xanc = [rec[:, 72 * r + 36:72 * r + 72] for r in range(3)]
        assert np.array_equal(xanc[0], xanc[1]) and np.array_equal(xanc[1], xanc[2])
        assert 0.3 < xanc[0].mean() < 0.7
    # the frames of the noisy circuit at zero hits are the same run
    assert np.array_equal(symptoms(circuit_ops(tag), np.zeros((64, prog.num_noise), np.uint8), rbits)[1], rec)


@pytest.mark.parametrize("tag", CIRCUITS)
def test_detectors_do_not_depend_on_randomisation(tag):
    """the noisy circuits: the records differ between the two modes, the detectors and observables do not (the parities a memory
    circuit declares are deterministic; the hand-written list of tests/frame_ref.py declares arbitrary ones, so it is not here)"""
    from slidingwindowdecoder_amd import measurements as ms
    ops = circuit_ops(tag)
    on, off = frame_ref.records(ops, 96, 11, 5, True), frame_ref.records(ops, 96, 11, 5, False)
    mm = ms.measurement_map(ops)
    assert not np.array_equal(on, off)
    for a, b in zip(ms.detectors_from_measurements_host(mm, on), ms.detectors_from_measurements_host(mm, off)):
        assert np.array_equal(a, b) and a.any()


def test_compile_ops_validation_and_slots():
    from slidingwindowdecoder_amd.circuit import CX, DEP1, DEP2, DETECTOR, M, MR, MRX, MX, OBSERVABLE, R, RX, XERR, ZERR
    from slidingwindowdecoder_amd.frames import compile_ops
    good = [(R, 0), (R, 1), (XERR, 0, 0.25), (CX, 0, 1), (DEP2, 0, 1, 1.0), (MR, 1, 0), (DEP1, 0, 0.0), (M, 0, 1), (DETECTOR, (0, 1)), (OBSERVABLE, (1,))]
    prog = compile_ops(good)
    assert (len(prog), prog.num_qubits, prog.num_meas, prog.num_noise, prog.num_rand) == (8, 2, 2, 3, 4)
    assert prog.thr.dtype == np.uint32 and prog.thr.tolist() == [0, 0, 1 << 30, 0, 0xFFFFFFFF, 0, 0, 0]
    assert prog.noise_slot.tolist() == [-1, -1, 0, -1, 1, -1, 2, -1] and prog.rand_slot.tolist() == [0, 1, -1, -1, -1, 2, -1, 3]
    assert prog.meas.tolist() == [-1, -1, -1, -1, -1, 0, -1, 1] and prog.qb.tolist() == [-1, -1, -1, 1, 1, -1, -1, -1]

    def bad(ops, *words):
        with pytest.raises(ValueError) as e:
            compile_ops(ops)
        assert all(w in str(e.value) for w in words), str(e.value)
    bad(good[:4] + [(DEP2, 0, 1, 1.5)] + good[5:], "op 4 (DEP2)", "1.5")
    bad(good[:2] + [(XERR, 0, -1e-9)] + good[3:], "op 2 (XERR)")
    bad(good[:2] + [(XERR, 0, float("nan"))] + good[3:], "op 2 (XERR)")
    bad(good[:7] + [(M, 0, 0)] + good[8:], "op 7 (M)", "twice")
    bad(good[:7] + [(M, 0, 2)] + good[8:], "measurement index 1", "never written")
    bad(good[:8] + [(DETECTOR, (0, 2))], "op 8 (DETECTOR)", "measurement 2")
    bad(good[:9] + [(OBSERVABLE, (5,))], "op 9 (OBSERVABLE)", "measurement 5")
    bad(good[:3] + [(CX, 1, 1)] + good[4:], "op 3 (CX)")
    bad([(99, 0)], "op 0")
    # slots are numbered in list order: the noise ops and the ops that draw a randomisation bit, each counted from 0
    for tag in ("bb72z", "shyps3"):
        a = compile_ops(circuit_ops(tag))
        assert np.array_equal(a.noise_slot[a.noise_slot >= 0], np.arange(a.num_noise))
        assert np.array_equal(a.rand_slot[a.rand_slot >= 0], np.arange(a.num_rand))
        assert np.array_equal(a.noise_slot >= 0, np.isin(a.kind, [XERR, ZERR, DEP1, DEP2]))
        assert np.array_equal(a.rand_slot >= 0, np.isin(a.kind, [R, RX, M, MR, MX, MRX]))


def test_stream_restatement_draws_the_documented_words():
    seed, first = 0x0123456789ABCDEF, (1 << 32) - 2
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    u = frame_ref.noise_words(11, 4, seed, first)
    assert u.shape == (4, 11)
    for b, j in ((0, 0), (1, 3), (2, 4), (3, 10)):  # shot 2 is shot number 2^32: its high counter word is 1
        shot = first + b
        w = philox4x32_10(shot & 0xFFFFFFFF, shot >> 32, j // 4, 2, k0, k1)
        assert int(u[b, j]) == int(w[j % 4]), (b, j)
    assert (first + 2) >> 32 == 1
    bits = frame_ref.random_bits(300, 4, seed, first)
    assert bits.shape == (4, 300) and 0.3 < bits.mean() < 0.7
    for b, r in ((0, 0), (1, 31), (2, 32), (3, 127), (2, 128), (1, 299)):
        shot = first + b
        w = philox4x32_10(shot & 0xFFFFFFFF, shot >> 32, r // 128, 3, k0, k1)
        assert int(bits[b, r]) == (int(w[(r // 32) % 4]) >> (r % 32)) & 1, (b, r)
    # the four streams of one (seed, shot) are disjoint: counter word 3 tells them apart
    w = [philox4x32_10(7, 0, 0, tag, k0, k1).tolist() for tag in range(4)]
    assert len({tuple(x) for x in w}) == 4
    # Pauli codes: the word against the threshold, then the 64-bit products
    from slidingwindowdecoder_amd.circuit import DEP1, DEP2, XERR, ZERR
    from slidingwindowdecoder_amd.frames import compile_ops
    prog = compile_ops(frame_ref.hand_written_ops())
    codes = frame_ref.pauli_codes(prog, 200, seed, first)
    u = frame_ref.noise_words(prog.num_noise, 200, seed, first)
    ops, seen = np.flatnonzero(prog.noise_slot >= 0), {}
    for j, i in enumerate(ops):
        t, k = int(prog.thr[i]), int(prog.kind[i])
        mult = {XERR: 0, ZERR: 0, DEP1: 3, DEP2: 15}[k]
        want = [1 + (int(x) * mult) // t if int(x) < t else 0 for x in u[:, j]]
        assert codes[:, j].tolist() == want
        seen.setdefault(k, set()).update(want)
    assert seen == {XERR: {0, 1}, ZERR: {0, 1}, DEP1: set(range(4)), DEP2: set(range(16))}  # every Pauli of every channel occurs


def test_host_marginals_equal_the_dem():
    """32 768 shots of [[72,12,6]] z, 3 rounds, p = 0.01 through the host statement, seed and shots of the device test: every detector
    and observable frequency within 5 sigma of the DEM's exact marginal (a binomial bound), so that the device test can fail only
    through a device / host difference"""
    from slidingwindowdecoder_amd import measurements as ms
    ops = circuit_ops("bb72z")
    P = dem_marginals(ops)
    N = 32768
    rec = frame_ref.records(ops, N, 20240318, 0, True)
    det, obs = ms.detectors_from_measurements_host(ms.measurement_map(ops), rec)
    freq = np.concatenate([det, obs], axis=1).mean(axis=0)
    dev = np.abs(freq - P) / np.sqrt(P * (1.0 - P) / N)
    print(f"largest deviation {dev.max():.2f} sigma over {len(P)} rows")
    assert (P > 0).all() and dev.max() <= 5.0


def dem_marginals(ops):
    """P(row = 1) = (1 - prod(1 - 2 p_j)) / 2 over the DEM columns touching the row; detectors, then observables"""
    import scipy.sparse as sp
    from slidingwindowdecoder_amd.circuit import dem_from_ops
    dem = dem_from_ops(ops)
    rows = sp.vstack([dem.chk, dem.obs]).tocsr()
    logs = np.log1p(-2.0 * dem.priors)
    return 0.5 * (1.0 - np.exp(np.array([logs[rows.indices[rows.indptr[i]:rows.indptr[i + 1]]].sum() for i in range(rows.shape[0])])))
