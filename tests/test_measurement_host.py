"""The measurement map (``slidingwindowdecoder_amd.measurements``): which measurements every detector and observable is the parity
of, cut into round blocks for the device front end.  Expected values come from the op lists themselves, from a forward Pauli-frame
propagation written here, and from ``circuit.dem_from_ops`` -- never from the map's own inverse."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from slidingwindowdecoder_amd import circuit as ck


@functools.lru_cache(maxsize=None)
def case(tag):
    """(ops, detector rows per round, measurements per round, measurements of the final block)"""
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.shyps import shyps_memory_ops
    if tag == "shyps":
        return shyps_memory_ops(3, 0.002, 3), 21, 98, 49
    code, A, B = bb_code(72)
    return ck.bb_memory_ops(code, A, B, 0.004, 3, z_basis=(tag == "bb72z")), 36, 72, 72


def index_sets(ops, kind):
    out = []
    for o in ops:
        if o[0] == kind:
            idx, cnt = np.unique(np.asarray(list(o[1])), return_counts=True)
            out.append(set(int(i) for i in idx[cnt % 2 == 1]))
    return out


def csr_rows(a):
    a = sp.csr_matrix(a)
    return [set(int(j) for j in a.indices[a.indptr[i]:a.indptr[i + 1]]) for i in range(a.shape[0])]


@pytest.mark.parametrize("tag", ["bb72z", "bb72x", "shyps"])
def test_map_rows_are_the_index_sets_of_the_op_list(tag):
    from slidingwindowdecoder_amd.measurements import measurement_map
    ops, h, mpr, fin = case(tag)
    mm = measurement_map(ops, h)
    assert mm.num_meas == 3 * mpr + fin and mm.det.shape == (4 * h, mm.num_meas) and mm.obs.shape[1] == mm.num_meas
    assert csr_rows(mm.det) == index_sets(ops, ck.DETECTOR)
    assert csr_rows(mm.obs) == index_sets(ops, ck.OBSERVABLE)
    assert all(len(r) for r in csr_rows(mm.det)) and all(len(r) for r in csr_rows(mm.obs))
    blk = mm.blocks()
    assert (blk.rounds, blk.meas_per_round, blk.meas_final, blk.n_half) == (3, mpr, fin, h)
    assert blk.head.shape == blk.body.shape == (h, 2 * mpr) and blk.tail.shape == (h, mpr + fin)
    assert blk.obs_tail.shape == (mm.obs.shape[0], mpr + fin)
    # the templates, moved back to their rounds, are the map
    want = index_sets(ops, ck.DETECTOR)
    for r, t in ((0, blk.head), (1, blk.body), (2, blk.body), (3, blk.tail)):
        assert [set(j + (r - 1) * mpr for j in row) for row in csr_rows(t)] == want[r * h:(r + 1) * h]
    assert [set(j + 2 * mpr for j in row) for row in csr_rows(blk.obs_tail)] == index_sets(ops, ck.OBSERVABLE)
    if tag == "shyps":  # parities of several gauge outcomes of two rounds
        assert min(len(r) for r in csr_rows(blk.body)) > 2


def test_phenomenological_map_of_the_repetition_code():
    """rep_code(5): 4 syndrome bits per round, 5 data bits; d_0 = s_0, d_t = s_t ^ s_{t-1}, d_R = H data ^ s_{R-1}, obs = L data"""
    from slidingwindowdecoder_amd.codes import rep_code
    from slidingwindowdecoder_amd.measurements import detectors_from_measurements_host, phenomenological_measurement_map
    H, L, R = rep_code(5), np.ones((1, 5), np.uint8), 5
    mm = phenomenological_measurement_map(H, L, R)
    assert mm.num_meas == 4 * R + 5 and mm.det.shape == (4 * (R + 1), 25) and mm.obs.shape == (1, 25)
    rows = csr_rows(mm.det)
    for t in range(R):
        for i in range(4):
            assert rows[4 * t + i] == ({4 * t + i} | ({4 * (t - 1) + i} if t else set()))
    for i in range(4):
        assert rows[4 * R + i] == {4 * R + int(j) for j in np.flatnonzero(H[i])} | {4 * (R - 1) + i}
    assert csr_rows(mm.obs) == [set(range(20, 25))]
    blk = mm.blocks()
    assert (blk.rounds, blk.meas_per_round, blk.meas_final, blk.n_half) == (5, 4, 5, 4)
    # against the experiment the model describes: accumulate faults, read syndromes, difference them
    from slidingwindowdecoder_amd.phenomenological import phenomenological_dem, simulate_host
    rng = np.random.default_rng(2)
    dem = phenomenological_dem(H, L, 0.1, R)
    faults = (rng.random((50, dem.chk.shape[1])) < 0.1).astype(np.uint8)
    det, obs = simulate_host(H, L, faults, R)
    err, meas = np.zeros((50, 5), np.int64), []
    for t in range(R + 1):
        err ^= faults[:, 9 * t:9 * t + 5]
        meas.append((err @ H.T) % 2 ^ faults[:, 9 * t + 5:9 * t + 9] if t < R else err)
    got = detectors_from_measurements_host(mm, np.concatenate(meas, axis=1))
    assert np.array_equal(got[0], det) and np.array_equal(got[1], obs) and det.any() and obs.any()
    # the record of a two-basis model: exact final syndromes, then the logical values
    mb = phenomenological_measurement_map(H, L, R, exact_final_syndrome=True)
    assert mb.num_meas == 4 * R + 4 + 1 and csr_rows(mb.obs) == [{24}]
    assert csr_rows(mb.det)[4 * R:] == [{20 + i, 16 + i} for i in range(4)]


def propagate(ops, site, pauli):
    """Forward, noiseless Pauli-frame propagation: the fault ``pauli`` -- ((x, z) per qubit of the noise op) -- is injected at op
    ``site``; returns the set of measurements it flips.  CX copies X forward and Z backward, H swaps, a Z-basis measurement is
    flipped by X and an X-basis one by Z, resets clear the frame."""
    fx, fz, flips = {}, {}, set()
    for q, (x, z) in zip(ops[site][1:], pauli):
        fx[q], fz[q] = x, z
    for o in ops[site + 1:]:
        k = o[0]
        if k == ck.CX:
            c, t = o[1], o[2]
            if fx.get(c):
                fx[t] = fx.get(t, 0) ^ 1
            if fz.get(t):
                fz[c] = fz.get(c, 0) ^ 1
        elif k == ck.H:
            fx[o[1]], fz[o[1]] = fz.get(o[1], 0), fx.get(o[1], 0)
        elif k in (ck.M, ck.MR):
            if fx.get(o[1]):
                flips.add(o[2])
        elif k in (ck.MX, ck.MRX):
            if fz.get(o[1]):
                flips.add(o[2])
        if k in (ck.MR, ck.MRX, ck.R, ck.RX):
            fx[o[1]] = fz[o[1]] = 0
    return flips


_COMPONENTS = {ck.XERR: [((1, 0),)], ck.ZERR: [((0, 1),)], ck.DEP1: [((1, 0),), ((1, 1),), ((0, 1),)],
               ck.DEP2: [(a, b) for a in ((0, 0), (1, 0), (1, 1), (0, 1)) for b in ((0, 0), (1, 0), (1, 1), (0, 1)) if a != (0, 0) or b != (0, 0)]}


@pytest.mark.parametrize("tag,samples", [("bb72z", 200), ("shyps", 100)])
def test_a_single_faults_measurement_flips_give_its_dem_column(tag, samples):
    """ties the map to the DEM without the synthesiser: one X, Y or Z at a noise site flips the measurements ``f``; ``det f`` and
    ``obs f`` must be the symptom and observable mask of a column ``dem_from_ops`` emits (a fault nothing sees has no column)"""
    from slidingwindowdecoder_amd.measurements import measurement_map
    ops, h, _, _ = case(tag)
    mm = measurement_map(ops, h)
    dem = ck.dem_from_ops(ops)
    chk, obs = sp.csc_matrix(dem.chk), sp.csc_matrix(dem.obs)
    columns = {(frozenset(chk.indices[chk.indptr[j]:chk.indptr[j + 1]].tolist()), frozenset(obs.indices[obs.indptr[j]:obs.indptr[j + 1]].tolist()))
               for j in range(chk.shape[1])}
    assert len(columns) == chk.shape[1]
    sites = [i for i, o in enumerate(ops) if o[0] in _COMPONENTS]
    rng = np.random.default_rng(11)
    det_rows, obs_rows = csr_rows(mm.det), csr_rows(mm.obs)
    seen, rounds_hit = 0, set()
    for site in rng.choice(sites, samples, replace=False):
        comps = _COMPONENTS[ops[site][0]]
        f = propagate(ops, int(site), comps[rng.integers(len(comps))])
        sym = frozenset(d for d, row in enumerate(det_rows) if len(row & f) & 1)
        mask = frozenset(k for k, row in enumerate(obs_rows) if len(row & f) & 1)
        if not sym and not mask:
            continue  # invisible to this basis: dem_from_ops emits nothing for it
        assert (sym, mask) in columns, f"op {site} {ops[site]}"
        seen += 1
        rounds_hit |= {d // h for d in sym}
    assert seen >= samples // 3 and rounds_hit == {0, 1, 2, 3}


@pytest.mark.parametrize("tag", ["bb72z", "bb72x", "shyps"])
def test_synthesiser_round_trip(tag):
    from slidingwindowdecoder_amd.measurements import detectors_from_measurements_host, measurement_map, synthesize_measurements_host
    from slidingwindowdecoder_amd.windows import sample_dem
    ops, h, mpr, _ = case(tag)
    mm = measurement_map(ops, h)
    dem = ck.dem_from_ops(ops)
    det, flips, _ = sample_dem(dem.chk, dem.obs, dem.priors * 4, 64, seed=5)
    assert det.any() and flips.any()
    a = synthesize_measurements_host(mm, det, flips, np.random.default_rng(1))
    b = synthesize_measurements_host(mm, det, flips, np.random.default_rng(2))
    assert a.shape == (64, mm.num_meas) and a.dtype == np.uint8 and a.max() == 1
    assert not np.array_equal(a, b)
    for rec in (a, b):
        d, f = detectors_from_measurements_host(mm, rec)
        assert np.array_equal(d, det) and np.array_equal(f, flips)
    if tag == "bb72z":  # the X ancillas, which no z-basis detector reads, come out as random bits
        assert a[:, 36:72].any() and not a[:, 36:72].all()
    # detectors no record has: hz (hx) has dependent rows, and one flipped final detector inside a dependency violates it
    if tag != "shyps":
        from slidingwindowdecoder_amd import gf2
        from slidingwindowdecoder_amd.codes import bb_code
        code = bb_code(72)[0]
        dep = gf2.nullspace(np.asarray(code.hz if tag == "bb72z" else code.hx).T)
        assert dep.shape[0] > 0
        bad = det.copy()
        bad[:, 3 * h + int(np.flatnonzero(dep[0])[0])] ^= 1
        with pytest.raises(ValueError, match="no measurement record has these detectors"):
            synthesize_measurements_host(mm, bad, flips, np.random.default_rng(1))


def test_blocks_refusals():
    from slidingwindowdecoder_amd.measurements import MeasurementMap, measurement_map
    ops, h, mpr, fin = case("bb72z")
    mm = measurement_map(ops, h)
    # a detector of round 2 that also reads round 0
    det = sp.lil_matrix(mm.det)
    det[2 * h + 5, 7] = 1
    with pytest.raises(ValueError, match=rf"detector {2 * h + 5} of round 2 reads measurement 7 of round 0"):
        MeasurementMap(sp.csr_matrix(det), mm.obs, mm.num_meas).blocks(h)
    # a body round that differs: round 2's detector 3 reads one more measurement of its own round
    det = sp.lil_matrix(mm.det)
    det[2 * h + 3, 2 * mpr + 40] = 1
    with pytest.raises(ValueError, match="round 2 is not a translate of round 1"):
        MeasurementMap(sp.csr_matrix(det), mm.obs, mm.num_meas).blocks(h)
    # an observable that reaches back beyond the last syndrome round
    obs = sp.lil_matrix(mm.obs)
    obs[0, 3] = 1
    with pytest.raises(ValueError, match="observable 0 of round 3 reads measurement 3 of round 0"):
        MeasurementMap(mm.det, sp.csr_matrix(obs), mm.num_meas).blocks(h)
    with pytest.raises(ValueError, match="144 detector rows are not"):
        mm.blocks(35)
    with pytest.raises(ValueError, match="n_half"):
        measurement_map(ops).blocks()


def test_front_end_create_checks_its_templates_before_it_needs_a_device():
    """swd_frontend_create refuses a head template with an entry in its previous-round half, a template of another shape and a
    record longer than a launch stages -- all before the device is looked for, so the messages come back on a CPU-only host too"""
    import ctypes as C
    import os
    from slidingwindowdecoder_amd import _lib
    from slidingwindowdecoder_amd.decoders import _template_desc
    from slidingwindowdecoder_amd.measurements import measurement_map
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libswd_hip.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    ops, h, mpr, fin = case("bb72z")
    blk = measurement_map(ops, h).blocks()

    def create(head, body, tail, obs, mpr_=mpr, fin_=fin, h_=h):
        keep = []
        d = [_template_desc(t, keep) for t in (head, body, tail, obs)]
        return L.swd_frontend_create(C.byref(d[0]), C.byref(d[1]), C.byref(d[2]), C.byref(d[3]), mpr_, fin_, h_, 4, 0)
    assert not create(blk.body, blk.body, blk.tail, blk.obs_tail)
    assert "head template: row 0 reads column 0 outside [72, 144)" in _lib.last_error()
    assert not create(blk.head, blk.tail[:, :2 * mpr], blk.tail[:h - 1], blk.obs_tail)
    assert "the tail template is 35 x 144, expected 36 x 144" in _lib.last_error()
    assert not create(blk.head, blk.body, blk.tail, blk.obs_tail, fin_=40000)
    assert "exceed the 32768 bytes a launch stages" in _lib.last_error()
    # a descriptor whose row_ptr runs past its entries
    keep = []
    d = [_template_desc(t, keep) for t in (blk.head, blk.body, blk.tail, blk.obs_tail)]
    d[1].nnz -= 1
    assert not L.swd_frontend_create(C.byref(d[0]), C.byref(d[1]), C.byref(d[2]), C.byref(d[3]), mpr, fin, h, 4, 0)
    assert "body template: row_ptr ends at 72, the descriptor has 71 entries" in _lib.last_error()
    assert L.swd_frontend_push_dev(None, 0, None, 0, 0, None, 0, None, None) == -1 and "null front end" in _lib.last_error()
