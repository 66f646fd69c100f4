"""From raw measurement records to detector rows: the measurement map of an experiment.

A running experiment produces measurement outcomes, the sessions (``SlidingWindowDecoder.session`` / ``rolling_session``) take
detector rows.  The relation between the two is linear over GF(2) and already stated by the op lists of ``circuit.bb_memory_ops``
and ``shyps.shyps_memory_ops``: every ``DETECTOR`` and ``OBSERVABLE`` op carries the absolute measurement indices it is the parity
of.  This module exposes it:

* ``measurement_map(ops)`` -- ``det`` [num_det x num_meas] and ``obs`` [num_obs x num_meas] as CSR, rows in op order (the plans of
  ``windows.plan_windows`` permute columns only, so this is the row order of a session);
* ``phenomenological_measurement_map(H, logicals, num_repeat)`` -- the same for the models of ``phenomenological.py``, whose record
  is the raw syndrome of every round and the final data readout;
* ``MeasurementMap.blocks(n_half)`` -- the map cut into round blocks: three templates over ``[previous round | this block]`` (HEAD
  for round 0, BODY for the rounds after it, TAIL for the final block with the observables), which is what the device front end
  (``decoders.MeasurementFrontEnd``, C ABI swd_frontend_*) applies push by push;
* ``detectors_from_measurements_host`` -- the executable statement, dense numpy;
* ``synthesize_measurements_host`` -- a measurement record with given detectors and observable parities (tests and examples).

Host-side, runs once per experiment.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

from .circuit import DETECTOR, M, MR, MRX, MX, OBSERVABLE


def _csr_from_index_sets(sets, ncols):
    """rows = parities of the listed columns (an index listed twice cancels)"""
    indptr, indices = [0], []
    for s in sets:
        idx, cnt = np.unique(np.asarray(list(s), dtype=np.int64), return_counts=True)
        idx = idx[cnt % 2 == 1]
        if len(idx) and (idx[0] < 0 or idx[-1] >= ncols):
            raise ValueError(f"measurement index {int(idx[-1] if idx[-1] >= ncols else idx[0])} outside the record of {ncols} measurements")
        indices.append(idx)
        indptr.append(indptr[-1] + len(idx))
    ind = np.concatenate(indices) if indices else np.zeros(0, np.int64)
    return sp.csr_matrix((np.ones(len(ind), np.uint8), ind.astype(np.int32), np.asarray(indptr, np.int32)), shape=(len(sets), ncols))


@dataclass
class MeasurementBlocks:
    """``MeasurementMap.blocks``: the map as the device front end applies it.  ``head`` / ``body`` / ``tail`` are CSR
    [n_half x (meas_per_round + width)] over ``[previous round's measurements | this block's measurements]`` (width =
    ``meas_per_round``, for ``tail`` and ``obs_tail`` ``meas_final``); ``head`` has no entry in its previous-round half."""
    n_half: int
    rounds: int
    meas_per_round: int
    meas_final: int
    head: sp.csr_matrix
    body: sp.csr_matrix
    tail: sp.csr_matrix
    obs_tail: sp.csr_matrix


@dataclass
class MeasurementMap:
    det: sp.csr_matrix  # [num_det x num_meas]
    obs: sp.csr_matrix  # [num_obs x num_meas]
    num_meas: int
    meas_per_round: int | None = None  # known to the constructor (phenomenological maps); else ``blocks`` infers it
    n_half: int | None = None          # detector rows per round, where the constructor was told or knows

    def blocks(self, n_half=None, meas_per_round=None) -> MeasurementBlocks:
        """The round blocks of the map for detector blocks of ``n_half`` rows (default: the map's own): R = num_det / n_half - 1 syndrome rounds of
        ``meas_per_round`` measurements each, then the final block with the rest.  ``meas_per_round`` is taken from the argument,
        from the map, or from the distance between the latest measurement that the first detector of round 1 reads and that of
        round 0 (every detector's latest measurement lies in its own round).
        ValueError, naming the round: a detector that reads a measurement after its own round or more than one round back; body
        rounds that are not translates of round 1; fewer than two syndrome rounds (there is no body round to take a template from)."""
        if n_half is None and self.n_half is None:
            raise ValueError("n_half (detector rows per round) is needed: the map does not carry it")
        h = int(self.n_half if n_half is None else n_half)
        det = sp.csr_matrix(self.det)
        det.sort_indices()
        num_det = det.shape[0]
        if h <= 0 or num_det % h or num_det // h < 3:
            raise ValueError(f"{num_det} detector rows are not a head, a body and a final block of {h} rows each")
        R = num_det // h - 1
        row_sets = [det.indices[det.indptr[i]:det.indptr[i + 1]] for i in range(num_det)]
        for i, s in enumerate(row_sets):
            if len(s) == 0:
                raise ValueError(f"detector {i} (round {i // h}) reads no measurement")
        mpr = meas_per_round if meas_per_round is not None else self.meas_per_round
        if mpr is None:
            mpr = int(row_sets[h][-1]) - int(row_sets[0][-1])
        mpr = int(mpr)
        final = self.num_meas - R * mpr
        if mpr <= 0 or final <= 0:
            raise ValueError(f"{self.num_meas} measurements are not {R} rounds of {mpr} and a final block")

        def template(rows, r, width, what):
            """rows ``rows`` of a CSR over the record, as a CSR over [round r - 1 | block r]"""
            lo, hi = (r - 1) * mpr, r * mpr + width
            indptr, indices = [0], []
            for i in rows:
                s = row_sets[i] if what == "detector" else obs_sets[i]
                if len(s) and (s[0] < lo or s[-1] >= hi):
                    bad = int(s[0] if s[0] < lo else s[-1])
                    where = f"round {bad // mpr}" if bad < R * mpr else "the final block"
                    raise ValueError(f"{what} {i} of round {r} reads measurement {bad} of {where}: a {what} may read its own "
                                     f"round and the one before it only")
                indices.append(s - lo)
                indptr.append(indptr[-1] + len(s))
            ind = np.concatenate(indices) if indices else np.zeros(0, np.int64)
            return sp.csr_matrix((np.ones(len(ind), np.uint8), ind.astype(np.int32), np.asarray(indptr, np.int32)),
                                 shape=(len(indptr) - 1, mpr + width))

        obs = sp.csr_matrix(self.obs)
        obs.sort_indices()
        obs_sets = [obs.indices[obs.indptr[k]:obs.indptr[k + 1]] for k in range(obs.shape[0])]
        per_round = [template(range(r * h, (r + 1) * h), r, mpr, "detector") for r in range(R)]
        head, body = per_round[0], per_round[1]
        if head.indices.size and head.indices.min() < mpr:
            raise ValueError("a detector of round 0 reads a measurement before the record begins")
        for r in range(2, R):
            t = per_round[r]
            if not (np.array_equal(t.indptr, body.indptr) and np.array_equal(t.indices, body.indices)):
                raise ValueError(f"round {r} is not a translate of round 1: its detectors read other measurements of their two rounds")
        tail = template(range(R * h, (R + 1) * h), R, final, "detector")
        obs_tail = template(range(obs.shape[0]), R, final, "observable")
        return MeasurementBlocks(h, R, mpr, final, head, body, tail, obs_tail)


def measurement_map(ops, n_half=None) -> MeasurementMap:
    """The measurement map of an op list in ``circuit.py``'s op codes (``bb_memory_ops`` in either basis, ``shyps_memory_ops``):
    row d of ``det`` is the index set of the d-th ``DETECTOR`` op, row k of ``obs`` that of the k-th ``OBSERVABLE`` op.
    ``n_half``: the detector rows per round (``code.N // 2`` for the BB circuits, ``plan.n_half``), kept with the map for
    ``blocks`` and ``synthesize_measurements_host``; an op list does not mark its rounds."""
    num_meas = 0
    dets, obss = [], []
    for o in ops:
        if o[0] in (M, MR, MRX, MX):
            num_meas = max(num_meas, int(o[2]) + 1)
        elif o[0] == DETECTOR:
            dets.append(o[1])
        elif o[0] == OBSERVABLE:
            obss.append(o[1])
    return MeasurementMap(_csr_from_index_sets(dets, num_meas), _csr_from_index_sets(obss, num_meas), num_meas,
                          n_half=None if n_half is None else int(n_half))


def phenomenological_measurement_map(H, logicals, num_repeat, exact_final_syndrome=False) -> MeasurementMap:
    """The map of a single-basis phenomenological model (``phenomenological.phenomenological_dem``): the record is the raw syndrome
    ``s_t`` (m bits) of every round ``t < R``, then the n data bits of the final readout, and
    ``d_0 = s_0``, ``d_t = s_t ^ s_{t-1}``, ``d_R = H data ^ s_{R-1}``, ``obs = logicals data``.
    ``exact_final_syndrome=True`` is the record of a model whose final block cannot be a data readout -- ``basis="both"`` of
    ``css_phenomenological_dem``, where ``H`` is ``[hz; hx]`` and no readout gives both kinds of check: the final block is then the
    exact syndrome ``s_R`` (m bits) followed by the logical values (k bits; 2k for ``basis="both"``), ``d_R = s_R ^ s_{R-1}`` and
    observable j is bit j of the logical values; ``H`` and ``logicals`` are read for their shapes only."""
    H = np.asarray(H.toarray() if sp.issparse(H) else H).astype(np.int64) & 1
    L = np.asarray(logicals.toarray() if sp.issparse(logicals) else logicals).astype(np.int64) & 1
    m, n = H.shape
    R = int(num_repeat)
    if R < 1 or R != num_repeat:
        raise ValueError(f"num_repeat must be a positive integer, got {num_repeat!r}")
    if L.ndim != 2 or (L.shape[1] != n and not exact_final_syndrome):
        raise ValueError(f"logicals must be [k, {n}]")
    k = L.shape[0]
    dets = [[i] if t == 0 else [t * m + i, (t - 1) * m + i] for t in range(R) for i in range(m)]
    base = R * m
    if exact_final_syndrome:
        dets += [[base + i, base - m + i] for i in range(m)]
        obss = [[base + m + j] for j in range(k)]
        num_meas = base + m + k
    else:
        dets += [[base + int(j) for j in np.flatnonzero(H[i])] + [base - m + i] for i in range(m)]
        obss = [[base + int(j) for j in np.flatnonzero(L[j_])] for j_ in range(k)]
        num_meas = base + n
    return MeasurementMap(_csr_from_index_sets(dets, num_meas), _csr_from_index_sets(obss, num_meas), num_meas, meas_per_round=m, n_half=m)


def _as_record(mmap, meas):
    meas = np.asarray(meas)
    if meas.ndim != 2 or meas.shape[1] != mmap.num_meas:
        raise ValueError(f"meas must be [shots, {mmap.num_meas}], got {meas.shape}")
    return (meas != 0).astype(np.int32)


def detectors_from_measurements_host(mmap: MeasurementMap, meas):
    """meas [shots, num_meas] (0/1) -> (det uint8 [shots, num_det], raw_obs uint8 [shots, num_obs]): every detector and every raw
    observable as the parity of its measurements.  The statement the device front end is held against."""
    x = sp.csr_matrix(_as_record(mmap, meas))
    det = (x @ sp.csr_matrix(mmap.det).T.astype(np.int32)).toarray() % 2
    obs = (x @ sp.csr_matrix(mmap.obs).T.astype(np.int32)).toarray() % 2
    return det.astype(np.uint8), obs.astype(np.uint8)


def observable_masks(obs_bits) -> np.ndarray:
    """[shots, num_obs <= 32] bits -> uint32 [shots] masks, bit k = observable k: the form ``obs_flips`` and ``raw_obs`` travel in"""
    b = np.asarray(obs_bits).astype(np.uint32) & 1
    if b.ndim != 2 or b.shape[1] > 32:
        raise ValueError("obs_bits must be [shots, num_obs <= 32]")
    return (b << np.arange(b.shape[1], dtype=np.uint32)).sum(axis=1).astype(np.uint32)


class _Gf2System:
    """``A x = b`` over GF(2) for many right-hand sides: one elimination of ``A`` [r x c] (any rank) gives the row transform, the pivot
    columns and a basis of the kernel."""

    def __init__(self, A):
        A = (np.asarray(A).astype(np.uint8) & 1)
        r, c = A.shape
        aug = np.concatenate([A, np.identity(r, dtype=np.uint8)], axis=1)
        piv, row = [], 0
        for col in range(c):
            if row == r:
                break
            nz = np.flatnonzero(aug[row:, col])
            if len(nz) == 0:
                continue
            p = row + int(nz[0])
            if p != row:
                aug[[row, p]] = aug[[p, row]]
            others = np.flatnonzero(aug[:, col])
            others = others[others != row]
            aug[others] ^= aug[row]
            piv.append(col)
            row += 1
        self.rank, self.piv, self.ncols = row, np.asarray(piv, np.int64), c
        self.T = aug[:, c:].astype(np.int32)      # T A = reduced row echelon form
        rref = aug[:row, :c]
        free = np.setdiff1d(np.arange(c), self.piv)
        K = np.zeros((len(free), c), np.uint8)  # kernel: one vector per free column
        K[np.arange(len(free)), free] = 1
        if len(free) and row:
            K[:, self.piv] = rref[:, free].T
        self.kernel = K.astype(np.int32)

    def solve(self, b, rng, what):
        """b [shots, r] -> x [shots, c] with A x = b: the solution that is zero on the free columns, plus a random kernel vector"""
        y = (np.asarray(b).astype(np.int32) @ self.T.T) % 2
        if y[:, self.rank:].any():
            raise ValueError(f"{what}: no measurement record has these detectors (shot {int(np.flatnonzero(y[:, self.rank:].any(axis=1))[0])})")
        x = np.zeros((y.shape[0], self.ncols), np.int32)
        x[:, self.piv] = y[:, :self.rank]
        if len(self.kernel):
            x ^= (rng.integers(0, 2, (y.shape[0], len(self.kernel)), dtype=np.int32) @ self.kernel) % 2
        return x


def synthesize_measurements_host(mmap: MeasurementMap, det, obs_flips, rng, n_half=None) -> np.ndarray:
    """A measurement record [shots, num_meas] (uint8) whose detectors are ``det`` [shots, num_det] and whose raw observable parities
    are ``obs_flips`` [shots, num_obs] (bits) -- the inverse of ``detectors_from_measurements_host``, for tests and examples.
    Block by block (``mmap.blocks(n_half)``; ``n_half`` defaults to the map's own): a particular GF(2) solution of the block's rows given the round before, plus a random
    vector of the block's kernel drawn from ``rng`` (``numpy.random.Generator``) -- the outcomes no detector reads (the X ancillas
    of a z-basis BB run) and the freedom the detectors leave (the gauge outcomes of SHYPS) come out as random bits, which a front
    end must ignore.  Rank-deficient consistent systems are fine (``hz`` of the BB codes has dependent rows); ValueError when no
    record has the given detectors."""
    det = np.asarray(det).astype(np.int32) & 1
    flips = np.asarray(obs_flips).astype(np.int32) & 1
    blk = mmap.blocks(n_half)
    h, R, mpr, fin = blk.n_half, blk.rounds, blk.meas_per_round, blk.meas_final
    if det.ndim != 2 or det.shape[1] != (R + 1) * h or flips.shape != (det.shape[0], mmap.obs.shape[0]):
        raise ValueError(f"det must be [shots, {(R + 1) * h}] and obs_flips [shots, {mmap.obs.shape[0]}]")
    head, body = blk.head.toarray().astype(np.int32), blk.body.toarray().astype(np.int32)
    tail = np.concatenate([blk.tail.toarray(), blk.obs_tail.toarray()]).astype(np.int32)
    sys_head, sys_body, sys_tail = _Gf2System(head[:, mpr:]), _Gf2System(body[:, mpr:]), _Gf2System(tail[:, mpr:])
    out = np.zeros((det.shape[0], mmap.num_meas), np.uint8)
    prev = None
    for r in range(R):
        rhs = det[:, r * h:(r + 1) * h]
        if r:
            rhs = rhs ^ ((prev @ body[:, :mpr].T) % 2)
        prev = (sys_body if r else sys_head).solve(rhs, rng, f"round {r}")
        out[:, r * mpr:(r + 1) * mpr] = prev
    rhs = np.concatenate([det[:, R * h:], flips], axis=1) ^ ((prev @ tail[:, :mpr].T) % 2)
    out[:, R * mpr:] = sys_tail.solve(rhs, rng, "the final block")
    return out
