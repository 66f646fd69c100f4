"""Pauli-frame simulation of the op lists of ``circuit.bb_memory_ops`` and ``shyps.shyps_memory_ops``: the FORWARD direction.

``circuit.dem_from_ops`` analyses an op list backwards into the detector error model; this module runs the same list forwards.  Per
shot and qubit two bits ``x``, ``z`` -- the Pauli frame against a noiseless run -- and a record of ``num_meas`` bits, ops in list
order; ``rnd`` is the op's randomisation bit (0 when randomisation is off):

    R q       x[q] = 0, z[q] = rnd                 RX q       z[q] = 0, x[q] = rnd
    H q       swap x[q], z[q]                      CX c,t     x[t] ^= x[c], z[c] ^= z[t]
    M q,i     rec[i] = x[q], z[q] = rnd            MX q,i     rec[i] = z[q], x[q] = rnd
    MR q,i    rec[i] = x[q], x[q] = 0, z[q] = rnd  MRX q,i    rec[i] = z[q], z[q] = 0, x[q] = rnd
    XERR q,p / ZERR q,p   flip x[q] / z[q]  iff  u < T(p)
    DEP1 q,p      iff u < T(p): Pauli 1 + (u * 3) // T(p) on q           (1 = X, 2 = Y, 3 = Z; Y flips both bits)
    DEP2 a,b,p    iff u < T(p): k = 1 + (u * 15) // T(p), Pauli k >> 2 on a and k & 3 on b   (0 = I)

with ``T(p) = min(floor(p 2^32 + 0.5), 2^32 - 1)`` (the DEM sampler's rule) and ``u`` the op's 32-bit noise word.  ``DETECTOR`` and
``OBSERVABLE`` are not executed: they are the measurement map (``measurements.measurement_map``).  Noise ops are numbered in list
order (noise slots), and so are the ops that consume ``rnd`` (randomisation slots); the device sampler (``decoders.CircuitSampler``,
csrc/swd_circuit.hip) draws ``u`` and ``rnd`` per (seed, shot number, slot) from Philox4x32-10 (include/swd.h), and executes exactly
this table.  With randomisation off the record is the flips against the all-zero noiseless record, which is a valid noiseless record
of these circuits; with it the record has the distribution of the circuit's outcomes.  Detectors and observables are the same in both.

* ``compile_ops(ops)`` -- the validated flat program the library takes;
* ``simulate_frames_host(ops, pauli_codes, random_bits)`` -- the executable statement, dense numpy over all shots, with the Pauli
  applied per noise slot and the randomisation bits given explicitly (no generator here: tests/frame_ref.py restates the streams);
* ``single_faults(program)`` -- every (noise slot, Pauli) with its component probability: the input of the forward check of
  ``dem_from_ops``.

Host-side, runs once per experiment.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .circuit import CX, DEP1, DEP2, DETECTOR, H, M, MR, MRX, MX, OBSERVABLE, R, RX, XERR, ZERR

OP_NAMES = {R: "R", RX: "RX", H: "H", CX: "CX", M: "M", MR: "MR", MRX: "MRX", XERR: "XERR", DEP1: "DEP1", DEP2: "DEP2",
            DETECTOR: "DETECTOR", OBSERVABLE: "OBSERVABLE", MX: "MX", ZERR: "ZERR"}
NOISE_OPS = (XERR, ZERR, DEP1, DEP2)
MEASURE_OPS = (M, MR, MX, MRX)
RANDOM_OPS = (R, RX) + MEASURE_OPS  # the ops that consume a randomisation bit
_TWO_QUBIT = (CX, DEP2)


def threshold(p) -> int:
    """T(p) = min(floor(p 2^32 + 0.5), 2^32 - 1)"""
    return int(min(np.floor(float(p) * 4294967296.0 + 0.5), 4294967295.0))


@dataclass
class FrameProgram:
    """The executable ops of a list (``DETECTOR`` / ``OBSERVABLE`` left out), one entry per op in list order.  ``qb`` is -1 for
    one-qubit ops, ``thr`` 0 and ``prob`` 0.0 for ops without noise, ``meas`` / ``noise_slot`` / ``rand_slot`` -1 where the op has
    none.  The kernel walks the list in order, so there are no layers; the slots are numbered in list order."""
    kind: np.ndarray        # int32
    qa: np.ndarray          # int32
    qb: np.ndarray          # int32
    thr: np.ndarray         # uint32
    prob: np.ndarray        # float64 (host only)
    meas: np.ndarray        # int32
    noise_slot: np.ndarray  # int32
    rand_slot: np.ndarray   # int32
    num_qubits: int
    num_meas: int
    num_noise: int
    num_rand: int

    def __len__(self):
        return len(self.kind)


def compile_ops(ops) -> FrameProgram:
    """ValueError, naming the op: an unknown op code, a negative qubit, a two-qubit op on one qubit, a probability outside [0, 1], a
    measurement index used twice; also for a gap in the measurement indices and for a ``DETECTOR`` / ``OBSERVABLE`` that reads a
    measurement that does not exist."""
    kind, qa, qb, thr, prob, meas, nslot, rslot = ([] for _ in range(8))
    seen, reads = {}, []
    nq = nn = nr = 0
    for i, o in enumerate(ops):
        k = o[0]
        if k not in OP_NAMES:
            raise ValueError(f"op {i}: unknown op code {k!r}")
        name = f"op {i} ({OP_NAMES[k]})"
        if k in (DETECTOR, OBSERVABLE):
            reads.append((name, [int(m) for m in o[1]]))
            continue
        a, b = int(o[1]), int(o[2]) if k in _TWO_QUBIT else -1
        if a < 0 or (k in _TWO_QUBIT and (b < 0 or a == b)):
            raise ValueError(f"{name}: qubits {a}, {b} are not two distinct qubits" if k in _TWO_QUBIT else f"{name}: qubit {a} is negative")
        nq = max(nq, a + 1, b + 1)
        p = 0.0
        if k in NOISE_OPS:
            p = float(o[-1])
            if not 0.0 <= p <= 1.0:  # (also refuses NaN)
                raise ValueError(f"{name}: probability {p!r} outside [0, 1]")
        mi = -1
        if k in MEASURE_OPS:
            mi = int(o[2])
            if mi < 0:
                raise ValueError(f"{name}: measurement index {mi} is negative")
            if mi in seen:
                raise ValueError(f"{name}: measurement index {mi} is used twice (first by {seen[mi]})")
            seen[mi] = name
        kind.append(k); qa.append(a); qb.append(b); thr.append(threshold(p)); prob.append(p); meas.append(mi)
        nslot.append(nn if k in NOISE_OPS else -1)
        rslot.append(nr if k in RANDOM_OPS else -1)
        nn += k in NOISE_OPS
        nr += k in RANDOM_OPS
    num_meas = len(seen)
    if seen and max(seen) != num_meas - 1:
        gap = next(m for m in range(num_meas) if m not in seen)
        raise ValueError(f"measurement index {gap} is never written: the {num_meas} measurements must be numbered 0 .. {num_meas - 1}")
    for name, idx in reads:
        for m in idx:
            if m < 0 or m >= num_meas:
                raise ValueError(f"{name} reads measurement {m}, the record has {num_meas}")
    i32 = lambda v: np.asarray(v, np.int32).reshape(-1)  # noqa: E731
    return FrameProgram(i32(kind), i32(qa), i32(qb), np.asarray(thr, np.uint32).reshape(-1), np.asarray(prob, np.float64).reshape(-1),
                        i32(meas), i32(nslot), i32(rslot), nq, num_meas, nn, nr)


def _as_program(ops) -> FrameProgram:
    return ops if isinstance(ops, FrameProgram) else compile_ops(ops)


def simulate_frames_host(ops, pauli_codes=None, random_bits=None) -> np.ndarray:
    """The table of the module docstring, all shots at once -> record uint8 [shots, num_meas].
    ``pauli_codes`` [shots, num_noise]: the Pauli a noise slot applies in a shot -- 0 none; ``XERR`` / ``ZERR``: non-zero = the flip;
    ``DEP1``: 1..3 (X, Y, Z); ``DEP2``: 1..15, ``k >> 2`` on the first qubit and ``k & 3`` on the second.  ``random_bits``
    [shots, num_rand]: the bit each randomisation slot draws; None: randomisation off.  One of the two may be None (no noise /
    no randomisation), not both: they give the number of shots."""
    prog = _as_program(ops)
    if pauli_codes is None and random_bits is None:
        raise ValueError("pauli_codes or random_bits must be given: they carry the number of shots")
    shots = len(pauli_codes) if pauli_codes is not None else len(random_bits)
    codes = np.zeros((shots, prog.num_noise), np.uint8) if pauli_codes is None else np.asarray(pauli_codes).astype(np.uint8)
    rbits = np.zeros((shots, prog.num_rand), np.uint8) if random_bits is None else (np.asarray(random_bits) != 0).astype(np.uint8)
    if codes.shape != (shots, prog.num_noise) or rbits.shape != (shots, prog.num_rand):
        raise ValueError(f"pauli_codes must be [shots, {prog.num_noise}] and random_bits [shots, {prog.num_rand}]")
    codes, rbits = np.ascontiguousarray(codes.T), np.ascontiguousarray(rbits.T)  # a slot's shots are contiguous
    x = np.zeros((prog.num_qubits, shots), np.uint8)
    z = np.zeros((prog.num_qubits, shots), np.uint8)
    rec = np.zeros((prog.num_meas, shots), np.uint8)
    px = np.array([0, 1, 1, 0], np.uint8)  # x / z part of Pauli 0..3 = I, X, Y, Z
    pz = np.array([0, 0, 1, 1], np.uint8)
    for j in range(len(prog)):
        k, a, b = int(prog.kind[j]), int(prog.qa[j]), int(prog.qb[j])
        rnd = rbits[prog.rand_slot[j]] if prog.rand_slot[j] >= 0 else None
        if k == CX:
            x[b] ^= x[a]
            z[a] ^= z[b]
        elif k == H:
            x[a], z[a] = z[a].copy(), x[a].copy()
        elif k == R:
            x[a], z[a] = 0, rnd
        elif k == RX:
            z[a], x[a] = 0, rnd
        elif k == M:
            rec[prog.meas[j]], z[a] = x[a], rnd
        elif k == MR:
            rec[prog.meas[j]] = x[a]
            x[a], z[a] = 0, rnd
        elif k == MX:
            rec[prog.meas[j]], x[a] = z[a], rnd
        elif k == MRX:
            rec[prog.meas[j]] = z[a]
            z[a], x[a] = 0, rnd
        else:
            c = codes[prog.noise_slot[j]]
            if k == XERR:
                x[a] ^= c != 0
            elif k == ZERR:
                z[a] ^= c != 0
            elif k == DEP1:
                x[a] ^= px[c & 3]
                z[a] ^= pz[c & 3]
            else:  # DEP2
                x[a] ^= px[(c >> 2) & 3]
                z[a] ^= pz[(c >> 2) & 3]
                x[b] ^= px[c & 3]
                z[b] ^= pz[c & 3]
    return np.ascontiguousarray(rec.T)


def single_faults(ops):
    """Every single fault of the circuit -> (slot int32 [F], code uint8 [F], prob float64 [F]): noise slot, the Pauli code it applies
    (``simulate_frames_host``) and the probability of that component as ``circuit.py`` states it -- ``XERR`` / ``ZERR``: p;
    ``DEP1``: (1 - sqrt(1 - 4p/3)) / 2 for each of X, Y, Z; ``DEP2``: (1 - (1 - 16p/15)^(1/8)) / 2 for each of the 15 Paulis."""
    prog = _as_program(ops)
    slot, code, prob = [], [], []
    for j in np.flatnonzero(prog.noise_slot >= 0):
        k, p = int(prog.kind[j]), float(prog.prob[j])
        if k == DEP1:
            n, q = 3, 0.5 * (1.0 - (1.0 - 4.0 * p / 3.0) ** 0.5)
        elif k == DEP2:
            n, q = 15, 0.5 * (1.0 - (1.0 - 16.0 * p / 15.0) ** 0.125)
        else:
            n, q = 1, p
        slot += [int(prog.noise_slot[j])] * n
        code += list(range(1, n + 1))
        prob += [q] * n
    return np.asarray(slot, np.int32), np.asarray(code, np.uint8), np.asarray(prob, np.float64)
