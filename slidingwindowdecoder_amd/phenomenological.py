"""Phenomenological-noise detector error models for any CSS code.

The rung between code capacity and circuit level: data qubits fail between rounds, syndrome bits are read wrongly, and no
circuit is needed -- a check matrix and the logicals it protects are the whole input.  The reference names the model where it
explains its windows (`Round Analysis.ipynb`: the identity block at the right edge of a window is the "virtual nodes" technique
of phenomenological noise); here it is a model of its own, handed to the same host planning (``windows.plan_windows`` with
``method=0``), samplers and window loops as a circuit-level model.

Single basis, ``R = num_repeat`` noisy rounds and a final exact one:

* round ``t = 0 .. R - 1`` draws a data fault ``e_t ~ Bernoulli(p)``; its syndrome is ``s_t = H (e_0 ^ .. ^ e_t) ^ u_t`` with
  the measurement fault ``u_t ~ Bernoulli(q)``;
* the final block ``t = R`` draws one more ``e_R`` (``final_data_noise``) and its syndrome ``s_R`` is exact: the data qubits are
  read out and the checks computed from them;
* detectors: ``d_0 = s_0``, ``d_t = s_t ^ s_{t-1}`` -- ``(R + 1) m`` rows in blocks of ``m``;
* observables: ``logicals (e_0 ^ .. ^ e_R)``.

Columns come in the order ``plan_windows`` permutes them into, so that its ``perm`` is the identity: for every ``t`` the ``n`` data
columns of round ``t`` (rows of ``H`` moved into block ``t``), then for ``t < R`` its ``m`` measurement columns (row ``i`` of blocks
``t`` and ``t + 1``).  A window of W blocks then ends, without any help, in the identity block with prior ``q`` on its last round:
the measurement columns of that round, cut at the window's last row.

Host-side, runs once per experiment.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from .circuit import DEM


def _binary(a, name):
    a = np.asarray(a.toarray() if sp.issparse(a) else a)
    if a.ndim != 2:
        raise ValueError(f"{name} must be a matrix, got shape {a.shape}")
    return (a.astype(np.int64) % 2).astype(np.uint8)


def _probabilities(v, count, name):
    v = np.asarray(v, dtype=np.float64)
    if v.ndim == 0:
        v = np.full(count, float(v))
    if v.shape != (count,):
        raise ValueError(f"{name} must be a scalar or an array of length {count}, got shape {v.shape}")
    if not ((v > 0.0) & (v <= 0.5)).all():
        raise ValueError(f"{name} must lie in (0, 0.5]")
    return v


def _rounds(num_repeat):
    if int(num_repeat) != num_repeat or int(num_repeat) < 1:
        raise ValueError(f"num_repeat must be a positive integer, got {num_repeat!r}")
    return int(num_repeat)


def _assemble(Hd, Ld, pd, qv, R, final_data_noise) -> DEM:
    """the model of data faults with rows ``Hd`` [m, nd], observables ``Ld`` [k, nd] and priors ``pd``, measurement priors ``qv`` [m]"""
    m, nd = Hd.shape
    Hd_c, Ld_c = sp.csc_matrix(Hd), sp.csc_matrix(Ld)
    zero_obs = sp.csc_matrix((Ld.shape[0], m), dtype=np.uint8)
    chk, obs, priors = [], [], []
    for t in range(R + 1):
        if t < R or final_data_noise:
            chk.append(sp.vstack([sp.csc_matrix((t * m, nd), dtype=np.uint8), Hd_c, sp.csc_matrix(((R - t) * m, nd), dtype=np.uint8)],
                                 format="csc"))
            obs.append(Ld_c)
            priors.append(pd)
        if t < R:
            i = np.arange(m)
            chk.append(sp.csc_matrix((np.ones(2 * m, np.uint8), (np.concatenate([t * m + i, (t + 1) * m + i]), np.concatenate([i, i]))),
                                     shape=((R + 1) * m, m)))
            obs.append(zero_obs)
            priors.append(qv)
    chk, obs = sp.hstack(chk, format="csc").astype(np.uint8), sp.hstack(obs, format="csc").astype(np.uint8)
    chk.sort_indices()
    obs.sort_indices()
    return DEM(chk, obs, np.concatenate(priors))


def phenomenological_dem(H, logicals, p, num_repeat, q=None, final_data_noise=True, other_checks=None) -> DEM:
    """The single-basis model of the module's docstring: ``H`` [m, n] the checks that see the faults, ``logicals`` [k, n] the
    logical operators those faults flip (``hz`` and ``lz`` for X faults), ``p`` the data and ``q`` the measurement fault
    probability -- scalars or arrays per qubit / per check, ``q=None`` means ``q = p``.  -> ``circuit.DEM`` with
    ``chk`` [(R + 1) m, R (n + m) + n], ``obs`` [k, same] (``logicals`` under every data block, zero under the measurement blocks)
    and ``priors``; without ``final_data_noise`` the last n columns are left out.
    Columns with equal symptoms are NOT merged (two qubits with the same column of ``H`` and the same logicals stay two columns
    with their own priors): every column is one fault of one round, which is what keeps the rounds translates of one another.
    ``other_checks``: the check matrix of the other kind (``hx`` beside ``hz``); logicals that do not commute with its rows are no
    logicals of the code.  ValueError: a probability outside (0, 0.5], shapes that do not fit, such logicals, a check without
    qubits or a qubit without checks (its faults would have no detector to be placed by)."""
    H, L = _binary(H, "H"), _binary(logicals, "logicals")
    m, n = H.shape
    R = _rounds(num_repeat)
    if m == 0 or n == 0:
        raise ValueError(f"H is empty: shape {H.shape}")
    if L.shape[1] != n:
        raise ValueError(f"logicals have {L.shape[1]} columns, H has {n}")
    if not H.any(axis=1).all():
        raise ValueError(f"check row {int(np.flatnonzero(~H.any(axis=1))[0])} of H is all zero")
    if not H.any(axis=0).all():
        raise ValueError(f"qubit {int(np.flatnonzero(~H.any(axis=0))[0])} is in no check of H")
    if other_checks is not None:
        other = _binary(other_checks, "other_checks")
        if other.shape[1] != n:
            raise ValueError(f"other_checks have {other.shape[1]} columns, H has {n}")
        if ((L.astype(np.int64) @ other.T.astype(np.int64)) % 2).any():
            raise ValueError("logicals do not commute with the rows of other_checks")
    pd = _probabilities(p, n, "p")
    qv = _probabilities(p if q is None else q, m, "q")
    return _assemble(H, L, pd, qv, R, bool(final_data_noise))


def css_fault_model(code, basis="z", noise="bitflip"):
    """``(Hd, Ld)``: the rows (detectors of one round) and the observables of every data fault of one round -- what
    ``css_phenomenological_dem`` repeats.  ``basis="z"``: ``hz``, ``lz``; ``"x"``: ``hx``, ``lx``;
    ``"both"``: the ``hz`` rows, then the ``hx`` rows, observables ``lz`` then ``lx``, data faults X (flip ``hz``, ``lz``), Z (flip
    ``hx``, ``lx``) and with ``noise="depolarizing"`` Y (both)."""
    if basis not in ("z", "x", "both"):
        raise ValueError("basis: 'z', 'x' or 'both'")
    if noise not in ("bitflip", "depolarizing"):
        raise ValueError("noise: 'bitflip' or 'depolarizing'")
    if noise == "depolarizing" and basis != "both":
        raise ValueError("depolarizing noise needs basis='both': a single basis sees bit flips only")
    hx, hz, lx, lz = (_binary(a, s) for a, s in ((code.hx, "hx"), (code.hz, "hz"), (code.lx, "lx"), (code.lz, "lz")))
    if basis == "z":
        return hz, lz
    if basis == "x":
        return hx, lx
    zx, zz = np.zeros_like(hx), np.zeros_like(hz)
    ox, oz = np.zeros_like(lx), np.zeros_like(lz)
    X = (np.vstack([hz, zx]), np.vstack([lz, ox]))
    Z = (np.vstack([zz, hx]), np.vstack([oz, lx]))
    parts = [X, Z] + ([(X[0] | Z[0], X[1] | Z[1])] if noise == "depolarizing" else [])
    return np.hstack([a for a, _ in parts]), np.hstack([b for _, b in parts])


def css_phenomenological_dem(code, p, num_repeat, q=None, basis="z", noise="bitflip", final_data_noise=True) -> DEM:
    """``phenomenological_dem`` of a ``codes.CSSCode``.  ``basis="z"``: the Z checks ``hz`` and the Z logicals ``lz``, which X faults
    flip; ``basis="x"`` the mirror image.  ``basis="both"`` stacks the two kinds of detector in every round -- the ``hz`` rows, then
    the ``hx`` rows, ``mz + mx`` detectors per round -- with the observables ``lz`` then ``lx`` (2k); ``noise="bitflip"``: independent X
    and Z data faults, each with prior p; ``noise="depolarizing"`` (``basis="both"`` only): X, Z and Y faults with prior p / 3 each, a
    Y fault carrying the rows and observables of both.  Data columns are ordered X, Z, Y within a round.  ``p``: scalar or per
    qubit; ``q``: scalar or per detector of a round (``None``: ``p``).  Equal symptoms are not merged."""
    Hd, Ld = css_fault_model(code, basis, noise)
    n, m = int(np.asarray(code.hx).shape[1]), Hd.shape[0]
    R = _rounds(num_repeat)
    pq = _probabilities(p, n, "p")
    qv = _probabilities(p if q is None else q, m, "q")
    if basis != "both":
        other = code.hx if basis == "z" else code.hz
        return phenomenological_dem(Hd, Ld, pq, R, qv, final_data_noise, other_checks=other)
    if not Hd.any(axis=1).all():
        raise ValueError(f"check row {int(np.flatnonzero(~Hd.any(axis=1))[0])} of [hz; hx] is all zero")
    if not Hd.any(axis=0).all():
        raise ValueError("a qubit is in no check of its kind")
    copies = Hd.shape[1] // n
    pd = np.concatenate([pq / 3.0 if noise == "depolarizing" else pq] * copies)
    return _assemble(Hd, Ld, pd, qv, R, bool(final_data_noise))


def simulate_host(H, logicals, faults, num_repeat, final_data_noise=True):
    """The model restated as the experiment it describes -- what the tests hold ``chk @ faults`` and ``obs @ faults`` against; it never
    touches ``chk``.  ``faults`` [shots, R (n + m) + n] (without ``final_data_noise``: R (n + m)) in the model's column order: per round
    the data faults, then the measurement faults.  The error accumulates, every round reads the syndrome of what has accumulated and
    flips the bits its measurement faults name, the final block reads it exactly, and consecutive syndromes are differenced.
    -> (det uint8 [shots, (R + 1) m], obs uint8 [shots, k]).  ``H`` and ``logicals`` may be any per-round fault model
    (``css_fault_model``): one column per kind of data fault."""
    H, L = _binary(H, "H").astype(np.int64), _binary(logicals, "logicals").astype(np.int64)
    m, n = H.shape
    R = _rounds(num_repeat)
    faults = np.asarray(faults).astype(np.int64) & 1
    if faults.ndim != 2 or faults.shape[1] != R * (n + m) + (n if final_data_noise else 0):
        raise ValueError(f"faults must be [shots, {R * (n + m) + (n if final_data_noise else 0)}], got {faults.shape}")
    shots = faults.shape[0]
    err = np.zeros((shots, n), np.int64)
    prev = np.zeros((shots, m), np.int64)
    det = np.zeros((shots, (R + 1) * m), np.uint8)
    for t in range(R + 1):
        c = t * (n + m)
        if t < R or final_data_noise:
            err ^= faults[:, c:c + n]
        synd = (err @ H.T) % 2
        if t < R:
            synd ^= faults[:, c + n:c + n + m]
        det[:, t * m:(t + 1) * m] = synd ^ prev
        prev = synd
    return det, ((err @ L.T) % 2).astype(np.uint8)


def experiment_model(code_or_matrices, p, num_repeat, q=None, basis="z", noise="bitflip"):
    """``(dem, detectors per round, default observable groups)`` for the experiments' ``phenomenological`` constructors: a
    ``codes.CSSCode`` goes through ``css_phenomenological_dem``, a pair ``(H, logicals)`` through ``phenomenological_dem`` (``basis`` and
    ``noise`` must then be left at their defaults).  The groups are ``{"z": the first k observables, "x": the last k}`` for
    ``basis="both"`` and None otherwise."""
    if hasattr(code_or_matrices, "hx") and hasattr(code_or_matrices, "hz"):
        code = code_or_matrices
        dem = css_phenomenological_dem(code, p, num_repeat, q, basis, noise)
        k = int(np.asarray(code.lz).shape[0])
        if basis == "both":
            if 2 * k > 32:
                raise ValueError(f"a memory experiment carries at most 32 observables per shot: basis='both' needs k <= 16, the code has k = {k}")
            return dem, int(code.hz.shape[0] + code.hx.shape[0]), {"z": (1 << k) - 1, "x": ((1 << k) - 1) << k}
        return dem, int((code.hz if basis == "z" else code.hx).shape[0]), None
    try:
        H, logicals = code_or_matrices
    except (TypeError, ValueError):
        raise ValueError("code_or_matrices: a CSSCode or a pair (H, logicals)") from None
    if basis != "z" or noise != "bitflip":
        raise ValueError("a pair (H, logicals) is one basis with bit flips: basis and noise belong to a CSSCode")
    dem = phenomenological_dem(H, logicals, p, num_repeat, q)
    return dem, int(dem.chk.shape[0] // (_rounds(num_repeat) + 1)), None
