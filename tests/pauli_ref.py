"""Numpy restatement of the device Pauli sampler's random stream (include/swd.h, swd_pauli_sampler_*): Philox4x32-10 keyed by
the seed, counter (shot lo, shot hi, qubit // 4, 1); output word qubit % 4 = u decides the qubit: u < tx -> X, tx <= u < txy -> Y,
txy <= u < txyz -> Z, else I, with tx, txy, txyz = round(px 2^32), round((px + py) 2^32), round(((px + py) + pz) 2^32), each
floor(v 2^32 + 0.5) clamped to 2^32 - 1.  Also the reference's logical-error criterion.  Test infrastructure only."""
import numpy as np

from tests.philox_ref import philox4x32_10


def thresholds(px, py, pz):
    px, py, pz = (np.asarray(v, np.float64) for v in (px, py, pz))
    rnd = lambda v: np.minimum(np.floor(v * 4294967296.0 + 0.5), 4294967295.0).astype(np.uint64)  # noqa: E731
    return rnd(px), rnd(px + py), rnd((px + py) + pz)


def sample_paulis(px, py, pz, shots, seed, first_shot=0):
    """-> uint8 [shots, 2, n]: row 0 the X string (X or Y on the qubit), row 1 the Z string (Y or Z)."""
    n = len(px)
    tx, txy, txyz = thresholds(px, py, pz)
    shot = ((np.arange(shots, dtype=np.uint64) + np.uint64(first_shot)) & np.uint64(0xFFFFFFFFFFFFFFFF))[:, None]
    grp = np.arange((n + 3) // 4, dtype=np.uint64)[None, :]
    u = philox4x32_10(shot & np.uint64(0xFFFFFFFF), shot >> np.uint64(32), grp, np.uint64(1), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = u.reshape(shots, -1)[:, :n]
    err_x = u < txy[None, :]
    err_z = (u >= tx[None, :]) & (u < txyz[None, :])
    return np.stack([err_x, err_z], axis=1).astype(np.uint8)


def sample(Hx, Hz, px, py, pz, shots, seed, first_shot=0):
    """-> err [shots, 2, n], sx = Hx err_z [shots, mx], sz = Hz err_x [shots, mz] (Misc.ipynb cell 2)."""
    err = sample_paulis(px, py, pz, shots, seed, first_shot)
    Hx, Hz = np.asarray(Hx, np.int64), np.asarray(Hz, np.int64)
    sx = ((err[:, 1].astype(np.int64) @ Hx.T) % 2).astype(np.uint8)
    sz = ((err[:, 0].astype(np.int64) @ Hz.T) % 2).astype(np.uint8)
    return err, sx, sz


def reference_logical_error(dx, dz, hx_perp, hz_perp):
    """Misc.ipynb's criterion on one shot's difference strings: ((dz @ hz_perp.T) % 2).any() or ((dx @ hx_perp.T) % 2).any()."""
    return bool(((dz.astype(np.int64) @ hz_perp.T.astype(np.int64)) % 2).any() or ((dx.astype(np.int64) @ hx_perp.T.astype(np.int64)) % 2).any())
