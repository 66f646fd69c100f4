"""Host-side facts the device code-capacity path rests on (no GPU): the restated Pauli stream has the rates it is asked for, and
the split accounting matrices [Hx; Lx] / [Hz; Lz] give the reference's ker(hz) / ker(hx) criterion."""
import numpy as np

from slidingwindowdecoder_amd import gf2
from slidingwindowdecoder_amd.codes import bb_code
from tests import pauli_ref as P


def test_restated_stream_has_the_requested_rates():
    """X / Y / Z frequencies of 20 000 shots within 5 sigma of px, py, pz, per class over all qubits and for single qubits with
    their own probabilities; the three classes are disjoint by construction (one word decides a qubit)."""
    shots, n = 20000, 12
    rng = np.random.default_rng(3)
    px, py, pz = rng.uniform(0.01, 0.2, n), rng.uniform(0.01, 0.2, n), rng.uniform(0.01, 0.2, n)
    px[0] = py[0] = pz[0] = 0.0
    px[1], py[1], pz[1] = 0.25, 0.25, 0.5
    err = P.sample_paulis(px, py, pz, shots, seed=20240318)
    ex, ez = err[:, 0].astype(bool), err[:, 1].astype(bool)
    got = {"x": (ex & ~ez), "y": (ex & ez), "z": (~ex & ez)}
    for name, p in (("x", px), ("y", py), ("z", pz)):
        f = got[name].mean(axis=0)
        sigma = np.sqrt(np.maximum(p * (1 - p), 1e-12) / shots)
        print(name, np.abs(f - p).max(), (np.abs(f - p) / sigma).max())
        assert (np.abs(f - p) <= 5 * sigma + 1e-12).all(), name
        tot, ptot = got[name].mean(), p.mean()
        assert abs(tot - ptot) <= 5 * np.sqrt((p * (1 - p)).sum() / shots) / n
    assert not err[:, :, 0].any()                      # all three probabilities 0: always I
    assert (ex[:, 1] | ez[:, 1]).mean() > 0.9999       # sum exactly 1: I only for the one word 2^32 - 1
    # another seed, another first shot: another stream
    assert (P.sample_paulis(px, py, pz, 64, seed=1) != err[:64]).any()
    assert (P.sample_paulis(px, py, pz, 64, seed=20240318, first_shot=64) == err[64:128]).all()


def test_split_matrices_give_the_reference_criterion():
    """[[72,12,6]]: 'some row of [Hx; Lx] has odd overlap with dz or some row of [Hz; Lz] with dx' equals
    ((dz @ ker(hz).T) % 2).any() or ((dx @ ker(hx).T) % 2).any() on random and crafted difference strings."""
    code, _, _ = bb_code(72)
    hx, hz, lx, lz = (np.asarray(m, np.int64) for m in (code.hx, code.hz, code.lx, code.lz))
    hx_perp, hz_perp = gf2.nullspace(code.hx), gf2.nullspace(code.hz)
    cx, cz = np.vstack([hx, lx]), np.vstack([hz, lz])
    assert gf2.rank(cx) == gf2.rank(hz_perp) == gf2.rank(np.vstack([cx, hz_perp])) == 72 - gf2.rank(code.hz)
    assert gf2.rank(cz) == gf2.rank(hx_perp) == gf2.rank(np.vstack([cz, hx_perp])) == 72 - gf2.rank(code.hx)
    rng = np.random.default_rng(11)
    zero = np.zeros(72, np.int64)
    one = zero.copy(); one[17] = 1
    # (dx, dz): an X-type operator lives in the X string -- rows of hx are its stabilisers, rows of lx its logicals -- and is seen by cz
    cases = [(zero, zero), (hx[3], hz[5]), (lx[0], zero), (zero, lz[4]), (one, zero), (zero, one), (hx[1] ^ hx[7], hz[0] ^ hz[2]),
             (lx[2] ^ hx[9], lz[1] ^ hz[30]), (lz[0], zero), (zero, lx[0])]
    cases += [(rng.integers(0, 2, 72), rng.integers(0, 2, 72)) for _ in range(100)]
    # combinations of stabilisers and logicals: in ker(h), so only the logical rows can fire
    for _ in range(100):
        dx = (rng.integers(0, 2, hx.shape[0]) @ hx + (rng.random() < 0.5) * (rng.integers(0, 2, lx.shape[0]) @ lx)) % 2
        dz = (rng.integers(0, 2, hz.shape[0]) @ hz + (rng.random() < 0.5) * (rng.integers(0, 2, lz.shape[0]) @ lz)) % 2
        cases.append((dx, dz))
    hits = 0
    for dx, dz in cases:
        mine = bool(((cx @ dz) % 2).any() or ((cz @ dx) % 2).any())
        assert mine == P.reference_logical_error(dx, dz, hx_perp, hz_perp)
        hits += mine
    assert 0 < hits < len(cases)
    assert not ((cx @ hz[5]) % 2).any() and not ((cz @ hx[3]) % 2).any()            # stabilisers: no row fires
    assert ((lz @ lx[0]) % 2).any() and not ((hz @ lx[0]) % 2).any()                # a logical: only logical rows fire
    assert ((hz @ one) % 2).any()                                                   # one qubit: a stabiliser row fires
