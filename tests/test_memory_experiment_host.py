"""The memory experiment on the host: ``windows.memory_experiment_host`` -- the executable specification of ``MemoryExperiment``
(tests/test_gpu_memory_experiment.py) -- against ``logical_error_stats`` on the oracle's window loop, and the arithmetic of
``MemoryResult``.  [[72,12,6]], 6 rounds, p = 0.004; the shots are the device sampler's own stream as tests/philox_ref.py restates
it, so the GPU tests decode the same 160 shots."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import philox_ref
from tests.test_gpu_rolling import KW_NO_OSD
from tests.test_session_host import KW

SEED, SHOTS = 20240318, 160
PARAMS = {"KW": KW, "KW_NO_OSD": KW_NO_OSD}


@functools.lru_cache(maxsize=None)
def plan_for(W=3, F=1, method=1):
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows
    code, A, B = bb_code(72)
    dem = bb_dem(code, A, B, 0.004, 6)
    return plan_windows(dem.chk, dem.obs, dem.priors, 36, W, F, method=method)


def sample(plan, shots, seed=SEED, first_shot=0):
    """(det [shots, num_det], obs [shots, num_obs], flips uint32 [shots]) of the device sampler's stream, restated in numpy"""
    e = sp.csr_matrix(philox_ref.sample_faults(plan.priors, shots, seed, first_shot).astype(np.int32))
    det = ((e @ plan.chk.T.astype(np.int32)).toarray() % 2).astype(np.uint8)
    obs = ((e @ plan.obs.T.astype(np.int32)).toarray() % 2).astype(np.uint8)
    flips = (obs.astype(np.uint32) << np.arange(obs.shape[1], dtype=np.uint32)).sum(axis=1).astype(np.uint32)
    return det, obs, flips


@functools.lru_cache(maxsize=None)
def specification(kw="KW", geometry=(3, 1, 1), shots=SHOTS, first_shot=0):
    """(plan, det, obs, flips, what ``memory_experiment_host`` returns with the oracle's osd_window in the windows); shared, read-only"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import memory_experiment_host
    plan = plan_for(*geometry)
    det, obs, flips = sample(plan, shots, SEED, first_shot)
    spec = memory_experiment_host(plan, det, obs, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **PARAMS[kw]))
    for a in (det, obs, flips) + tuple(v for v in spec.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return plan, det, obs, flips, spec


def as_result(spec, failures=True):
    """the ``MemoryResult`` a run over the specification's shots must give (shots numbered from 0, every failing shot kept)"""
    from slidingwindowdecoder_amd import MemoryResult
    return MemoryResult(spec["shots"], spec["logical_errors"], spec["flagged"], spec["observable_mismatches"], spec["window_exit_classes"],
                        spec["window_not_converged"], spec["window_bp_iterations"],
                        failed_shots=np.flatnonzero(spec["result"] & 1) if failures else None, failed_shots_complete=failures or None)


@pytest.mark.parametrize("kw,geometry", [("KW", (3, 1, 1)), ("KW_NO_OSD", (3, 1, 1)), ("KW", (3, 3, 0))])
def test_restatement_equals_logical_error_stats_of_the_oracle_loop(kw, geometry):
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import logical_error_stats, sliding_window_decode_host
    plan, det, obs, flips, spec = specification(kw, geometry)
    assert plan.chk.shape == (252, 2232) and det.shape == (SHOTS, 252) and obs.shape == (SHOTS, 12)
    exits = np.zeros((len(plan.windows), 8), np.int64)

    def tap(wi, j, dec, s, e_hat):
        exits[wi, dec.exit_class] += 1
    total, not_solved = sliding_window_decode_host(plan, det, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **PARAMS[kw]), on_decode=tap)
    flagged, logical = logical_error_stats(plan, det, obs, total)
    wrong = (obs != (total.astype(np.int64) @ plan.obs.T.toarray().astype(np.int64)) % 2).any(axis=1)
    print(f"{kw} {geometry}: logical {int(logical.sum())}, flagged {int(flagged.sum())}, mismatches {int(wrong.sum())}, "
          f"flagged with correct observables {int((flagged & ~wrong).sum())} of {SHOTS}")
    assert np.array_equal(spec["total_e_hat"], total)
    assert (spec["shots"], spec["logical_errors"], spec["flagged"], spec["observable_mismatches"]) == \
        (SHOTS, int(logical.sum()), int(flagged.sum()), int(wrong.sum()))
    assert np.array_equal(spec["result"] & 1, logical) and np.array_equal((spec["result"] >> 1) & 1, flagged)
    assert np.array_equal((spec["result"] >> 2) & 1, wrong) and np.array_equal(logical, flagged | wrong)
    # per window: every shot leaves through one exit class; a window decode that does not reproduce its syndrome did not converge
    assert np.array_equal(spec["window_exit_classes"], exits) and (exits.sum(axis=1) == SHOTS).all()
    assert spec["window_not_converged"].shape == (len(plan.windows),) and (spec["window_not_converged"] >= np.array(not_solved)).all()
    assert (spec["window_bp_iterations"] >= SHOTS).all()
    # the cases the device tests lean on
    if kw == "KW" and geometry == (3, 1, 1):
        assert (wrong & ~flagged).any(), "no shot fails by observable mismatch while not flagged"
    if kw == "KW_NO_OSD":
        assert (flagged & ~wrong).any(), "no flagged shot has correct observables"
        assert (~logical).any(), "no shot has neither error"


def test_restatement_without_window_records():
    """a factory whose decoders expose no exit class: the counters all the same, the per-window counts None"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import memory_experiment_host
    plan, det, obs, flips, spec = specification()

    class Bare:
        def __init__(self, w):
            self._d = O.osd_window(w.mat, channel_probs=w.prior, **KW)

        def decode(self, s):
            return self._d.decode(s)
    got = memory_experiment_host(plan, det[:12], obs[:12], Bare)
    assert got["window_exit_classes"] is None and got["window_not_converged"] is None and got["window_bp_iterations"] is None
    assert np.array_equal(got["result"], spec["result"][:12]) and got["shots"] == 12


def test_memory_result_arithmetic():
    from slidingwindowdecoder_amd import MemoryResult
    r = MemoryResult(160, 5, 1, 4)
    assert r.ler == 5 / 160 and r.ler_stderr == pytest.approx(np.sqrt((5 / 160) * (155 / 160) / 160), rel=1e-12)
    assert r.ler_per_round(6) == pytest.approx(1.0 - (1.0 - 5 / 160) ** (1.0 / 6), rel=1e-12) and r.ler_per_round(1) == pytest.approx(r.ler)
    assert np.isnan(MemoryResult(0, 0, 0, 0).ler) and np.isnan(MemoryResult(0, 0, 0, 0).ler_stderr)
    assert r.window_exit_classes is None and len(r.failed_shots) == 0 and not r.failed_shots_complete
    assert r == MemoryResult(160, 5, 1, 4) and r != MemoryResult(160, 5, 0, 4) and r != MemoryResult(160, 5, 1, 5) and r != (160, 5, 1, 4)
    win = (np.arange(16).reshape(2, 8), [3, 0], [700, 800])
    a = MemoryResult(160, 2, 1, 1, *win, failed_shots=[2 ** 40 + 7, 3])
    assert a.failed_shots.dtype == np.uint64 and a.failed_shots.tolist() == [3, 2 ** 40 + 7] and a.failed_shots_complete
    assert a == MemoryResult(160, 2, 1, 1, *win, failed_shots=[3, 2 ** 40 + 7]) and a != MemoryResult(160, 2, 1, 1, *win, failed_shots=[3, 8])
    assert a != MemoryResult(160, 2, 1, 1, failed_shots=[3, 2 ** 40 + 7]) and a != MemoryResult(160, 2, 1, 1, win[0], win[1], [700, 801], failed_shots=[3, 2 ** 40 + 7])
    # an incomplete list is not reproducible: it stays out of the comparison, its completeness does not
    b, c = MemoryResult(160, 2, 1, 1, *win, failed_shots=[3]), MemoryResult(160, 2, 1, 1, *win, failed_shots=[2 ** 40 + 7])
    assert not b.failed_shots_complete and b == c and b != a
    s = a + MemoryResult(40, 1, 0, 1, *win, failed_shots=[200])
    assert (s.shots, s.logical_errors, s.flagged, s.observable_mismatches) == (200, 3, 1, 2) and s.failed_shots.tolist() == [3, 200, 2 ** 40 + 7]
    assert s.failed_shots_complete and np.array_equal(s.window_bp_iterations, [1400, 1600]) and np.array_equal(s.window_exit_classes, 2 * win[0])
    assert (a + r).window_not_converged is None and not (a + r).failed_shots_complete
    assert "logical_errors=2" in repr(a) and "window_not_converged=[3, 0]" in repr(a)
