"""Rolling form of the window loop on the host: ``rolling_template`` and ``sliding_window_decode_rolling_host`` (a frame of residual
rows, head / body / tail windows of a template plan) against ``sliding_window_decode_host`` on ``plan_windows`` of the experiment's own
length, with the oracle in the windows -- the executable specification of ``SlidingWindowDecoder.rolling_session``
(tests/test_gpu_rolling.py).  [[72,12,6]], p = 0.004."""
import copy
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_session_host import KW, chunkings

# tag: (W, F, method, R0 of the template)
TEMPLATES = {"w3f1m1": (3, 1, 1, 6), "w4f2m1": (4, 2, 1, 8), "w3f3m0": (3, 3, 0, 6)}
CASES = [("w3f1m1", 9), ("w3f1m1", 14), ("w4f2m1", 12), ("w3f3m0", 9)]


@functools.lru_cache(maxsize=None)
def plan_for(tag, rounds):
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows
    code, A, B = bb_code(72)
    dem = bb_dem(code, A, B, 0.004, rounds)
    W, F, method, _ = TEMPLATES[tag]
    plan = plan_windows(dem.chk, dem.obs, dem.priors, 36, W, F, method=method)
    assert plan.chk.shape[0] == 36 * (rounds + 1)
    return plan


def template_plan(tag):
    return plan_for(tag, TEMPLATES[tag][3])


@functools.lru_cache(maxsize=None)
def experiment(tag, rounds, shots=16, seed=7):
    """(plan of the experiment's own length, det, total_e_hat of the offline host loop with the oracle)"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sample_dem, sliding_window_decode_host
    plan = plan_for(tag, rounds)
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, shots, seed=seed)
    want, _ = sliding_window_decode_host(plan, det, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW))
    want.setflags(write=False)
    det.setflags(write=False)
    return plan, det, want


def expected_shot_results(plan, det, want):
    """(residual-any [shots], observable flips [shots, num_obs]) of osd.py:184-187 for the committed faults ``want``"""
    t = sp.csr_matrix(want)
    resid = (det.astype(np.int32) + (t @ sp.csr_matrix(plan.chk.T.astype(np.int32))).toarray()) % 2
    flips = (t @ sp.csr_matrix(plan.obs.T.astype(np.int32))).toarray() % 2
    return resid.any(axis=1), flips.astype(np.uint8)


@pytest.mark.parametrize("tag", sorted(TEMPLATES))
def test_template_is_accepted(tag):
    from slidingwindowdecoder_amd.windows import rolling_template
    W, F, method, R0 = TEMPLATES[tag]
    plan = template_plan(tag)
    T = rolling_template(plan)
    assert (T.W, T.F, T.R0, T.n_half) == (W, F, R0, 36)
    assert T.row_stride == F * 36 and T.head is plan.windows[0] and T.body is plan.windows[1] and T.tail is plan.windows[-1]
    # the frame covers every row a committed column touches; (3, 3, method 0) commits reach one block beyond the window
    assert T.frame_rows == (4 * 36 if tag == "w3f3m0" else W * 36)
    assert T.body_chk.shape == (T.frame_rows, plan.windows[1].commit)
    for R in range(0, 30):
        assert T.serves(R) == (R >= W and (R - R0) % F == 0)


def test_template_windows_are_those_of_longer_plans():
    """what the rolling form rests on: head, body and tail of the template ARE the windows of plan_windows(R), R = R0 (mod F)"""
    from slidingwindowdecoder_amd.windows import _same_matrix
    for tag, R in CASES:
        tp, plan = template_plan(tag), plan_for(tag, R)
        pairs = [(tp.windows[0], plan.windows[0]), (tp.windows[-1], plan.windows[-1])] + [(tp.windows[1], w) for w in plan.windows[1:-1]]
        for a, b in pairs:
            assert _same_matrix(a.mat, b.mat) and np.array_equal(a.prior, b.prior) and a.commit == b.commit


def test_template_refuses_a_changed_prior_in_one_body_round():
    from slidingwindowdecoder_amd.windows import rolling_template
    plan = copy.copy(template_plan("w3f1m1"))
    plan.priors = plan.priors.copy()
    w2 = plan.windows[2]
    plan.priors[w2.col0 + 5] *= 1.5
    with pytest.raises(ValueError, match="priors.* not periodic"):
        rolling_template(plan)
    # ... and the same change made where plan_windows sees it (the window's own prior differs too)
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows
    code, A, B = bb_code(72)
    dem = bb_dem(code, A, B, 0.004, 6)
    priors = np.asarray(dem.priors, dtype=np.float64).copy()
    priors[template_plan("w3f1m1").perm[w2.col0 + 5]] *= 1.5
    with pytest.raises(ValueError, match="not periodic"):
        rolling_template(plan_windows(dem.chk, dem.obs, priors, 36, 3, 1, method=1))


def test_template_refuses_fewer_than_two_body_windows():
    from slidingwindowdecoder_amd.windows import rolling_template
    plan = plan_for("w3f1m1", 4)  # head, one body window of one round, tail
    assert len(plan.windows) == 3
    with pytest.raises(ValueError, match="at least two body windows"):
        rolling_template(plan)
    with pytest.raises(ValueError, match="a first, a body and a last window"):
        rolling_template(plan_for("w3f1m1", 3))


@pytest.mark.parametrize("chunking", ["whole", "rounds", "irregular"])
@pytest.mark.parametrize("tag,rounds", CASES)
def test_rolling_host_loop_equals_the_offline_loop_of_the_long_plan(tag, rounds, chunking):
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sliding_window_decode_rolling_host
    plan, det, want = experiment(tag, rounds)
    syndrome, final = det[:, :36 * rounds], det[:, 36 * rounds:]
    events, flips, flagged = sliding_window_decode_rolling_host(template_plan(tag), chunkings(syndrome)[chunking], final,
                                                                lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW))
    assert [e[0] for e in events] == list(range(len(plan.windows)))
    for (t, faults), w in zip(events, plan.windows):
        assert np.array_equal(faults, want[:, w.col0:w.col0 + w.commit]), f"window {t}"
    want_flagged, want_flips = expected_shot_results(plan, det, want)
    assert np.array_equal(flagged, want_flagged) and np.array_equal(flips, want_flips)
    assert want.any()


def test_rolling_host_loop_refuses_a_length_the_template_does_not_serve():
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sliding_window_decode_rolling_host
    fac = lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW)  # noqa: E731
    det = np.zeros((2, 36 * 12), np.uint8)
    with pytest.raises(ValueError, match=r"11 syndrome rounds; this template serves R = 8 \(mod 2\)"):
        sliding_window_decode_rolling_host(template_plan("w4f2m1"), [det[:, :36 * 11]], det[:, :36], fac)
    # fewer rows than head and tail need; the final block handed to a push
    with pytest.raises(ValueError, match="this template serves"):
        sliding_window_decode_rolling_host(template_plan("w4f2m1"), [det[:, :36 * 2]], det[:, :36], fac)
    with pytest.raises(ValueError, match="final block must go to the closing call"):
        sliding_window_decode_rolling_host(template_plan("w4f2m1"), [det[:, :36 * 13]], det[:, :0], fac)
