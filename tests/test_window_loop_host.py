"""The device window loop (``SlidingWindowDecoder(window_loop="device")``, csrc/swd_loop.hip) without a GPU: the keyword is checked
before the library is touched, the helpers that say which windows share a decoder and which rows a commit reaches, and the synthetic
overlapping plan and its shots that tests/test_gpu_window_loop.py decodes."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

H, N = 12, 40  # rows and columns of one block of ``overlap_plan``
KW = dict(pre_max_iter=4, post_max_iter=8, osd_method="osd_0")
SHOTS = 96


@functools.lru_cache(maxsize=None)
def overlap_plan(nb):
    """A plan of ``nb - 1`` overlapping windows that no pipeline kernel takes, small enough for the oracle: ``nb`` column blocks of
    40 columns, ``nb + 1`` row blocks of 12 rows.  Column block k carries the block matrix ``a`` in row block k and the spill matrix
    ``c`` in row block k + 1.  Column 0 of ``a`` has weight 11 (above the kernels' column weight 10: SWD_ERR_CAPACITY).  The last
    row block holds only the spill of the last column block, and its last row repeats the row before it: the last window is rank
    deficient.  Window t < nb - 2 covers row and column blocks t, t + 1 and commits one column block; the last window runs to the
    end and commits everything.  Windows 0 .. nb - 3 are identical."""
    from slidingwindowdecoder_amd.windows import Window, WindowPlan
    rng = np.random.default_rng(5)
    a = (rng.random((H, N)) < 0.15).astype(np.uint8)
    a[:, 0] = 0
    a[:H - 1, 0] = 1
    a[np.arange(H), 1 + np.arange(H)] = 1  # a shifted diagonal on columns 1..12: every row has a column of its own
    for j in np.flatnonzero(a.sum(axis=0) == 0):
        a[rng.integers(H), j] = 1
    c = (rng.random((H, N)) < 0.05).astype(np.uint8)
    c[:, 0] = 0
    c_last = c.copy()
    c_last[H - 1] = c_last[H - 2]
    chk = np.zeros(((nb + 1) * H, nb * N), np.uint8)
    for k in range(nb):
        chk[k * H:(k + 1) * H, k * N:(k + 1) * N] = a
        chk[(k + 1) * H:(k + 2) * H, k * N:(k + 1) * N] = c_last if k == nb - 1 else c
    priors = np.full(nb * N, 0.03)
    obs = (rng.random((3, nb * N)) < 0.2).astype(np.uint8)
    windows = []
    for t in range(nb - 1):
        last = t == nb - 2
        r0, r1, c0, c1 = t * H, ((nb + 1) if last else (t + 2)) * H, t * N, (t + 2) * N
        windows.append(Window(r0, r1, c0, c1 - c0, c1 - c0 if last else N, sp.csr_matrix(chk[r0:r1, c0:c1]), priors[c0:c1].copy(), last))
    return WindowPlan(sp.csr_matrix(chk), sp.csr_matrix(obs), priors, np.arange(nb * N), [(k * H, k * N) for k in range(nb + 1)],
                      windows, None, H)


@functools.lru_cache(maxsize=None)
def overlap_shots(nb, shots=SHOTS):
    """(det [shots, num_det], obs [shots, 3], flips uint32 [shots]): faults at 0.05, every third shot XORed with 10 % random
    detector bits (no fault pattern explains those: flagged shots, failing eliminations); read-only"""
    plan = overlap_plan(nb)
    rng = np.random.default_rng(11)
    e = (rng.random((shots, plan.chk.shape[1])) < 0.05).astype(np.int32)
    det = ((e @ plan.chk.T.toarray().astype(np.int32)) % 2).astype(np.uint8)
    det[::3] ^= (rng.random((len(det[::3]), det.shape[1])) < 0.1).astype(np.uint8)
    obs = ((e @ plan.obs.T.toarray().astype(np.int32)) % 2).astype(np.uint8)
    flips = (obs.astype(np.uint32) << np.arange(obs.shape[1], dtype=np.uint32)).sum(axis=1).astype(np.uint32)
    for x in (det, obs, flips):
        x.setflags(write=False)
    return det, obs, flips


@functools.lru_cache(maxsize=None)
def bb72_plan(rounds=5, W=3, F=1):
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows
    code, A, B = bb_code(72)
    dem = bb_dem(code, A, B, 0.004, rounds)
    return plan_windows(dem.chk, dem.obs, dem.priors, 36, W, F, 1)


def test_overlap_plan_is_what_the_gpu_tests_need():
    plan = overlap_plan(4)
    assert plan.chk.shape == (60, 160) and len(plan.windows) == 3
    w0, w1, w2 = plan.windows
    assert (w0.row0, w0.row1, w0.col0, w0.commit, w0.mat.shape) == (0, 24, 0, 40, (24, 80))
    assert (w1.row0, w1.row1, w1.col0, w1.commit, w1.mat.shape) == (12, 36, 40, 40, (24, 80))
    assert (w2.row0, w2.row1, w2.col0, w2.commit, w2.mat.shape) == (24, 60, 80, 80, (36, 80))
    assert int(w0.mat.sum(axis=0).max()) == 11 and int(plan.chk.getnnz(axis=0).min()) >= 1  # beyond the kernels' column weight; no empty column
    m2 = w2.mat.toarray()
    assert np.array_equal(m2[-1], m2[-2]) and m2[-1].any()  # the rank-deficient last window
    det, obs, flips = overlap_shots(4)
    assert det.shape == (SHOTS, 60) and obs.shape == (SHOTS, 3) and det.any() and flips.any()


def test_bad_window_loop_value_is_refused_before_the_library_is_touched(monkeypatch):
    from slidingwindowdecoder_amd import SlidingWindowDecoder, _lib

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    for bad in ("gpu", "Device", "", 0, True):
        with pytest.raises(ValueError, match="window_loop"):
            SlidingWindowDecoder(overlap_plan(4), window_loop=bad, **KW)


def test_distinct_windows():
    from slidingwindowdecoder_amd.windows import distinct_windows
    assert distinct_windows(bb72_plan()) == [0, 1, 1, 3]  # first, two body windows, last: 3 of 4
    assert distinct_windows(overlap_plan(4)) == [0, 0, 2]  # 2 of 3
    assert distinct_windows(overlap_plan(6)) == [0, 0, 0, 0, 4]
    # the priors count: the same matrix with another prior is another decoder
    import copy
    plan = copy.deepcopy(overlap_plan(4))
    plan.windows[1].prior[7] = 0.031
    assert distinct_windows(plan) == [0, 1, 2]


@pytest.mark.parametrize("geometry", [(5, 3, 1), (6, 3, 2)])
def test_committed_row_spans_of_the_bb_plan_lie_inside_their_windows(geometry):
    from slidingwindowdecoder_amd.windows import commit_row_spans
    plan = bb72_plan(*geometry)
    spans = commit_row_spans(plan)
    assert len(spans) == len(plan.windows)
    for w, (lo, hi) in zip(plan.windows, spans):
        assert w.row0 <= lo < hi <= w.row1, (w.row0, lo, hi, w.row1)
    dense = plan.chk.toarray()
    for w, (lo, hi) in zip(plan.windows, spans):  # the span is exact
        rows = np.flatnonzero(dense[:, w.col0:w.col0 + w.commit].any(axis=1))
        assert (lo, hi) == (rows.min(), rows.max() + 1)


def test_committed_row_spans_of_the_overlap_plan():
    from slidingwindowdecoder_amd.windows import commit_row_spans
    assert commit_row_spans(overlap_plan(4)) == [(0, 24), (12, 36), (24, 60)]
