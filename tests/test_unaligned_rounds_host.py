"""The host window loops on codes whose round is no whole number of 32-bit words of residual syndrome: [[90,8,10]] (45 detector
rows per round) and SHYPS r = 3 (21 rows per round), p = 0.004.  ``sliding_window_decode_online_host`` and
``sliding_window_decode_rolling_host`` against ``sliding_window_decode_host`` with the oracle in the windows -- the executable
specification of the sessions on these round sizes (tests/test_gpu_unaligned_rounds.py, which imports the problem builders below).
Every other window-loop test runs on 36, 72 or 144 rows per round, where a row never changes its byte inside a word."""
import functools

import numpy as np
import pytest

from tests.test_rolling_host import expected_shot_results
from tests.test_session_host import KW, chunkings

N_HALF = {"bb90": 45, "shyps": 21}
# tag: (code, W, F, method, rounds of the template, rounds of the longer experiment a rolling session decodes on it)
PLANS = {"bb90_w3f1m1": ("bb90", 3, 1, 1, 6, 9), "bb90_w3f3m0": ("bb90", 3, 3, 0, 6, 9), "bb90_w4f2m1": ("bb90", 4, 2, 1, 8, 12),
         "shyps_w3f1m1": ("shyps", 3, 1, 1, 6, 9), "shyps_w4f2m1": ("shyps", 4, 2, 1, 8, 12)}
# tag: (row_stride, frame_rows) of rolling_template -- (3, 3, method 0) commits reach one block beyond the window
GEOMETRY = {"bb90_w3f1m1": (45, 135), "bb90_w3f3m0": (135, 180), "bb90_w4f2m1": (90, 180), "shyps_w3f1m1": (21, 63),
            "shyps_w4f2m1": (42, 84)}
# rounds: (detector rows, columns) of the detector error model
SHAPES = {"bb90": {6: (315, 2790), 8: (405, 3690), 9: (450, 4140), 12: (585, 5490)},
          "shyps": {6: (147, 1225), 8: (189, 1617), 9: (210, 1813), 12: (273, 2401), 14: (315, 2793)}}
HOST_CASES = ["bb90_w3f1m1", "bb90_w3f3m0", "bb90_w4f2m1", "shyps_w3f1m1"]


def n_half(tag):
    return N_HALF[tag.split("_")[0]]


@functools.lru_cache(maxsize=None)
def dem_for(code, rounds):
    if code == "bb90":
        from slidingwindowdecoder_amd.circuit import bb_dem
        from slidingwindowdecoder_amd.codes import bb_code
        c, A, B = bb_code(90)
        dem = bb_dem(c, A, B, 0.004, rounds)
    else:
        from slidingwindowdecoder_amd.shyps import shyps_dem
        dem = shyps_dem(3, 0.004, rounds)
    assert dem.chk.shape == SHAPES[code][rounds]
    return dem


@functools.lru_cache(maxsize=None)
def plan_windows_for(code, W, F, method, rounds):
    from slidingwindowdecoder_amd.windows import plan_windows
    dem, h = dem_for(code, rounds), N_HALF[code]
    plan = plan_windows(dem.chk, dem.obs, dem.priors, h, W, F, method=method)
    assert plan.chk.shape[0] == h * (rounds + 1)
    assert [w.row0 for w in plan.windows] == [F * h * t for t in range(len(plan.windows))]
    return plan


def plan_for(tag, rounds):
    code, W, F, method, _, _ = PLANS[tag]
    return plan_windows_for(code, W, F, method, rounds)


def template_plan(tag):
    return plan_for(tag, PLANS[tag][4])


def oracle_loop(plan, det, kw=KW, factory=None):
    """the offline host loop with the oracle in the windows: (total_e_hat, exit class [shots, windows], min_pm [shots, windows],
    bp_iteration [shots, windows]) -- the last three as the ORACLE reports them after every window decode"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sliding_window_decode_host
    shape = (det.shape[0], len(plan.windows))
    cls, pm, it = np.full(shape, -1, np.int32), np.zeros(shape), np.zeros(shape, np.int32)

    def tap(wi, j, dec, s, e_hat):
        cls[j, wi], pm[j, wi], it[j, wi] = getattr(dec, "exit_class", -1), dec.min_pm, getattr(dec, "bp_iteration", 0)
    factory = factory or (lambda w: O.osd_window(w.mat, channel_probs=w.prior, **kw))
    want, _ = sliding_window_decode_host(plan, det, factory, on_decode=tap)
    return want, cls, pm, it


@functools.lru_cache(maxsize=None)
def sampled(plan_key, shots, seed):
    from slidingwindowdecoder_amd.windows import sample_dem
    plan = plan_windows_for(*plan_key)
    det = sample_dem(plan.chk, plan.obs, plan.priors, shots, seed=seed)[0]
    det.setflags(write=False)
    return det


@functools.lru_cache(maxsize=None)
def experiment(tag, rounds, shots=16, seed=13):
    """(plan of ``rounds`` rounds, det, total_e_hat of the offline host loop with the oracle, its exit classes, min_pm,
    bp_iteration); shared, read-only"""
    plan = plan_for(tag, rounds)
    det = sampled(PLANS[tag][:4] + (rounds,), shots, seed)
    out = (plan, det) + oracle_loop(plan, det)
    for a in out[2:]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("tag", sorted(PLANS))
def test_template_geometry_is_off_the_word_grid(tag):
    """what makes these cases what they claim to be: the frame, or the number of rows it moves per window, is no multiple of four,
    and no window but the first starts at a whole word"""
    from slidingwindowdecoder_amd.windows import rolling_template
    code, W, F, method, R0, R = PLANS[tag]
    h = N_HALF[code]
    T = rolling_template(template_plan(tag))
    assert (T.n_half, T.W, T.F, T.R0) == (h, W, F, R0)
    assert (T.row_stride, T.frame_rows) == GEOMETRY[tag] and T.row_stride == F * h
    assert T.frame_rows % 4 != 0 or T.row_stride % 4 != 0
    assert T.serves(R) and T.serves(R0)
    assert any(w.row0 % 4 for w in plan_for(tag, R).windows) and h % 4 != 0
    # strides 45, 135, 21, 42 (and 90): every non-zero position of a row inside its word is covered
    assert {GEOMETRY[t][0] % 4 for t in PLANS} == {1, 2, 3}


def test_irregular_chunking_holds_the_unaligned_pieces():
    for h, n in ((45, 270), (21, 126), (45, 315), (21, 147)):
        sizes = [c.shape[1] for c in chunkings(np.zeros((1, n), np.uint8), h)["irregular"]]
        assert 1 in sizes and 3 in sizes and 0 in sizes and any(k > h for k in sizes) and sum(sizes) == n
        assert any(r % 4 for r in np.cumsum(sizes)[:-1])  # pieces begin inside a 32-bit word of the residual syndrome
    # the aligned rounds keep the list they always had
    assert [c.shape[1] for c in chunkings(np.zeros((1, 252), np.uint8))["irregular"]] == [1, 35, 50, 0, 22, 144]


def test_commit_reaches_rows_that_have_not_arrived_on_bb90():
    """(3, 3, method 0) on 45-row rounds: window 0 is ready after 135 rows and its committed columns touch rows up to 179"""
    import scipy.sparse as sp
    plan = template_plan("bb90_w3f3m0")
    assert [(w.row0, w.row1) for w in plan.windows] == [(0, 135), (135, 270), (270, 315)]
    w0 = plan.windows[0]
    assert sp.csc_matrix(plan.chk)[:, w0.col0:w0.col0 + w0.commit].indices.max() == 179 >= w0.row1


@pytest.mark.parametrize("chunking", ["rounds", "irregular"])
@pytest.mark.parametrize("tag", HOST_CASES)
def test_online_host_loop_equals_the_offline_loop(tag, chunking):
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sliding_window_decode_online_host
    plan, det, want = experiment(tag, PLANS[tag][4])[:3]
    chunks = chunkings(det, n_half(tag))[chunking]
    total, events, resid = sliding_window_decode_online_host(plan, chunks, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW))
    assert np.array_equal(total, want) and want.any()
    rows, nxt = 0, 0
    for ch, ev in zip(chunks, events):
        rows += ch.shape[1]
        ready = []
        while nxt < len(plan.windows) and rows >= plan.windows[nxt].row1:
            ready.append(nxt)
            nxt += 1
        assert [e[0] for e in ev] == ready
        for t, col0, faults in ev:
            w = plan.windows[t]
            assert col0 == w.col0 and np.array_equal(faults, want[:, w.col0:w.col0 + w.commit])
    assert nxt == len(plan.windows)
    assert np.array_equal(resid.any(axis=1), expected_shot_results(plan, det, want)[0])


@pytest.mark.parametrize("chunking", ["rounds", "irregular"])
@pytest.mark.parametrize("tag", HOST_CASES)
def test_rolling_host_loop_equals_the_offline_loop_of_the_long_plan(tag, chunking):
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sliding_window_decode_rolling_host
    h, rounds = n_half(tag), PLANS[tag][5]
    plan, det, want = experiment(tag, rounds)[:3]
    syndrome, final = det[:, :h * rounds], det[:, h * rounds:]
    events, flips, flagged = sliding_window_decode_rolling_host(template_plan(tag), chunkings(syndrome, h)[chunking], final,
                                                                lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW))
    assert [e[0] for e in events] == list(range(len(plan.windows)))
    for (t, faults), w in zip(events, plan.windows):
        assert np.array_equal(faults, want[:, w.col0:w.col0 + w.commit]), f"window {t}"
    want_flagged, want_flips = expected_shot_results(plan, det, want)
    assert np.array_equal(flagged, want_flagged) and np.array_equal(flips, want_flips)
    assert want.any()


def test_a_stride_cut_to_whole_words_is_caught():
    """the error a device frame that moved by ``row_stride & ~3`` rows would make, restated on the host: [[90,8,10]] (3, 1), the
    45-row stride cut to 44.  The committed faults differ from the offline loop's from window 1 on -- the rolling comparisons of
    this file and of the GPU file notice such a frame."""
    import copy
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import rolling_template, sliding_window_decode_rolling_host
    plan, det, want = experiment("bb90_w3f1m1", 9)[:3]
    T = copy.copy(rolling_template(template_plan("bb90_w3f1m1")))
    T.row_stride &= ~3
    assert T.row_stride == 44
    # (the host loop counts the rows in the frame by the same stride: 135 rows for the head, 44 more fill the frame again, 44 more
    # close it -- the first two windows are what is looked at)
    events, _, _ = sliding_window_decode_rolling_host(T, [det[:, :135], det[:, 135:179]], det[:, 179:223],
                                                      lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW))
    w0, w1 = plan.windows[:2]
    assert np.array_equal(events[0][1], want[:, w0.col0:w0.col0 + w0.commit])
    assert not np.array_equal(events[1][1], want[:, w1.col0:w1.col0 + w1.commit])
