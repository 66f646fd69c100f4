"""Rolling sessions (``SlidingWindowDecoder.rolling_session``, C ABI swd_pipeline_rolling_*): a template plan of R0 rounds decodes
experiments of R = R0 (mod F) rounds, R known only at ``finish``, on a frame of residual rows.  Expected values come from the
one-launch ``decode`` of a ``SlidingWindowDecoder`` built on ``plan_windows(R)`` and from the oracle driven through
``sliding_window_decode_host`` on that plan -- never from the rolling code itself.
[[72,12,6]], p = 0.004; seed 13 was chosen on the CPU with the oracle: in every case below the batch leaves through pre-processing
BP, post-processing BP and the OSD (``exit_classes``: the oracle's own exit class of every window decode, asserted per case)."""
import functools

import numpy as np
import pytest

from tests.test_rolling_host import CASES, KW, expected_shot_results, plan_for, template_plan
from tests.test_session_host import chunkings

pytestmark = pytest.mark.gpu

SEED, SHOTS = 13, 96
_EXIT_CLASSES = {}


@functools.lru_cache(maxsize=None)
def problem(tag, rounds, shots=SHOTS):
    """(plan of R rounds, det, total_e_hat of the oracle's host loop on it); shared, read-only"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sample_dem, sliding_window_decode_host
    plan = plan_for(tag, rounds)
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, shots, seed=SEED)
    cls = np.full((shots, len(plan.windows)), -1, np.int32)

    def tap(wi, j, dec, s, e_hat):
        cls[j, wi] = dec.exit_class
    want, _ = sliding_window_decode_host(plan, det, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW), on_decode=tap)
    for a in (det, want, cls):
        a.setflags(write=False)
    _EXIT_CLASSES[tag, rounds, shots] = cls
    return plan, det, want


def exit_classes(tag, rounds, shots=SHOTS):
    """[shots, windows]: the exit class of every window decode in the ORACLE's host loop (0 pre-BP, 1 post-BP, 2 OSD)"""
    problem(tag, rounds, shots)
    return _EXIT_CLASSES[tag, rounds, shots]


def decode_ref(dec, det):
    total = dec.decode(det).copy()
    ref = (total, dec.last_stats.copy(), dec.last_min_pm.copy(), dec.last_obs_flips.copy(), dec.last_flagged.copy())
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def one_launch(tag, rounds, shots=SHOTS):
    """what ``decode`` of a decoder built on plan_windows(R) leaves: (total, stats, min_pm, obs_flips, flagged)"""
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, det, _ = problem(tag, rounds, shots)
    return decode_ref(SlidingWindowDecoder(plan, **KW), det)


@functools.lru_cache(maxsize=None)
def template_decoder(tag):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    return SlidingWindowDecoder(template_plan(tag), **KW)


def run_rolling(ses, plan, det, chunking, ref, stat_words=8, device=False, rows_per_round=36):
    """pushes the syndrome rounds of ``det`` (``rows_per_round`` rows each) in pieces, finishes with the final block; every event is
    compared with ``ref``, the one-launch records of the plan of the experiment's own length"""
    h = int(rows_per_round)
    B, R = det.shape[0], det.shape[1] // h - 1
    total, st_ref, pm_ref, flips_ref, flagged_ref = [r[:B] for r in ref]
    ses.begin(B)
    events, rows = [], 0
    for ch in chunkings(det[:, :h * R], h)[chunking]:
        assert ses.rows_received == rows and ses.rounds_received == rows // h
        ev = ses.push(ch)
        rows += ch.shape[1]
        # a window is complete when its last row is there, and only syndrome rounds have been pushed: windows 0 .. n - 2 of the plan
        assert [e[0] for e in ev] == [t for t, w in enumerate(plan.windows[:-1]) if rows - ch.shape[1] < w.row1 <= rows and ch.shape[1]]
        events += ev
        if ses.windows_done < len(plan.windows) - 1:
            assert ses.rows_needed == plan.windows[ses.windows_done].row1 - rows
    assert ses.windows_done == len(plan.windows) - 1
    t, faults, st, pm, flips, flagged = ses.finish(det[:, h * R:])
    events.append((t, faults, st, pm))
    assert [e[0] for e in events] == list(range(len(plan.windows)))
    for (t, faults, st, pm), w in zip(events, plan.windows):
        assert faults.shape == (B, w.commit) and st.shape == (B, 8) and pm.shape == (B,)
        assert np.array_equal(faults, total[:, w.col0:w.col0 + w.commit]), f"window {t}"
        assert np.array_equal(st[:, :stat_words], st_ref[:, t, :stat_words]), f"window {t}"
        assert (pm == pm_ref[:, t]).all(), f"window {t}"
    assert np.array_equal(flips, flips_ref) and np.array_equal(flagged, flagged_ref)
    return events, flips, flagged


@pytest.mark.parametrize("chunking", ["rounds", "irregular"])
@pytest.mark.parametrize("tag,rounds", CASES)
def test_rolling_equals_one_launch_of_the_long_plan_and_oracle(tag, rounds, chunking):
    plan, det, want = problem(tag, rounds)
    ref = one_launch(tag, rounds)
    assert np.array_equal(ref[0], want), "the one-launch decode itself differs from the oracle on this plan"
    assert want.any()
    cls = exit_classes(tag, rounds)
    assert set(np.unique(cls)) == {0, 1, 2}  # in the oracle the batch leaves through pre-BP, post-BP and the OSD, all three
    assert np.array_equal(ref[1][..., 0] & 0xFF, cls)
    want_flagged, want_flips = expected_shot_results(plan, det, want)
    assert np.array_equal(ref[4], want_flagged)
    assert np.array_equal(ref[3], (want_flips.astype(np.uint32) << np.arange(want_flips.shape[1], dtype=np.uint32)).sum(axis=1))
    ses = template_decoder(tag).rolling_session(SHOTS)
    run_rolling(ses, plan, det, chunking, ref)
    ses.close()


@pytest.mark.parametrize("B", [1, 5])
def test_ragged_batches_in_a_larger_session(B):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, det, want = problem("w3f1m1", 9)
    ref = decode_ref(SlidingWindowDecoder(plan, **KW), det[:B])
    assert np.array_equal(ref[0], want[:B])
    ses = template_decoder("w3f1m1").rolling_session(8)
    run_rolling(ses, plan, det[:B], "irregular", ref)
    ses.close()


# BP alone (osd_order = -1): windows that do not converge leave a residual syndrome behind -- with the OSD of KW no shot of these
# experiments is flagged (checked with the oracle), and the sticky flagged bit would never be set
KW_NO_OSD = dict(pre_max_iter=4, post_max_iter=8, ms_scaling_factor=1.0, osd_method="osd_cs", osd_order=-1)


def test_flagged_shots_and_begin_again_after_finish():
    """(3, 1), R = 9, no OSD: 78 of the 96 shots end flagged in the oracle's host loop.  Two different batches through one session,
    then the first again: the sticky flag, the accumulators and the frame are really cleared by ``begin``."""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    from slidingwindowdecoder_amd.windows import sliding_window_decode_host
    plan, det, _ = problem("w3f1m1", 9)
    want, _ = sliding_window_decode_host(plan, det, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW_NO_OSD))
    want_flagged, _ = expected_shot_results(plan, det, want)
    assert want_flagged.sum() == 78
    ref = decode_ref(SlidingWindowDecoder(plan, **KW_NO_OSD), det)
    assert np.array_equal(ref[0], want) and np.array_equal(ref[4], want_flagged) and ref[3].any()
    ses = SlidingWindowDecoder(template_plan("w3f1m1"), **KW_NO_OSD).rolling_session(SHOTS)
    first = run_rolling(ses, plan, det, "rounds", ref)
    # the same rows in reverse shot order in between: flagged and unflagged shots change places
    assert not np.array_equal(want_flagged, want_flagged[::-1])
    run_rolling(ses, plan, det[::-1], "rounds", tuple(r[::-1] for r in ref))
    again = run_rolling(ses, plan, det, "irregular", ref)
    assert np.array_equal(first[1], again[1]) and np.array_equal(first[2], again[2])
    ses.close()


def test_long_run_in_the_memory_of_a_short_one():
    """R = 40 on the (3, 1) template of 6 rounds, 32 shots: equal to the one-launch decode of plan_windows(40); the session's device
    allocation is what it was for R = 9"""
    plan, det, want = problem("w3f1m1", 40, 32)
    ref = one_launch("w3f1m1", 40, 32)
    assert np.array_equal(ref[0], want) and len(plan.windows) == 39
    ses = template_decoder("w3f1m1").rolling_session(32)
    before = ses.device_bytes
    plan9, det9, _ = problem("w3f1m1", 9)
    run_rolling(ses, plan9, det9[:32], "rounds", one_launch("w3f1m1", 9))
    after9 = ses.device_bytes
    run_rolling(ses, plan, det, "irregular", ref)
    assert ses.device_bytes == after9 == before and before > 0
    # ... and it is the frame that is kept per shot, not the experiment: 108 rows against 41 * 36
    assert before < 32 * (plan.chk.shape[0] + plan.chk.shape[1])
    ses.close()


def test_guessing_decoder_windows():
    """bpgdg_decoder in the windows (parameters of tests/test_gpu_session.py::test_guessing_decoder_session): faults, statistics
    words 0-6 and min_pm of the one-launch decode of plan_windows(9); word 7 is a scheduling diagnostic (include/swd.h)"""
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    from tests import fixtures as fx
    plan, det, _ = problem("w3f1m1", 9)
    kw = fx.params(fx.load("bb72_capacity.npz"), "gdg_params")
    kw.pop("multi_thread", None)
    d = det[:48]
    ref = decode_ref(SlidingWindowDecoder(plan, decoder="bpgdg_decoder", **kw), d)
    assert ref[0].any()
    dec = SlidingWindowDecoder(template_plan("w3f1m1"), decoder="bpgdg_decoder", **kw)
    ses = dec.rolling_session(48)
    run_rolling(ses, plan, d, "rounds", ref, stat_words=7)
    ses.close()


def test_device_form_on_a_side_stream_with_caller_owned_faults():
    import torch
    plan, det, want = problem("w4f2m1", 12)
    ref = one_launch("w4f2m1", 12)
    dec = template_decoder("w4f2m1")
    ses = dec.rolling_session(SHOTS)
    host = run_rolling(ses, plan, det, "rounds", ref)[0]
    side = torch.cuda.Stream()
    ddet = torch.from_numpy(np.ascontiguousarray(det)).cuda()
    cmax = max(plan.windows[0].commit, plan.windows[1].commit)
    slab = torch.full((len(plan.windows), 2, SHOTS, cmax), 7, dtype=torch.uint8, device="cuda")  # room for two windows per push
    torch.cuda.synchronize()
    ses.begin(SHOTS)
    got, r = [], 0
    for k in [36, 72, 36, 108, 0, 72, 108]:  # unaligned with the (4, 2) windows; 108 + 72 rows complete two windows at once
        ev = ses.push_device(ddet[:, r:r + k], faults_out=slab[len(got)], stream=side)
        r += k
        for t, faults, st, pm in ev:
            assert faults.data_ptr() >= slab.data_ptr() and faults.is_cuda and st.is_cuda and pm.is_cuda
        got += ev
    assert r == 36 * 12
    t, faults, st, pm, flips, flagged = ses.finish_device(ddet[:, r:], stream=side)
    side.synchronize()
    got.append((t, faults, st, pm))
    assert len(got) == len(host) == len(plan.windows)
    for (t, faults, st, pm), (th, fh, sh, ph) in zip(got, host):
        assert t == th and np.array_equal(faults.cpu().numpy(), fh) and np.array_equal(st.cpu().numpy(), sh)
        assert (pm.cpu().numpy() == ph).all()
    assert np.array_equal(flips.cpu().numpy().astype(np.uint32), ref[3]) and np.array_equal(flagged.cpu().numpy().astype(bool), ref[4])
    # columns beyond a window's commit were left alone
    w0 = plan.windows[0]
    if w0.commit < cmax:
        assert (slab[0, 0, :, w0.commit:] == 7).all()
    ses.close()


def test_errors():
    plan, det, _ = problem("w4f2m1", 12)
    dec = template_decoder("w4f2m1")
    ses = dec.rolling_session(4)
    with pytest.raises(RuntimeError, match="begin first"):
        ses.push(np.zeros((0, 36), np.uint8))
    with pytest.raises(RuntimeError, match=r"5 shots, the session was created for 1\.\.4"):
        ses.begin(5)
    d = det[:4]
    # a wrong residue: 11 syndrome rounds on the template of 8 (mod 2); the state is untouched and the twelfth round mends it
    ses.begin(4)
    ses.push(d[:, :36 * 11])
    with pytest.raises(ValueError, match=r"11 syndrome rounds.*this template serves R = 8 \(mod 2\) syndrome rounds, R >= 4"):
        ses.finish(d[:, 36 * 12:])
    done = ses.windows_done
    ses.push(d[:, 36 * 11:36 * 12])
    assert ses.windows_done == done + 1
    with pytest.raises(ValueError, match="final block must go to finish"):
        ses.finish(d[:, :0])
    t, faults, _, _, _, _ = ses.finish(d[:, 36 * 12:])
    assert t == len(plan.windows) - 1
    with pytest.raises(RuntimeError, match="has been finished; begin a new batch"):
        ses.push(d[:, :36])
    # too few rows: no window before the tail
    ses.begin(4)
    ses.push(d[:, :36 * 2])
    with pytest.raises(ValueError, match="fewer rows than the first and the last window need"):
        ses.finish(d[:, 36 * 12:])
    # the library refuses the same on its own (a caller of the C ABI has no Python check in front)
    import ctypes as C
    from slidingwindowdecoder_amd import _lib
    rows = np.ascontiguousarray(d[:, 36 * 12:])
    assert _lib.lib().swd_pipeline_rolling_finish(ses._h, 36, rows.ctypes.data, None, None, None, None) != 0
    assert "fewer than the first and the last window need" in _lib.last_error()
    first, count = C.c_int64(), C.c_int32()
    big = np.zeros((4, 36 * 8), np.uint8)
    assert _lib.lib().swd_pipeline_rolling_push(ses._h, 36 * 8, big.ctypes.data, 1, None, None, None, C.byref(first), C.byref(count)) != 0
    assert "the output arrays hold 1" in _lib.last_error()
    ses.close()
    # a template that is not periodic is refused before anything is created
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    with pytest.raises(ValueError, match="at least two body windows"):
        SlidingWindowDecoder(plan_for("w3f1m1", 4), **KW).rolling_session(4)


def test_host_window_loop_plans_are_refused(monkeypatch):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    from tests.test_gpu_session import _tiny_host_loop_plan
    monkeypatch.setenv("SWD_FORCE_HUGE", "1")
    loop = SlidingWindowDecoder(_tiny_host_loop_plan(), pre_max_iter=4, post_max_iter=8, osd_method="osd_0")
    assert loop._loop is not None
    with pytest.raises(RuntimeError, match=r"rolling_session\(\) needs the one-launch pipeline"):
        loop.rolling_session(4)


def test_rolling_session_outlives_its_pipeline():
    """destroying the pipeline first is tolerated as for the online sessions: later calls fail with a message, close() still frees"""
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, det, _ = problem("w3f1m1", 9)
    dec = SlidingWindowDecoder(template_plan("w3f1m1"), **KW)
    ses = dec.rolling_session(4)
    ses.begin(4)
    assert [e[0] for e in ses.push(det[:4, :108])] == [0]
    dec.__del__()
    with pytest.raises(RuntimeError, match="pipeline of this session has been destroyed"):
        ses.push(det[:4, 108:144])
    with pytest.raises(RuntimeError, match="pipeline of this session has been destroyed"):
        ses.begin(4)
    ses.close()
