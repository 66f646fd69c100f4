"""Online sessions (``SlidingWindowDecoder.session``, C ABI swd_pipeline_session_*): detector rows arrive in pieces, every window
is decoded and committed when its last row is there.  Expected values come from ``decode`` of the same decoder (one launch, the
whole experiment) and from the oracle driven through ``sliding_window_decode_host`` -- never from the session itself.
[[72,12,6]], 6 rounds, p = 0.004 (252 x 2232); seed 13 was chosen on the CPU with the oracle: its first shot alone already leaves
through pre-processing BP, post-processing BP and the OSD."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_gpu_rolling import KW_NO_OSD
from tests.test_rolling_host import expected_shot_results
from tests.test_session_host import KW, PLANS, chunkings

pytestmark = pytest.mark.gpu

SEED, SHOTS = 13, 96


@functools.lru_cache(maxsize=None)
def problem(tag):
    """(plan, det [96, 252], total_e_hat of the oracle's host loop); shared, read-only"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows, sample_dem, sliding_window_decode_host
    code, A, B = bb_code(72)
    dem = bb_dem(code, A, B, 0.004, 6)
    W, F, method = PLANS[tag]
    plan = plan_windows(dem.chk, dem.obs, dem.priors, 36, W, F, method=method)
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, SHOTS, seed=SEED)
    want, _ = sliding_window_decode_host(plan, det, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW))
    for a in (det, want):
        a.setflags(write=False)
    return plan, det, want


@functools.lru_cache(maxsize=None)
def one_launch(tag, B=SHOTS):
    """(decoder, what ``decode`` of the first B shots leaves: total, stats, min_pm, obs_flips, flagged)"""
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, det, _ = problem(tag)
    dec = SlidingWindowDecoder(plan, **KW) if B == SHOTS else one_launch(tag)[0]
    total = dec.decode(det[:B]).copy()
    ref = (total, dec.last_stats.copy(), dec.last_min_pm.copy(), dec.last_obs_flips.copy(), dec.last_flagged.copy())
    for a in ref:
        a.setflags(write=False)
    return dec, ref


def ready_windows(plan, rows_before, rows_after):
    return [t for t, w in enumerate(plan.windows) if rows_before < w.row1 <= rows_after]


def run_session(ses, plan, chunks, want):
    """pushes the chunks; every push must return exactly the windows it completed, each with the faults of ``want``"""
    B = chunks[0].shape[0]
    ses.begin(B)
    rows = 0
    for ch in chunks:
        assert ses.rows_received == rows
        if ses.windows_done < len(plan.windows):
            assert ses.rows_needed == plan.windows[ses.windows_done].row1
        ev = ses.push(ch)
        # (an empty piece completes nothing: row1 > rows_before excludes windows already returned)
        assert [e[0] for e in ev] == ready_windows(plan, rows, rows + ch.shape[1]) if ch.shape[1] else ev == []
        rows += ch.shape[1]
        for t, col0, faults, st, pm in ev:
            w = plan.windows[t]
            assert col0 == w.col0 and faults.shape == (B, w.commit)
            assert np.array_equal(faults, want[:B, w.col0:w.col0 + w.commit]), f"window {t}"
            assert st.shape == (B, 8) and pm.shape == (B,)
    assert ses.windows_done == len(plan.windows) and ses.rows_needed is None
    return ses.finish()


def assert_equals_decode(got, ref, stat_words=8):
    total, st, pm, flips, flagged = got
    assert np.array_equal(total, ref[0])
    assert np.array_equal(st[..., :stat_words], ref[1][..., :stat_words])
    assert (pm == ref[2]).all()
    assert np.array_equal(flips, ref[3]) and np.array_equal(flagged, ref[4])


@pytest.mark.parametrize("chunking", ["whole", "rounds", "irregular"])
def test_session_equals_one_launch_and_oracle(chunking):
    plan, det, want = problem("w3f1m1")
    dec, ref = one_launch("w3f1m1")
    assert np.array_equal(ref[0], want)  # the one-launch decode against the oracle's host loop
    assert len(np.unique(ref[1][..., 0] & 0xFF)) >= 2
    ses = dec.session(SHOTS)
    got = run_session(ses, plan, chunkings(det)[chunking], want)
    assert_equals_decode(got, ref)
    full = (det.astype(np.int32) + (sp.csr_matrix(want) @ sp.csr_matrix(plan.chk.T.astype(np.int32))).toarray()) % 2
    assert np.array_equal(got[4], full.any(axis=1))
    # per-window records of a committed window stay readable after finish
    t, col0, faults, st, pm = ses.window(2)
    assert np.array_equal(st, ref[1][:, 2]) and (pm == ref[2][:, 2]).all()
    ses.close()


def test_commit_into_rows_that_have_not_arrived():
    """(3, 3, method 0), one round per push: window 0 is decoded after 108 rows and its committed faults flip rows up to 143, which
    arrive later.  The oracle is the expectation; the one-launch decode is compared with it too."""
    plan, det, want = problem("w3f3m0")
    w0 = plan.windows[0]
    assert sp.csc_matrix(plan.chk)[:, w0.col0:w0.col0 + w0.commit].indices.max() >= w0.row1
    dec, ref = one_launch("w3f3m0")
    ses = dec.session(SHOTS)
    got = run_session(ses, plan, chunkings(det)["rounds"], want)
    assert np.array_equal(got[0], want)
    assert np.array_equal(ref[0], want), "the one-launch decode itself differs from the oracle on this plan"
    assert_equals_decode(got, ref)
    assert len(np.unique(got[1][..., 0] & 0xFF)) >= 2


@pytest.mark.parametrize("B", [1, 5])
def test_ragged_batches_and_unaligned_rows(B):
    plan, det, want = problem("w3f1m1")
    dec, ref = one_launch("w3f1m1", B)
    assert np.array_equal(ref[0], want[:B])
    ses = dec.session(8)
    got = run_session(ses, plan, chunkings(det[:B])["irregular"], want)
    assert_equals_decode(got, ref)
    assert len(np.unique(got[1][..., 0] & 0xFF)) >= 2


# BP alone (KW_NO_OSD): windows that do not converge leave a residual syndrome behind.  With the OSD of KW no shot of ``problem`` ends
# flagged (0 of 96 for both plans, checked with the oracle), so ``flagged`` of the tests above is only ever compared with zeros.
FLAGGED = {"w3f1m1": 70, "w3f3m0": 75}  # of the 96 shots, in the oracle's host loop (computed on the CPU)


@functools.lru_cache(maxsize=None)
def bp_only(tag):
    """(decoder with KW_NO_OSD, what its one-launch ``decode`` leaves, the oracle's total_e_hat, flagged [shots], obs_flips [shots]);
    the one-launch decode is compared with the oracle here, once"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    from slidingwindowdecoder_amd.windows import sliding_window_decode_host
    plan, det, _ = problem(tag)
    want, _ = sliding_window_decode_host(plan, det, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW_NO_OSD))
    flagged, flips = expected_shot_results(plan, det, want)
    flips = (flips.astype(np.uint32) << np.arange(flips.shape[1], dtype=np.uint32)).sum(axis=1).astype(np.uint32)
    dec = SlidingWindowDecoder(plan, **KW_NO_OSD)
    total = dec.decode(det).copy()
    ref = (total, dec.last_stats.copy(), dec.last_min_pm.copy(), dec.last_obs_flips.copy(), dec.last_flagged.copy())
    for a in ref + (want, flagged, flips):
        a.setflags(write=False)
    assert np.array_equal(ref[0], want) and np.array_equal(ref[3], flips) and np.array_equal(ref[4], flagged)
    return dec, ref, want, flagged, flips


@pytest.mark.parametrize("tag", ["w3f1m1", "w3f3m0"])
def test_flagged_shots_and_begin_again(tag):
    """No OSD: most shots end flagged, every shot with an observable flip.  The batch, the same rows in reverse shot order (flagged
    and unflagged shots change places), the batch again in irregular pieces, all through one session: residual syndrome and
    accumulators are really cleared by ``begin``, and ``flagged`` is compared with both values.  (3, 3, method 0) is the plan whose
    window-0 commit flips rows that have not arrived yet."""
    plan, det, _ = problem(tag)
    dec, ref, want, flagged, flips = bp_only(tag)
    assert flagged.sum() == FLAGGED[tag] and 0 < flagged.sum() < SHOTS and (flips != 0).sum() == SHOTS
    assert not np.array_equal(flagged, flagged[::-1])
    ses = dec.session(SHOTS)
    assert_equals_decode(run_session(ses, plan, chunkings(det)["rounds"], want), ref)
    assert_equals_decode(run_session(ses, plan, chunkings(det[::-1])["rounds"], want[::-1]), tuple(r[::-1] for r in ref))
    assert_equals_decode(run_session(ses, plan, chunkings(det)["irregular"], want), ref)
    ses.close()


def test_fixed_and_rolling_sessions_agree_on_the_template_length():
    """(3, 1) of 6 rounds, no OSD: one decoder is the fixed plan and the rolling template.  Fed the same rounds -- the rolling session
    gets the last block through ``finish`` -- both commit the same faults with the same records window by window, and end with the
    oracle's obs_flips and flagged."""
    plan, det, _ = problem("w3f1m1")
    dec, ref, want, flagged, flips = bp_only("w3f1m1")
    fixed, rolling = dec.session(SHOTS), dec.rolling_session(SHOTS)
    fixed.begin(SHOTS)
    rolling.begin(SHOTS)
    ev_f, ev_r = [], []
    for ch in chunkings(det)["rounds"][:-1]:
        ev_f += fixed.push(ch)
        ev_r += rolling.push(ch)
    ev_f += fixed.push(det[:, -36:])
    t, faults, st, pm, flips_r, flagged_r = rolling.finish(det[:, -36:])
    ev_r.append((t, faults, st, pm))
    assert [e[0] for e in ev_f] == [e[0] for e in ev_r] == list(range(len(plan.windows)))
    for (t, col0, ff, sf, pf), (_, fr, sr, pr) in zip(ev_f, ev_r):
        assert np.array_equal(ff, fr) and np.array_equal(sf, sr) and (pf == pr).all(), f"window {t}"
        assert np.array_equal(ff, want[:, col0:col0 + ff.shape[1]]), f"window {t}"
    got = fixed.finish()
    assert_equals_decode(got, ref)
    assert np.array_equal(got[3], flips_r) and np.array_equal(got[4], flagged_r)
    assert np.array_equal(flips_r, flips) and np.array_equal(flagged_r, flagged)
    fixed.close()
    rolling.close()


def test_guessing_decoder_session():
    """bpgdg_decoder in the windows (parameters of the [[72,12,6]] case of tests/test_gpu_gdg.py): the session equals decode() in
    total_e_hat, statistics words 0-6 and min_pm; word 7 is a scheduling diagnostic (include/swd.h)."""
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    from tests import fixtures as fx
    plan, det, _ = problem("w3f1m1")
    kw = fx.params(fx.load("bb72_capacity.npz"), "gdg_params")
    kw.pop("multi_thread", None)
    dec = SlidingWindowDecoder(plan, decoder="bpgdg_decoder", **kw)
    d = det[:48]
    ref = (dec.decode(d).copy(), dec.last_stats.copy(), dec.last_min_pm.copy(), dec.last_obs_flips.copy(), dec.last_flagged.copy())
    assert ref[0].any()
    ses = dec.session(48)
    got = run_session(ses, plan, chunkings(d)["rounds"], ref[0])
    assert_equals_decode(got, ref, stat_words=7)


def test_device_form_two_sessions_interleaved_on_a_side_stream():
    import torch
    plan, det, want = problem("w3f1m1")
    dec, _ = one_launch("w3f1m1")
    halves = [det[:40], det[40:]]
    refs = []
    for d in halves:
        total = dec.decode(d).copy()
        refs.append((total, dec.last_stats.copy(), dec.last_min_pm.copy(), dec.last_obs_flips.copy(), dec.last_flagged.copy()))
    assert np.array_equal(np.concatenate([r[0] for r in refs]), want)
    side = torch.cuda.Stream()
    dets = [torch.from_numpy(np.ascontiguousarray(d)).cuda() for d in halves]
    torch.cuda.synchronize()
    sessions = [dec.session(len(d)) for d in halves]

    def run(which):
        for k in which:
            sessions[k].begin(len(halves[k]))
        rows = 0
        for r in range(0, 252, 36):  # round by round, the sessions in turn
            for k in which:
                first, count = sessions[k].push_device(dets[k][:, r:r + 36], stream=side)
                assert list(range(first, first + count)) == ready_windows(plan, rows, r + 36)
            rows = r + 36
        return {k: sessions[k].finish() for k in which}

    got = run([0, 1])
    for k in (0, 1):
        assert_equals_decode(got[k], refs[k])
        side.synchronize()
        assert np.array_equal(sessions[k].total_device().cpu().numpy(), refs[k][0])
    # a used session starts again from a zero state
    again = run([1])
    assert_equals_decode(again[1], refs[1])
    assert_equals_decode(sessions[0].finish(), refs[0])  # ... and the other one kept its own
    for s in sessions:
        s.close()


def _tiny_host_loop_plan():
    """two windows whose matrices have a column of weight 11: beyond every pipeline kernel (column weight <= 10), so the decoder runs
    its host window loop over general-form decoders"""
    from slidingwindowdecoder_amd.windows import Window, WindowPlan
    rng = np.random.default_rng(3)
    h, n = 12, 40
    blocks = []
    for _ in range(2):
        a = (rng.random((h, n)) < 0.15).astype(np.uint8)
        a[:11, 0] = 1
        a[np.arange(h), 1 + np.arange(h)] = 1
        a[:, 1:][:, a[:, 1:].sum(axis=0) == 0] = 1
        blocks.append(sp.csr_matrix(a))
    chk = sp.block_diag(blocks, format="csr")
    priors = np.full(2 * n, 0.02)
    obs = sp.csr_matrix(np.ones((1, 2 * n), np.uint8))
    wins = [Window(k * h, (k + 1) * h, k * n, n, n, blocks[k], priors[:n].copy(), k == 1) for k in range(2)]
    return WindowPlan(chk, obs, priors, np.arange(2 * n), [(0, 0), (h, n), (2 * h, 2 * n)], wins, None, h)


def test_errors(monkeypatch):
    plan, det, _ = problem("w3f1m1")
    dec, _ = one_launch("w3f1m1")
    ses = dec.session(4)
    with pytest.raises(RuntimeError, match="begin first"):
        ses.push(np.zeros((0, 36), np.uint8))
    with pytest.raises(RuntimeError, match=r"5 shots, the session was created for 1\.\.4"):
        ses.begin(5)
    ses.begin(4)
    with pytest.raises(RuntimeError, match="253 rows after 0 received, the experiment has 252"):
        ses.push(np.zeros((4, 253), np.uint8))
    assert ses.push(det[:4, :36]) == []
    with pytest.raises(RuntimeError, match=r"window 0 of 5 waits for detector rows 36\.\.107 \(36 of 252 received\)"):
        ses.finish()
    with pytest.raises(RuntimeError, match="217 rows after 36 received"):
        ses.push(np.zeros((4, 217), np.uint8))
    assert [e[0] for e in ses.push(det[:4, 36:])] == [0, 1, 2, 3, 4]
    with pytest.raises(RuntimeError, match="the last window has been committed"):
        ses.push(np.zeros((4, 1), np.uint8))
    with pytest.raises(RuntimeError, match="the last window has been committed"):
        ses.push(np.zeros((4, 0), np.uint8))
    total = ses.finish()[0]
    assert np.array_equal(total, dec.decode(det[:4]))
    ses.close()
    # a plan that runs as a host window loop has no sessions (as it has no stream())
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    monkeypatch.setenv("SWD_FORCE_HUGE", "1")
    loop = SlidingWindowDecoder(_tiny_host_loop_plan(), pre_max_iter=4, post_max_iter=8, osd_method="osd_0")
    assert loop._loop is not None
    with pytest.raises(RuntimeError, match=r"session\(\) needs the one-launch pipeline"):
        loop.session(4)
    with pytest.raises(RuntimeError, match=r"stream\(\) needs the one-launch pipeline"):
        loop.stream(4)


def test_session_outlives_its_pipeline():
    """destroying the pipeline first is tolerated as for stream objects: later calls fail with a message, close() still frees"""
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, det, _ = problem("w3f1m1")
    dec = SlidingWindowDecoder(plan, **KW)
    ses = dec.session(4)
    ses.begin(4)
    ses.push(det[:4, :108])
    dec.__del__()
    with pytest.raises(RuntimeError, match="pipeline of this session has been destroyed"):
        ses.push(det[:4, 108:144])
    ses.close()
