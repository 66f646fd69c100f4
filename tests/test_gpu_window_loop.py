"""The device window loop, ``SlidingWindowDecoder(window_loop="device")`` (C ABI swd_window_loop_*, csrc/swd_loop.hip): one
single-window decoder per distinct window, residual syndrome, commit and accounting on the device.  Against the oracle's loop
(``windows.memory_experiment_host``) and the host loop on a synthetic plan of overlapping windows that no pipeline kernel takes
(tests/test_window_loop_host.py: ``overlap_plan``), against the one-launch pipeline on [[72,12,6]] plans (other tests pin that
pipeline to the oracle), through ``decode_device`` with the caller's buffers and alternating streams, and in ``MemoryExperiment``."""
import functools

import numpy as np
import pytest

from tests.test_session_host import KW as KW_BB
from tests.test_window_loop_host import KW, SHOTS, bb72_plan, overlap_plan, overlap_shots

pytestmark = pytest.mark.gpu
KW_GDG = dict(max_iter=8, max_iter_per_step=6, max_step=4, max_tree_depth=2, max_side_depth=4, max_tree_branch_step=4,
              max_side_branch_step=4, gdg_factor=1.0, ms_scaling_factor=1.0)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _decode(dec, det):
    """-> (total, stats, min_pm, obs flips, flagged) of one host ``decode``, copies"""
    total = dec.decode(det)
    return _frozen(total.copy(), dec.last_stats.copy(), dec.last_min_pm.copy(), dec.last_obs_flips.copy(), dec.last_flagged.copy())


@functools.lru_cache(maxsize=None)
def oracle_spec():
    """``memory_experiment_host`` with the oracle's osd_window on the 96 shots of ``overlap_plan(4)``; shared, read-only"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import memory_experiment_host
    plan = overlap_plan(4)
    det, obs, flips = overlap_shots(4)
    spec = memory_experiment_host(plan, det, obs, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW))
    _frozen(*(v for v in spec.values() if isinstance(v, np.ndarray)))
    # the reference side is not trivial: flagged shots, and at least three ways out of a window
    assert spec["flagged"] >= 1 and (spec["window_exit_classes"].sum(axis=0) > 0).sum() >= 3, spec["window_exit_classes"]
    return spec


@functools.lru_cache(maxsize=None)
def host_loop(decoder="osd_window", shots=SHOTS):
    """the host loop (``window_loop="host"``) on the first ``shots`` shots of ``overlap_plan(4)``; shared, read-only"""
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    dec = SlidingWindowDecoder(overlap_plan(4), decoder=decoder, window_loop="host", **(KW if decoder == "osd_window" else KW_GDG))
    assert dec.window_loop == "host" and dec.distinct_windows == 2 and len(dec._loop) == 3
    return _decode(dec, overlap_shots(4)[0][:shots])


# ---- 1. overlapping windows beyond the pipeline kernels: the oracle and the host loop ------------------------------------------
@pytest.mark.parametrize("force_huge", [False, True])
def test_overlap_plan_equals_the_oracle_and_the_host_loop(force_huge, monkeypatch):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    if force_huge:
        monkeypatch.setenv("SWD_FORCE_HUGE", "1")
    plan, (det, obs, flips), spec = overlap_plan(4), overlap_shots(4), oracle_spec()
    dec =SlidingWindowDecoder(plan, window_loop="device", **KW)
    assert dec.window_loop == "device" and dec.distinct_windows == 2 and dec.last_form is None and dec._loop is None
    total, stats, min_pm, oflips, flagged = _decode(dec, det)
    dec.check_status()
    # the oracle
    assert np.array_equal(total, spec["total_e_hat"])
    W = len(plan.windows)
    exits = np.stack([np.bincount(stats[:, t, 0] & 7, minlength=8) for t in range(W)])
    assert np.array_equal(exits, spec["window_exit_classes"]), exits
    assert np.array_equal(stats[:, :, 1].sum(axis=0), spec["window_bp_iterations"])
    assert np.array_equal(((stats[:, :, 0] & 0x100) == 0).sum(axis=0), spec["window_not_converged"])
    assert np.array_equal(flagged, (spec["result"] >> 1) & 1) and flagged.sum() == spec["flagged"]
    assert np.array_equal(oflips != flips, (spec["result"] >> 2) & 1)
    want_flips = ((spec["total_e_hat"].astype(np.int64) @ plan.obs.T.toarray().astype(np.int64)) % 2).astype(np.uint32)
    assert np.array_equal(oflips, (want_flips << np.arange(3, dtype=np.uint32)).sum(axis=1))
    # the host loop: every word
    h = host_loop()
    for name, a, b in zip(("total", "stats", "min_pm", "obs_flips", "flagged"), (total, stats, min_pm, oflips, flagged), h):
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    # one shot (every shot by itself gives its row of the batch), packed output, an empty batch
    for b in (0, 3, 95):
        one = _decode(dec, det[b:b + 1])
        for name, a, x in zip(("total", "stats", "min_pm", "obs_flips", "flagged"), one, (total, stats, min_pm, oflips, flagged)):
            assert np.array_equal(a, x[b:b + 1]), (name, b)
    assert np.array_equal(np.unpackbits(dec.decode(det, packed=True), axis=1, count=plan.chk.shape[1], bitorder="little"), total)
    assert dec.decode(det[:0]).shape == (0, plan.chk.shape[1])


def test_overlap_plan_guessing_decoder_equals_the_host_loop():
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    det = overlap_shots(4)[0][:32]
    dec = SlidingWindowDecoder(overlap_plan(4), decoder="bpgdg_decoder", window_loop="device", **KW_GDG)
    assert dec.window_loop == "device" and dec.distinct_windows == 2
    got, want = _decode(dec, det), host_loop("bpgdg_decoder", 32)
    assert len(set((want[1][:, :, 0] & 0x1FF).ravel().tolist())) >= 2, "one way out only"
    for name, a, b in zip(("total", "stats", "min_pm", "obs_flips", "flagged"), got, want):
        if name == "stats":  # word 7 of the guessing decoders is a scheduling diagnostic, "not part of the result" (include/swd.h)
            a, b = a[:, :, :7], b[:, :, :7]
        assert np.array_equal(a, b), name


# ---- 2. plans the pipeline takes: the device loop equals the one launch -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bb72_pipeline(geometry):
    """(plan, det, what the one-launch pipeline returns) for 192 shots of ``DemSampler.sample``; shared, read-only"""
    from slidingwindowdecoder_amd import DemSampler, SlidingWindowDecoder
    plan = bb72_plan(*geometry)
    det = DemSampler(plan.chk, plan.obs, plan.priors).sample(192)[0]
    dec = SlidingWindowDecoder(plan, **KW_BB)
    assert dec.window_loop == "pipeline" and dec._loop is None
    return plan, _frozen(det)[0], _decode(dec, det)


@pytest.mark.parametrize("force_huge", [False, True])
@pytest.mark.parametrize("geometry", [(5, 3, 1), (6, 3, 2)])
def test_bb72_equals_the_one_launch_pipeline(geometry, force_huge, monkeypatch):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, det, want = bb72_pipeline(geometry)
    if force_huge:
        monkeypatch.setenv("SWD_FORCE_HUGE", "1")
    dec = SlidingWindowDecoder(plan, window_loop="device", **KW_BB)
    assert dec.window_loop == "device" and dec.W == len(plan.windows)
    if geometry == (5, 3, 1):
        assert dec.W == 4 and dec.distinct_windows == 3
    total, stats, min_pm, oflips, flagged = _decode(dec, det)
    assert np.array_equal(total, want[0])
    assert np.array_equal(stats[:, :, :2], want[1][:, :, :2])
    assert np.array_equal(min_pm, want[2])
    assert np.array_equal(oflips, want[3]) and np.array_equal(flagged, want[4])
    assert len(set((stats[:, :, 0] & 7).ravel().tolist())) >= 2 and oflips.any()


# ---- 3. decode_device: the caller's buffers, streams of its own ---------------------------------------------------------------
def test_decode_device_with_caller_buffers_and_alternating_streams():
    import torch
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, (det, obs, flips) = overlap_plan(4), overlap_shots(4)
    want = host_loop()
    dev = torch.device("cuda", 0)
    dec = SlidingWindowDecoder(plan, window_loop="device", **KW)
    B, W, ncol = len(det), len(plan.windows), plan.chk.shape[1]
    d = torch.from_numpy(det.copy()).to(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    # caller buffers (a padded total: the stride is honoured and the padding left alone) on a stream that is not the default
    total = torch.full((B, ncol + 24), 7, dtype=torch.uint8, device=dev)
    stats = torch.full((B, W, 8), -1, dtype=torch.int32, device=dev)
    shot = torch.full((B, 2), -1, dtype=torch.int32, device=dev)
    s1.wait_stream(torch.cuda.current_stream(dev))
    s2.wait_stream(torch.cuda.current_stream(dev))
    out = dec.decode_device(d, total=total[:, :ncol], stats=stats, shot_result=shot, stream=s1)
    assert out[0].data_ptr() == total.data_ptr() and out[1] is stats and out[2].shape == (B, W)
    # a second decode of other shots on another stream at once, then the first stream again: one handle, shared buffers
    half = B // 2
    out2 = dec.decode_device(d[half:], stream=s2)
    shot3 = torch.full((half, 2), -1, dtype=torch.int32, device=dev)
    out3 = dec.decode_device(d[:half], shot_result=shot3, stream=s1, want_stats=False)
    s1.synchronize()
    s2.synchronize()
    dec.check_status()
    assert np.array_equal(d.cpu().numpy(), det)  # the caller's detectors are not modified
    t = total.cpu().numpy()
    assert np.array_equal(t[:, :ncol], want[0]) and (t[:, ncol:] == 7).all()
    assert np.array_equal(stats.cpu().numpy(), want[1]) and np.array_equal(out[2].cpu().numpy(), want[2])
    sr = shot.cpu().numpy()
    assert np.array_equal(sr[:, 0].astype(np.uint32), want[3]) and np.array_equal(sr[:, 1].astype(bool), want[4])
    assert np.array_equal(out2[0].cpu().numpy(), want[0][half:]) and np.array_equal(out2[1].cpu().numpy(), want[1][half:])
    assert np.array_equal(out2[2].cpu().numpy(), want[2][half:])
    # want_stats=False: no records, the faults and the per-shot result all the same
    assert out3[1] is None and out3[2] is None
    assert np.array_equal(out3[0].cpu().numpy(), want[0][:half])
    sr3 = shot3.cpu().numpy()
    assert np.array_equal(sr3[:, 0].astype(np.uint32), want[3][:half]) and np.array_equal(sr3[:, 1].astype(bool), want[4][:half])


# ---- 4. MemoryExperiment ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def experiment_spec():
    """(experiment on ``overlap_plan(4)``, ``memory_experiment_host`` with the oracle on ``sampler.sample(96)``)"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import MemoryExperiment
    from slidingwindowdecoder_amd.windows import memory_experiment_host
    plan = overlap_plan(4)
    exp = MemoryExperiment(plan, window_loop="device", **KW)
    det, obs = exp.sampler.sample(SHOTS)
    return exp, memory_experiment_host(plan, det, obs, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW))


@pytest.mark.parametrize("lanes", [1, 2])
def test_memory_experiment_on_the_overlap_plan_equals_the_oracle(lanes):
    from tests.test_memory_experiment_host import as_result
    exp, spec = experiment_spec()
    assert exp.decoder.window_loop == "device"
    assert 0 < spec["logical_errors"] < SHOTS
    res = exp.run(SHOTS, batch=40, lanes=lanes, keep_failures=SHOTS)
    assert exp._stream is None  # no stream object: the lanes are torch streams that call decode_device
    assert res == as_result(spec), (res, as_result(spec))
    assert np.array_equal(np.sort(res.failed_shots), np.flatnonzero(spec["result"] & 1))


def test_memory_experiment_bb_equals_the_pipeline_experiment():
    from slidingwindowdecoder_amd import MemoryExperiment
    a = MemoryExperiment.bb(72, 0.004, 4, 3, 1, window_loop="device", **KW_BB)
    b = MemoryExperiment.bb(72, 0.004, 4, 3, 1, **KW_BB)
    assert a.decoder.window_loop == "device" and b.decoder.window_loop == "pipeline"
    ra, rb = a.run(256, keep_failures=256), b.run(256, keep_failures=256)
    assert ra == rb and rb == ra and ra.shots == 256
    assert np.array_equal(np.sort(ra.failed_shots), np.sort(rb.failed_shots))
    assert np.array_equal(ra.window_exit_classes, rb.window_exit_classes) and np.array_equal(ra.window_bp_iterations, rb.window_bp_iterations)


# ---- 5. what the device loop does not serve ------------------------------------------------------------------------------------
def test_refusals_and_errors():
    import torch
    from slidingwindowdecoder_amd import MemoryExperiment, RollingMemoryExperiment, SlidingWindowDecoder
    plan = overlap_plan(4)
    with pytest.raises(ValueError, match="window_loop"):
        SlidingWindowDecoder(plan, window_loop="gpu", **KW)
    dec = SlidingWindowDecoder(plan, window_loop="device", **KW)
    for what, call in ((r"stream\(\)", lambda: dec.stream(8)), (r"session\(\)", lambda: dec.session(8)),
                       (r"rolling_session\(\)", lambda: dec.rolling_session(8)),
                       (r"measurement_session\(\)", lambda: dec.measurement_session(8, None)),
                       (r"rolling_measurement_session\(\)", lambda: dec.rolling_measurement_session(8, None)),
                       (r"stream\(\)", lambda: next(dec.decode_stream([overlap_shots(4)[0]])))):
        with pytest.raises(RuntimeError, match=what + " needs the one-launch pipeline"):
            call()
    with pytest.raises(RuntimeError, match="RollingMemoryExperiment needs the one-launch pipeline"):
        RollingMemoryExperiment(bb72_plan(6, 3, 1), window_loop="device", **KW_BB)
    # the default experiment on a plan beyond the pipeline keeps refusing, and now says what serves it
    with pytest.raises(RuntimeError, match="MemoryExperiment needs the one-launch pipeline") as e:
        MemoryExperiment(plan, **KW)
    assert 'window_loop="device"' in str(e.value)
    # tensors on the wrong device
    d = torch.from_numpy(overlap_shots(4)[0][:4].copy())
    with pytest.raises(ValueError, match="det lives on cpu"):
        dec.decode_device(d)
    with pytest.raises(ValueError, match="total lives on cpu"):
        dec.decode_device(d.to("cuda:0"), total=torch.empty((4, plan.chk.shape[1]), dtype=torch.uint8))
    # the keyword is no decoder kwarg: the host loop's window decoders do not see it
    assert SlidingWindowDecoder(plan, window_loop="host", **KW).window_loop == "host"
