"""Memory experiments on the device: the per-shot accounting kernel (swd_shot_account_dev) against numpy on synthetic tensors,
``SlidingWindowStream.wait_last``, and ``MemoryExperiment`` end to end against the host restatement
(``windows.memory_experiment_host`` with the oracle, tests/test_memory_experiment_host.py), the Philox restatement of the sampler
and the one-launch ``decode`` -- never against the experiment itself."""
import functools

import numpy as np
import pytest

from tests.test_memory_experiment_host import PARAMS, SEED, SHOTS, as_result, plan_for, sample, specification

pytestmark = pytest.mark.gpu
WORDS = 10  # include/swd.h: SWD_WINDOW_COUNTER_WORDS


# ---- 1. the accounting kernel alone ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic(B, W, seed=5):
    """random decisions and records: (shot_result [B, 2], true_flips [B], stats [B, W, 8]); a quarter of the shots flagged, a
    quarter with other observable flips than the true ones; exit classes 0-6, converge bit random, 0-200 iterations; the words the
    kernel must not read are filled with large values"""
    rng = np.random.default_rng([seed, B, W])
    flips = rng.integers(0, 2 ** 32, B, dtype=np.uint64).astype(np.uint32)
    pred = np.where(rng.random(B) < 0.25, rng.integers(0, 2 ** 32, B, dtype=np.uint64).astype(np.uint32), flips)
    shot = np.stack([pred.view(np.int32), (rng.random(B) < 0.25) * rng.integers(1, 9, B)], axis=1).astype(np.int32)
    stats = rng.integers(2 ** 20, 2 ** 30, (B, W, 8)).astype(np.int32)
    stats[:, :, 0] = rng.integers(0, 7, (B, W)) | (rng.integers(0, 2, (B, W)) << 8)
    stats[:, :, 1] = rng.integers(0, 201, (B, W))
    for a in (shot, flips, stats):
        a.setflags(write=False)
    return shot, flips, stats


def numpy_account(shot, flips, stats=None):
    flagged, wrong = shot[:, 1] != 0, shot[:, 0].view(np.uint32) != flips
    word = ((flagged | wrong).astype(np.int32) | (flagged.astype(np.int32) << 1) | (wrong.astype(np.int32) << 2))
    counters = np.array([len(shot), (word & 1).sum(), flagged.sum(), wrong.sum()], np.int64)
    win = None
    if stats is not None:
        W = stats.shape[1]
        win = np.zeros((W, WORDS), np.int64)
        for t in range(W):
            win[t, :8] = np.bincount(stats[:, t, 0] & 7, minlength=8)
            win[t, 8] = ((stats[:, t, 0] & 0x100) == 0).sum()
            win[t, 9] = stats[:, t, 1].astype(np.int64).sum()
    return word, counters, win


def device_account(shot, flips, stats, first_shot=0, want=("result", "counters", "window_counters"), cap=None, into=None):
    """one launch on numpy inputs -> dict of the outputs asked for (``into``: device tensors of an earlier call, to be added to)"""
    import torch
    from slidingwindowdecoder_amd.decoders import shot_account_device
    dev = torch.device("cuda", 0)
    B = shot.shape[0]
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731  (a writable copy of the shared arrays)
    out = dict(into or {})
    if "result" in want:
        out.setdefault("result", torch.full((B,), -1, dtype=torch.int32, device=dev))
    if "counters" in want:
        out.setdefault("counters", torch.zeros(4, dtype=torch.int64, device=dev))
    if "window_counters" in want and stats is not None:
        out.setdefault("window_counters", torch.zeros((stats.shape[1], WORDS), dtype=torch.int64, device=dev))
    if cap is not None:
        out.setdefault("failed", torch.zeros(1 + cap, dtype=torch.int64, device=dev))
    shot_account_device(t(shot), t(flips.view(np.int32)), t(stats) if stats is not None else None, first_shot, **out)
    torch.cuda.synchronize()
    return out


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("B,W", [(0, 1), (0, 5), (1, 1), (1, 5), (257, 1), (257, 5), (2048 * 256 + 257, 2), (300, 70)])
def test_accounting_equals_numpy(B, W):
    """B = 2048 * 256 + 257: the grid-stride loop runs twice, the second pass with two live workgroups, the last of them
    partial; W = 70: more windows than the 64 a workgroup keeps in LDS at a time"""
    shot, flips, stats = synthetic(B, W)
    word, counters, win = numpy_account(shot, flips, stats)
    got = host(device_account(shot, flips, stats, cap=B + 3, first_shot=11))
    assert np.array_equal(got["result"], word)
    assert np.array_equal(got["counters"], counters), (got["counters"], counters)
    assert np.array_equal(got["window_counters"], win)
    failed = got["failed"].view(np.uint64)
    assert failed[0] == counters[1] and np.array_equal(np.sort(failed[1:1 + counters[1]]), np.flatnonzero(word & 1).astype(np.uint64) + np.uint64(11))
    assert not failed[1 + counters[1]:].any()
    if B > 1:
        assert 0 < counters[2] < counters[1] < B and 0 < counters[3] < counters[1] and (win[:, :7] > 0).all() and not win[:, 7].any()


def test_accounting_optional_outputs_and_accumulation():
    """stats, result and counters each left out alone; two calls ADD: counters, window counters and the failed list of two batches"""
    shot, flips, stats = synthetic(257, 5)
    word, counters, win = numpy_account(shot, flips, stats)
    got = host(device_account(shot, flips, None))
    assert np.array_equal(got["result"], word) and np.array_equal(got["counters"], counters) and "window_counters" not in got
    got = host(device_account(shot, flips, stats, want=("counters", "window_counters")))
    assert np.array_equal(got["counters"], counters) and np.array_equal(got["window_counters"], win)
    got = host(device_account(shot, flips, stats, want=("result", "window_counters")))
    assert np.array_equal(got["result"], word) and np.array_equal(got["window_counters"], win)
    shot2, flips2, stats2 = synthetic(300, 5, seed=6)
    word2, counters2, win2 = numpy_account(shot2, flips2, stats2)
    first = device_account(shot, flips, stats, cap=600, first_shot=0)
    first.pop("result")
    both = host(device_account(shot2, flips2, stats2, cap=600, first_shot=257, into=first))
    assert np.array_equal(both["counters"], counters + counters2) and np.array_equal(both["window_counters"], win + win2)
    failed, n = both["failed"].view(np.uint64), counters[1] + counters2[1]
    want = np.concatenate([np.flatnonzero(word & 1), 257 + np.flatnonzero(word2 & 1)]).astype(np.uint64)
    assert failed[0] == n and np.array_equal(np.sort(failed[1:1 + n]), want) and np.array_equal(both["result"], word2)


def test_accounting_failed_list_overflow_and_large_shot_numbers():
    """cap 3 below the number of failing shots: the count is whole, every stored number is a failing shot, none twice; shot
    numbers above 2^32 keep their high word"""
    shot, flips, stats = synthetic(257, 1)
    word, counters, _ = numpy_account(shot, flips)
    n, first = int(counters[1]), 2 ** 32 + 5
    assert n > 6
    failing = np.flatnonzero(word & 1).astype(np.uint64) + np.uint64(first)
    failed = host(device_account(shot, flips, None, first_shot=first, cap=n - 3))["failed"].view(np.uint64)
    assert failed.shape == (1 + n - 3,) and failed[0] == n
    assert np.isin(failed[1:], failing).all() and len(np.unique(failed[1:])) == n - 3
    whole = host(device_account(shot, flips, None, first_shot=first, cap=n))["failed"].view(np.uint64)
    assert whole[0] == n and np.array_equal(np.sort(whole[1:]), failing) and (whole[1:] >> np.uint64(32) == 1).all()
    none = host(device_account(shot, flips, None, first_shot=first, cap=0))["failed"].view(np.uint64)
    assert none.tolist() == [n]


# ---- 2. wait_last ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decoder(kw="KW"):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    return SlidingWindowDecoder(plan_for(), **PARAMS[kw])


@functools.lru_cache(maxsize=None)
def one_launch(kw="KW", shots=SHOTS):
    """what ``decode`` leaves for the first ``shots`` shots of the sampler's stream: (total, stats, obs_flips, flagged); read-only"""
    dec = decoder(kw)
    det = sample(plan_for(), shots)[0]
    total = dec.decode(det).copy()
    ref = (total, dec.last_stats.copy(), dec.last_obs_flips.copy(), dec.last_flagged.copy())
    for a in ref:
        a.setflags(write=False)
    return ref


def test_wait_last_orders_a_consumer_behind_its_own_batch():
    import torch
    dec, dev = decoder(), torch.device("cuda", 0)
    det = sample(plan_for(), SHOTS)[0]
    total = one_launch()[0]
    st = dec.stream(96)
    with pytest.raises(RuntimeError, match="nothing has been pushed"):
        st.wait_last(torch.cuda.current_stream(dev))
    halves = [(0, 96), (96, SHOTS)]
    d = [torch.from_numpy(np.array(det[a:b])).to(dev) for a, b in halves]
    out = [torch.zeros((b - a, dec.num_col), dtype=torch.uint8, device=dev) for a, b in halves]
    copy = [torch.zeros_like(o) for o in out]
    lanes = [torch.cuda.Stream(dev) for _ in halves]
    torch.cuda.synchronize()
    for k, s in enumerate(lanes):
        st.push_device(d[k], out[k], after=s)
        st.wait_last(s)
        with torch.cuda.stream(s):
            copy[k].copy_(out[k], non_blocking=True)
    for s in lanes:
        s.synchronize()
    dec.check_status()
    for (a, b), c in zip(halves, copy):
        assert np.array_equal(c.cpu().numpy(), total[a:b])
    st.close()


# ---- 3 - 8. the experiment --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def experiment(kw="KW"):
    from slidingwindowdecoder_amd import MemoryExperiment
    return MemoryExperiment(plan_for(), **PARAMS[kw])


def window_counts(stats):
    """numpy's reduction of [B, W, 8] records -> (exit classes [W, 8], not converged [W], iterations [W])"""
    W = stats.shape[1]
    return (np.stack([np.bincount(stats[:, t, 0] & 7, minlength=8) for t in range(W)]), ((stats[:, :, 0] & 0x100) == 0).sum(axis=0),
            stats[:, :, 1].astype(np.int64).sum(axis=0))


def test_run_batch_equals_the_specification():
    plan, det, obs, flips, spec = specification("KW")
    got = experiment("KW").run_batch(SHOTS, seed=SEED, first_shot=0)
    assert np.array_equal(got["det"], det) and got["true_flips"].dtype == np.uint32 and np.array_equal(got["true_flips"], flips)
    assert np.array_equal(got["total"], spec["total_e_hat"])
    assert np.array_equal(got["result"], spec["result"])
    assert got["stats"].shape == (SHOTS, len(plan.windows), 8) and got["shot_result"].shape == (SHOTS, 2)
    assert ((got["result"] & 5) == 5).any() and not (got["result"] & 2).any()  # observable mismatches on unflagged shots


@pytest.mark.parametrize("kw", ["KW", "KW_NO_OSD"])
def test_run_equals_the_specification(kw):
    spec = specification(kw)[4]
    total, stats, pred, flagged = one_launch(kw)
    res = experiment(kw).run(SHOTS, batch=64, keep_failures=SHOTS)
    want = as_result(spec)
    print(res, want)
    for name in ("shots", "logical_errors", "flagged", "observable_mismatches", "failed_shots_complete"):
        assert getattr(res, name) == getattr(want, name), name
    for name in ("window_exit_classes", "window_not_converged", "window_bp_iterations", "failed_shots"):
        assert np.array_equal(getattr(res, name), getattr(want, name)), name
    assert res == want
    cls, ncv, its = window_counts(stats)
    assert np.array_equal(res.window_exit_classes, cls) and np.array_equal(res.window_not_converged, ncv)
    assert np.array_equal(res.window_bp_iterations, its)
    assert res.flagged == flagged.sum() and res.ler == spec["logical_errors"] / SHOTS
    if kw == "KW_NO_OSD":
        assert 0 < res.observable_mismatches < res.flagged <= res.logical_errors < SHOTS


def test_result_is_a_pure_function_of_seed_and_shot_numbers():
    exp = experiment("KW_NO_OSD")
    want = as_result(specification("KW_NO_OSD")[4])
    for batch in (1, 64, 160):
        for lanes in (1, 2):
            assert exp.run(SHOTS, batch=batch, lanes=lanes, keep_failures=SHOTS) == want, (batch, lanes)
    a, b = exp.run(100, keep_failures=SHOTS), exp.run(60, first_shot=100, keep_failures=SHOTS)
    assert a.shots == 100 and b.shots == 60 and (b.failed_shots >= 100).all() and (a.failed_shots < 100).all()
    for name in ("shots", "logical_errors", "flagged", "observable_mismatches", "window_exit_classes", "window_not_converged",
                 "window_bp_iterations"):
        assert np.array_equal(getattr(a, name) + getattr(b, name), getattr(want, name)), name
    assert np.array_equal(np.concatenate([a.failed_shots, b.failed_shots]), want.failed_shots)
    assert a.failed_shots_complete and b.failed_shots_complete and a + b == want
    # without window statistics and without the list: the counters alone; a list too short is marked incomplete
    bare = exp.run(SHOTS, batch=64, window_stats=False)
    assert bare.window_exit_classes is None and bare.window_not_converged is None and bare.window_bp_iterations is None
    assert (bare.shots, bare.logical_errors, bare.flagged, bare.observable_mismatches) == \
        (want.shots, want.logical_errors, want.flagged, want.observable_mismatches)
    assert len(bare.failed_shots) == 0 and not bare.failed_shots_complete
    short = exp.run(SHOTS, batch=64, keep_failures=7)
    assert len(short.failed_shots) == 7 and not short.failed_shots_complete and np.isin(short.failed_shots, want.failed_shots).all()
    assert len(np.unique(short.failed_shots)) == 7
    other = exp.run(SHOTS, seed=SEED + 1, keep_failures=SHOTS)
    assert other != want and other.shots == SHOTS


def test_max_errors_stops_after_a_round_of_lanes():
    total, stats, pred, flagged = one_launch("KW_NO_OSD", 128)
    flips = sample(plan_for(), 128)[2]
    wrong = pred != flips
    assert (flagged[:64] | wrong[:64]).sum() < 50 <= (flagged | wrong).sum()  # one batch is not enough, the first round of two is
    res = experiment("KW_NO_OSD").run(1024, batch=64, lanes=2, max_errors=50)
    assert res.shots == 128
    assert (res.logical_errors, res.flagged, res.observable_mismatches) == ((flagged | wrong).sum(), flagged.sum(), wrong.sum())
    cls, ncv, its = window_counts(stats)
    assert np.array_equal(res.window_exit_classes, cls) and np.array_equal(res.window_not_converged, ncv)


def test_guessing_decoder_windows():
    """bpgdg_decoder in the windows (parameters of tests/test_gpu_unaligned_rounds.py::test_guessing_decoder_windows), 24 shots:
    the counters against the one-launch ``decode`` of the same sampled shots (statistics words 0 and 1 only)"""
    from slidingwindowdecoder_amd import MemoryExperiment, SlidingWindowDecoder
    from tests import fixtures as fx
    kw = fx.params(fx.load("bb72_capacity.npz"), "gdg_params")
    kw.pop("multi_thread", None)
    plan = plan_for()
    det, obs, flips = sample(plan, 24)
    dec = SlidingWindowDecoder(plan, decoder="bpgdg_decoder", **kw)
    dec.decode(det)
    wrong, flagged = dec.last_obs_flips != flips, dec.last_flagged
    res = MemoryExperiment(plan, decoder="bpgdg_decoder", **kw).run(24, batch=16, keep_failures=24)
    assert (res.shots, res.logical_errors, res.flagged, res.observable_mismatches) == (24, (wrong | flagged).sum(), flagged.sum(), wrong.sum())
    assert np.array_equal(res.failed_shots, np.flatnonzero(wrong | flagged)) and res.failed_shots_complete
    cls, ncv, its = window_counts(dec.last_stats)
    assert np.array_equal(res.window_exit_classes, cls) and np.array_equal(res.window_not_converged, ncv)
    assert np.array_equal(res.window_bp_iterations, its)


def test_constructor_errors_and_the_bb_shortcut(monkeypatch):
    import dataclasses

    import scipy.sparse as sp

    from slidingwindowdecoder_amd import MemoryExperiment
    plan = plan_for()
    kw = PARAMS["KW"]
    with pytest.raises(ValueError, match="needs observables"):
        MemoryExperiment(dataclasses.replace(plan, obs=plan.obs[:0]), **kw)
    with pytest.raises(ValueError, match="needs observables"):
        MemoryExperiment(dataclasses.replace(plan, obs=None), **kw)
    with pytest.raises(ValueError, match="at most 32 observables"):
        MemoryExperiment(dataclasses.replace(plan, obs=sp.vstack([plan.obs, plan.obs, plan.obs], format="csr")), **kw)
    exp = experiment("KW")
    for bad in (dict(lanes=3), dict(lanes=0), dict(batch=0), dict(keep_failures=-1)):
        with pytest.raises(ValueError):
            exp.run(8, **bad)
    empty = exp.run(0, keep_failures=4)
    assert empty.shots == 0 and empty.logical_errors == 0 and empty.failed_shots_complete and not empty.window_exit_classes.any()
    short = MemoryExperiment.bb(72, 0.004, 6, 3, 1, **kw)
    assert (short.plan.chk != plan.chk).nnz == 0 and (short.plan.obs != plan.obs).nnz == 0 and np.array_equal(short.plan.priors, plan.priors)
    assert [(w.row0, w.row1, w.col0, w.commit) for w in short.plan.windows] == [(w.row0, w.row1, w.col0, w.commit) for w in plan.windows]
    assert np.array_equal(short.run_batch(16)["result"], specification("KW")[4]["result"][:16])
    # a plan that runs as a host window loop (tests/test_gpu_session.py: windows beyond every pipeline kernel, general-form decoders)
    from tests.test_gpu_session import _tiny_host_loop_plan
    monkeypatch.setenv("SWD_FORCE_HUGE", "1")
    with pytest.raises(RuntimeError, match="MemoryExperiment needs the one-launch pipeline"):
        MemoryExperiment(_tiny_host_loop_plan(), pre_max_iter=4, post_max_iter=8, osd_method="osd_0")
