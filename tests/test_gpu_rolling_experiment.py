"""Rolling memory experiments on the device: the rolling DEM sampler (swd_rolling_sampler_*, ``RollingDemSampler``) against
``DemSampler`` on the plan of the experiment's own length and against the numpy restatement of
tests/test_rolling_experiment_host.py, and ``RollingMemoryExperiment`` against ``MemoryExperiment`` on that plan and its one-launch
``decode`` -- never against the rolling code itself.  [[72,12,6]], p = 0.004, at most 96 shots (257 for the partial workgroups of
the sampler alone)."""
import copy
import dataclasses
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_gpu_rolling import KW_NO_OSD
from tests.test_rolling_experiment_host import chunked, handmade, rows_ref, whole_ref
from tests.test_rolling_host import TEMPLATES, plan_for, template_plan
from tests.test_session_host import KW

pytestmark = pytest.mark.gpu
H, SEED, SHOTS, FIRST = 36, 20240318, 96, 2 ** 32 + 5
PARAMS = {"KW": KW, "KW_NO_OSD": KW_NO_OSD}


def bits(flips, num_obs):
    return ((np.asarray(flips, np.uint32)[:, None] >> np.arange(num_obs, dtype=np.uint32)) & 1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def rolling_sampler(tag):
    from slidingwindowdecoder_amd import RollingDemSampler
    return RollingDemSampler(template_plan(tag))


@functools.lru_cache(maxsize=None)
def template(tag):
    from slidingwindowdecoder_amd.windows import rolling_template
    return rolling_template(template_plan(tag))


@functools.lru_cache(maxsize=None)
def dem_reference(tag, rounds, shots=SHOTS, first_shot=FIRST):
    """``DemSampler`` on the plan of ``rounds`` rounds: (det, obs, faults); shared, read-only"""
    from slidingwindowdecoder_amd import DemSampler
    plan = plan_for(tag, rounds)
    ref = DemSampler(plan.chk, plan.obs, plan.priors).sample(shots, seed=SEED, first_shot=first_shot, return_faults=True)
    for a in ref:
        a.setflags(write=False)
    return ref


def device_rows(sampler, shots, rounds, pieces, first_shot=FIRST, seed=SEED, want_faults=True, want_flips=True, pad=0):
    """the experiment assembled from ``rows_device`` calls over ``pieces`` = [(block0, nblocks)]: (det, flips uint32, faults); ``pad``:
    every call writes into a column slice, ``pad`` bytes in, of a tensor ``2 * pad`` wider than its rows (0xEE elsewhere)"""
    import torch
    h = sampler.n_half
    det = np.zeros((shots, (rounds + 1) * h), np.uint8)
    faults = np.zeros((shots, sampler.columns(rounds)[1]), np.uint8)
    flips = torch.zeros(shots, dtype=torch.int32, device="cuda") if want_flips else None
    for b0, n in pieces:
        c0, nc = sampler.columns(rounds, b0, n)
        wide = torch.full((shots, n * h + 2 * pad), 0xEE, dtype=torch.uint8, device="cuda")
        fa = torch.full((shots, nc), 0xEE, dtype=torch.uint8, device="cuda") if want_faults else None
        out = sampler.rows_device(shots, rounds, b0, n, seed=seed, first_shot=first_shot, out=wide[:, pad:pad + n * h], flips=flips, faults=fa)
        torch.cuda.synchronize()
        assert out.data_ptr() == wide.data_ptr() + pad
        w = wide.cpu().numpy()
        assert (w[:, :pad] == 0xEE).all() and (w[:, pad + n * h:] == 0xEE).all()
        det[:, b0 * h:(b0 + n) * h] = w[:, pad:pad + n * h]
        if want_faults:
            faults[:, c0:c0 + nc] = fa.cpu().numpy()
    return det, flips.cpu().numpy().view(np.uint32) if want_flips else None, faults


# ---- 1. the whole experiment against DemSampler on the plan of its own length and against the restatement -----------------------------
@pytest.mark.parametrize("tag", sorted(TEMPLATES))
def test_sample_equals_dem_sampler_of_the_long_plan_and_the_restatement(tag):
    from slidingwindowdecoder_amd.windows import extend_template
    W, F, method, R0 = TEMPLATES[tag]
    T, rs = template(tag), rolling_sampler(tag)
    assert (rs.n_half, rs.num_obs, rs.R0, rs.min_rounds) == (H, 12, R0, T.min_rounds)
    for R in (T.min_rounds, R0, R0 + F, R0 + 5 * F):
        det, obs, faults = dem_reference(tag, R)
        got = rs.sample(SHOTS, R, seed=SEED, first_shot=FIRST, return_faults=True)
        assert got[0].shape == (SHOTS, (R + 1) * H) and got[2].shape == faults.shape == (SHOTS, plan_for(tag, R).chk.shape[1])
        assert np.array_equal(got[2], faults), (tag, R)
        assert np.array_equal(got[0], det) and np.array_equal(got[1], obs), (tag, R)
        rdet, rflips, rfaults = whole_ref(extend_template(T, R), SHOTS, SEED, FIRST)
        assert np.array_equal(got[2], rfaults) and np.array_equal(got[0], rdet) and np.array_equal(got[1], bits(rflips, 12)), (tag, R)
        assert det.any() and obs.any() and len(rs.sample(SHOTS, R, seed=SEED, first_shot=FIRST)) == 2
    low = rs.sample(8, R0, seed=SEED, first_shot=5, return_faults=True)  # the high counter word matters
    assert not np.array_equal(low[2], dem_reference(tag, R0)[2][:8])


# ---- 2. chunk invariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,rounds", [("w3f1m1", 9), ("w4f2m1", 12), ("w3f3m0", 12)])
def test_rows_do_not_depend_on_how_the_blocks_are_cut(tag, rounds):
    """one block at a time and F at a time draw two or F + 1 column blocks a call (a wave per shot); the uneven pieces and the whole
    experiment in one call reach the launches of seven row blocks, whose columns exceed what a wave takes (a workgroup per shot)"""
    F = TEMPLATES[tag][1]
    rs = rolling_sampler(tag)
    det, obs, faults = dem_reference(tag, rounds)
    nb = rounds + 1
    assert rs.columns(rounds, 0, 2)[1] <= 2048 < rs.columns(rounds, 0, 8)[1]
    by_f = [(b, min(F, nb - b)) for b in range(0, nb, F)]
    for pieces in (chunked(nb, "ones"), by_f, chunked(nb, "uneven"), [(0, nb)], [(0, 8), (8, nb - 8)]):
        gdet, gflips, gfaults = device_rows(rs, SHOTS, rounds, pieces)
        assert np.array_equal(gdet, det), pieces
        assert np.array_equal(gfaults, faults), pieces
        assert np.array_equal(bits(gflips, 12), obs), pieces
    # a sweep in another order, and one block drawn twice: the masks XOR in once per call
    gdet, gflips, _ = device_rows(rs, SHOTS, rounds, chunked(nb, "uneven")[::-1])
    assert np.array_equal(gdet, det) and np.array_equal(bits(gflips, 12), obs)
    _, twice, _ = device_rows(rs, SHOTS, rounds, [(3, 2), (3, 2)])
    assert not twice.any()


# ---- 3. partial workgroups, strides, optional outputs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 5, 257])
def test_partial_workgroups_strided_rows_and_optional_outputs(B):
    rs = rolling_sampler("w3f1m1")
    det, obs, faults = dem_reference("w3f1m1", 9, 257)
    pieces = [(0, 3), (3, 1), (4, 6)]  # (the last piece: a workgroup per shot, B = 5 and 257 leave a ragged grid in both forms)
    gdet, gflips, gfaults = device_rows(rs, B, 9, pieces, pad=5)
    assert np.array_equal(gdet, det[:B]) and np.array_equal(gfaults, faults[:B]) and np.array_equal(bits(gflips, 12), obs[:B])
    gdet, gflips, _ = device_rows(rs, B, 9, pieces, want_faults=False, want_flips=False, pad=3)
    assert np.array_equal(gdet, det[:B]) and gflips is None
    # shots past the batch were not touched: flips of a longer tensor
    import torch
    flips = torch.full((B + 4,), 77, dtype=torch.int32, device="cuda")
    flips[:B] = 0
    rs.rows_device(B, 9, 0, 10, seed=SEED, first_shot=FIRST, flips=flips[:B])
    torch.cuda.synchronize()
    assert (flips[B:] == 77).all() and np.array_equal(bits(flips[:B].cpu().numpy().view(np.uint32), 12), obs[:B])


# ---- 4. the unaligned hand-made model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rounds", [2, 5, 11])
def test_unaligned_handmade_model_equals_the_restatement(rounds):
    from slidingwindowdecoder_amd import RollingDemSampler
    from slidingwindowdecoder_amd.windows import extend_periodic, extended_block_cols
    chk, obs, priors, h, j0, j1, cols = handmade()
    rs = RollingDemSampler.from_blocks(chk, obs, priors, h, j0, j1, cols)
    assert (rs.n_half, rs.num_obs, rs.R0, rs.min_rounds) == (5, 3, 5, 2)
    ext, bc = extend_periodic(chk, obs, priors, h, j0, j1, cols, rounds), extended_block_cols(cols, j0, j1, rounds)
    shots = 70
    det, flips, faults = whole_ref(ext, shots, 99, FIRST)
    got = rs.sample(shots, rounds, seed=99, first_shot=FIRST, return_faults=True)
    assert np.array_equal(got[2], faults) and np.array_equal(got[0], det) and np.array_equal(got[1], bits(flips, 3))
    for kind in ("ones", "twos", "uneven"):
        pieces = chunked(rounds + 1, kind)
        gdet, gflips, gfaults = device_rows(rs, shots, rounds, pieces, seed=99, pad=1)
        assert np.array_equal(gdet, det) and np.array_equal(gfaults, faults) and np.array_equal(gflips, flips), kind
        for b0, n in pieces:  # call by call: the rows, the masks and the faults of that call alone
            rows, fl, fa = rows_ref(ext, bc, h, b0, n, shots, 99, FIRST)
            one = device_rows(rs, shots, rounds, [(b0, n)], seed=99)
            assert np.array_equal(one[0][:, b0 * h:(b0 + n) * h], rows) and np.array_equal(one[1], fl)
            assert np.array_equal(one[2][:, bc[b0]:bc[b0 + n]], fa)
    assert faults.all(axis=0).sum() == 0 and faults.any(axis=0).all()  # every column faults in some shot, boundary columns included


# ---- 5. the experiment against MemoryExperiment on the plan of its own length -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rolling_experiment(tag, kw="KW"):
    from slidingwindowdecoder_amd import RollingMemoryExperiment
    return RollingMemoryExperiment(template_plan(tag), **PARAMS[kw])


@functools.lru_cache(maxsize=None)
def long_experiment(tag, rounds, kw="KW"):
    from slidingwindowdecoder_amd import MemoryExperiment
    return MemoryExperiment(plan_for(tag, rounds), **PARAMS[kw])


@functools.lru_cache(maxsize=None)
def long_result(tag, rounds, kw="KW", shots=SHOTS, first_shot=0):
    return long_experiment(tag, rounds, kw).run(shots, first_shot=first_shot, keep_failures=shots)


def assert_same_experiment(res, want, rounds, windows):
    print(res, want)
    assert (res.rounds, res.windows_per_shot) == (rounds, windows) and len(want.window_not_converged) == windows
    for name in ("shots", "logical_errors", "flagged", "observable_mismatches"):
        assert getattr(res, name) == getattr(want, name), name
    for name in ("window_exit_classes", "window_not_converged", "window_bp_iterations"):
        a, b = getattr(res, name), getattr(want, name)
        assert a.shape[0] == 3 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1:-1].sum(axis=0)) and np.array_equal(a[2], b[-1]), name
    assert res.ler == want.ler and res.ler_per_round() == want.ler_per_round(rounds)


@pytest.mark.parametrize("tag,rounds,kw", [("w3f1m1", 9, "KW_NO_OSD"), ("w3f1m1", 9, "KW"), ("w4f2m1", 10, "KW")])
def test_run_equals_memory_experiment_of_the_long_plan(tag, rounds, kw):
    want = long_result(tag, rounds, kw)
    exp = rolling_experiment(tag, kw)
    res = exp.run(SHOTS, rounds=rounds, keep_failures=SHOTS)
    assert_same_experiment(res, want, rounds, len(plan_for(tag, rounds).windows))
    assert np.array_equal(res.failed_shots, want.failed_shots) and res.failed_shots_complete
    if kw == "KW_NO_OSD":
        assert 0 < res.observable_mismatches < res.flagged <= res.logical_errors < SHOTS  # most shots end flagged
    else:
        assert res.logical_errors > 0
    # run_batch: the per-shot arrays against the one-launch decode of the long plan on DemSampler's shots
    ref = long_experiment(tag, rounds, kw).run_batch(SHOTS)
    got = exp.run_batch(SHOTS, rounds=rounds)
    assert np.array_equal(got["det"], ref["det"]) and got["true_flips"].dtype == np.uint32 and np.array_equal(got["true_flips"], ref["true_flips"])
    assert np.array_equal(got["shot_result"], ref["shot_result"]) and np.array_equal(got["result"], ref["result"])
    assert got["stats"].shape == ref["stats"].shape and np.array_equal(got["stats"][..., :2], ref["stats"][..., :2])
    dec = long_experiment(tag, rounds, kw).decoder
    dec.decode(ref["det"])
    assert np.array_equal(got["shot_result"][:, 0].view(np.uint32), dec.last_obs_flips)
    assert np.array_equal(got["shot_result"][:, 1] != 0, dec.last_flagged) and np.array_equal(got["stats"], dec.last_stats)


# ---- 6. purity ------------------------------------------------------------------------------------------------------------------------
def test_result_is_a_pure_function_of_seed_shots_and_rounds():
    exp = rolling_experiment("w3f1m1", "KW_NO_OSD")
    want = long_result("w3f1m1", 9, "KW_NO_OSD")
    whole = exp.run(SHOTS, rounds=9, batch=SHOTS, lanes=1, keep_failures=SHOTS)
    assert_same_experiment(whole, want, 9, 8)
    for batch in (96, 40, 7):
        for lanes in (1, 2):
            assert exp.run(SHOTS, rounds=9, batch=batch, lanes=lanes, keep_failures=SHOTS) == whole, (batch, lanes)
    a, b = exp.run(50, rounds=9, keep_failures=SHOTS), exp.run(46, rounds=9, first_shot=50, keep_failures=SHOTS)
    assert a.shots == 50 and b.shots == 46 and (a.failed_shots < 50).all() and (b.failed_shots >= 50).all()
    assert a + b == whole and np.array_equal((a + b).failed_shots, want.failed_shots) and (a + b).failed_shots_complete
    assert np.array_equal(whole.failed_shots, want.failed_shots) and len(want.failed_shots) > 7
    short = exp.run(SHOTS, rounds=9, keep_failures=7)
    assert len(short.failed_shots) == 7 and not short.failed_shots_complete and np.isin(short.failed_shots, want.failed_shots).all()
    bare = exp.run(SHOTS, rounds=9, batch=40, window_stats=False)
    assert bare.window_exit_classes is None and (bare.shots, bare.logical_errors, bare.flagged, bare.observable_mismatches) == \
        (want.shots, want.logical_errors, want.flagged, want.observable_mismatches)
    assert exp.run(SHOTS, rounds=9, seed=SEED + 1, keep_failures=SHOTS) != whole
    # max_errors stops after a round of lanes
    stop = exp.run(1024, rounds=9, batch=16, lanes=2, max_errors=1)
    assert stop.shots == 32 and stop.logical_errors >= 1
    empty = exp.run(0, rounds=9)
    assert empty.shots == 0 and not empty.window_exit_classes.any() and empty.rounds == 9


# ---- 7. a long run in the memory of a short one ------------------------------------------------------------------------------------------
def test_forty_rounds_in_the_memory_of_nine():
    exp = rolling_experiment("w3f1m1")
    nine = exp.run(32, rounds=9, batch=32, lanes=2)
    before = exp.device_bytes
    assert nine.shots == 32 and before > 0
    res = exp.run(32, rounds=40, batch=32, lanes=2, keep_failures=32)
    want = long_result("w3f1m1", 40, "KW", 32)
    assert_same_experiment(res, want, 40, 39)
    assert np.array_equal(res.failed_shots, want.failed_shots)
    assert exp.device_bytes == before
    # ... and the lanes keep the rows of one step, not the experiment
    assert all(ln["rows"].shape == (32, 3 * H) for ln in exp._lanes)


# ---- 8. a guessing decoder in the windows -------------------------------------------------------------------------------------------------
def test_guessing_decoder_windows():
    """bpgdg_decoder with the parameters of tests/test_gpu_rolling.py::test_guessing_decoder_windows, 24 shots: the counters"""
    from slidingwindowdecoder_amd import MemoryExperiment, RollingMemoryExperiment
    from tests import fixtures as fx
    kw = fx.params(fx.load("bb72_capacity.npz"), "gdg_params")
    kw.pop("multi_thread", None)
    want = MemoryExperiment(plan_for("w3f1m1", 9), decoder="bpgdg_decoder", **kw).run(24, batch=16, keep_failures=24)
    res = RollingMemoryExperiment(template_plan("w3f1m1"), decoder="bpgdg_decoder", **kw).run(24, rounds=9, batch=16, keep_failures=24)
    assert (res.shots, res.logical_errors, res.flagged, res.observable_mismatches) == \
        (24, want.logical_errors, want.flagged, want.observable_mismatches)
    assert np.array_equal(res.failed_shots, want.failed_shots)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------
def test_errors_are_raised_before_anything_is_launched(monkeypatch):
    from slidingwindowdecoder_amd import RollingDemSampler, RollingMemoryExperiment, RollingMemoryResult
    exp = rolling_experiment("w4f2m1")
    with pytest.raises(ValueError, match=r"11 syndrome rounds: this template serves R = 8 \(mod 2\)"):
        exp.run(8, rounds=11)
    with pytest.raises(ValueError, match="this template serves"):
        exp.run(8, rounds=2)
    with pytest.raises(ValueError, match="this template serves"):
        exp.run_batch(8, rounds=9)
    for bad in (dict(lanes=3), dict(batch=0), dict(keep_failures=-1), dict(shots=-1)):
        with pytest.raises(ValueError):
            exp.run(**{"shots": 8, "rounds": 8, **bad})
    assert exp._lanes == []  # nothing was set up, let alone launched
    rs = rolling_sampler("w3f1m1")
    with pytest.raises(ValueError, match="fewer than the template's shortest experiment.*this template serves"):
        rs.sample(4, 2)
    with pytest.raises(ValueError, match="row blocks 9 .. 10 are not within"):
        rs.rows_device(4, 9, 9, 2)
    with pytest.raises(ValueError, match="row blocks"):
        rs.rows_device(4, 9, -1, 2)
    a, b = RollingMemoryResult(9, 8, 10, 1, 0, 1), RollingMemoryResult(10, 9, 10, 1, 0, 1)
    with pytest.raises(ValueError, match="9 and of 10 rounds do not add"):
        a + b
    assert (a + a).shots == 20 and (a + a).rounds == 9 and a != b and a.ler_per_round() == a.ler_per_round(9)
    # templates that create refuses
    chk, obs, priors, h, j0, j1, cols = handmade()
    wide = sp.lil_matrix(chk)
    wide[3 * h + 1, cols[1] + 2] = 1  # a column of block 1 that reaches row block 3
    with pytest.raises(ValueError, match=r"column 5 of round block 1 touches row 16, outside the rows \[5, 15\)"):
        RollingDemSampler.from_blocks(sp.csr_matrix(wide), obs, priors, h, j0, j1, cols)
    changed = priors.copy()
    changed[cols[2] + 4] *= 1.01
    with pytest.raises(ValueError, match="column 4 of block 2 differs from that of block 1 in its prior"):
        RollingDemSampler.from_blocks(chk, obs, changed, h, j0, j1, cols)
    moved = sp.lil_matrix(obs)
    moved[0, cols[3]] = 1 - moved[0, cols[3]]
    with pytest.raises(ValueError, match="column 0 of block 3 differs from that of block 1 in its observable mask"):
        RollingDemSampler.from_blocks(chk, sp.csr_matrix(moved), priors, h, j0, j1, cols)
    with pytest.raises(ValueError, match="at most 32 observables"):
        RollingDemSampler.from_blocks(chk, sp.vstack([obs] * 11, format="csr"), priors, h, j0, j1, cols)
    plan = copy.copy(template_plan("w3f1m1"))
    plan.priors = plan.priors.copy()
    plan.priors[plan.windows[2].col0 + 5] *= 1.5
    with pytest.raises(ValueError, match="priors.* not periodic"):
        RollingDemSampler(plan)
    # the experiment's own refusals: those of MemoryExperiment, and a plan too short to be a template
    tp = template_plan("w3f1m1")
    with pytest.raises(ValueError, match="needs observables"):
        RollingMemoryExperiment(dataclasses.replace(tp, obs=tp.obs[:0]), **KW)
    with pytest.raises(ValueError, match="at most 32 observables"):
        RollingMemoryExperiment(dataclasses.replace(tp, obs=sp.vstack([tp.obs] * 3, format="csr")), **KW)
    with pytest.raises(ValueError, match="at least two body windows"):
        RollingMemoryExperiment(plan_for("w3f1m1", 4), **KW)
    from tests.test_gpu_session import _tiny_host_loop_plan
    monkeypatch.setenv("SWD_FORCE_HUGE", "1")
    with pytest.raises(RuntimeError, match="RollingMemoryExperiment needs the one-launch pipeline"):
        RollingMemoryExperiment(_tiny_host_loop_plan(), pre_max_iter=4, post_max_iter=8, osd_method="osd_0")


def test_bb_builds_the_smallest_template_that_serves_the_length():
    from slidingwindowdecoder_amd import RollingMemoryExperiment
    exp = RollingMemoryExperiment.bb(72, 0.004, 9, 3, 1, **KW)
    assert exp.template.R0 == 5 and exp.rounds == 9 and exp.template.serves(9)
    assert_same_experiment(exp.run(SHOTS), long_result("w3f1m1", 9, "KW"), 9, 8)
    even = RollingMemoryExperiment.bb(72, 0.004, 10, 4, 2, **KW)
    assert even.template.R0 == 6 and even.rounds == 10
    assert_same_experiment(even.run(SHOTS), long_result("w4f2m1", 10, "KW"), 10, len(plan_for("w4f2m1", 10).windows))
    with pytest.raises(ValueError, match=r"no rolling template serves 4 rounds with \(W, F\) = \(3, 1\).*at least two body windows"):
        RollingMemoryExperiment.bb(72, 0.004, 4, 3, 1, **KW)
