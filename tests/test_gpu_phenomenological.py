"""Phenomenological-noise memory experiments on the device: ``MemoryExperiment.phenomenological`` and
``RollingMemoryExperiment.phenomenological`` against the host restatement (``windows.memory_experiment_host`` with the oracle's
decoders, tests/test_phenomenological_host.py) on the shots ``DemSampler`` drew, and the per-group accounting kernel
(swd_group_account_dev) against numpy.  Every comparison is exact equality."""
import functools

import numpy as np
import pytest

from tests.test_gpu_memory_experiment import synthetic
from tests.test_phenomenological_host import CASES, PARAMS, SEED, code_for, plan_for, specification

pytestmark = pytest.mark.gpu
SHOTS = 256
# case, rounds, W, F, decoder, parameters, shots
EXPERIMENTS = {
    "bb72_z": ("bb72_z", 6, 3, 1, "osd_window", "KW", SHOTS),                # 108 x 324 windows, OSD-CS of order 4
    "surface3_z": ("surface3_z", 4, 2, 1, "osd_window", "KW_OSD0", SHOTS),   # 6 rows per round, 12 x 38 windows
    "bb72_depol": ("bb72_depol", 4, 3, 1, "osd_window", "KW", SHOTS),        # 216 x 864 windows, row weight 14, 24 observables
    "bb72_z_gdg": ("bb72_z", 6, 3, 1, "bpgdg_decoder", "GDG", SHOTS),
}


@functools.lru_cache(maxsize=None)
def experiment(tag, rolling=False, geometry=None, rounds=None):
    from slidingwindowdecoder_amd import MemoryExperiment, RollingMemoryExperiment
    case, R, W, F, decoder, kw, _ = EXPERIMENTS[tag]
    name, basis, noise, p, q = CASES[case]
    W, F = geometry or (W, F)
    cls = RollingMemoryExperiment if rolling else MemoryExperiment
    return cls.phenomenological(code_for(name), p, rounds or R, W, F, q=q, basis=basis, noise=noise, decoder=decoder, **PARAMS[kw])


def spec_for(tag, rounds=None, geometry=None, shots=None):
    case, R, W, F, decoder, kw, n = EXPERIMENTS[tag]
    W, F = geometry or (W, F)
    return specification(case, rounds or R, W, F, shots or n, decoder, kw)


def as_result(spec, **kw):
    from slidingwindowdecoder_amd import MemoryResult
    return MemoryResult(spec["shots"], spec["logical_errors"], spec["flagged"], spec["observable_mismatches"], spec["window_exit_classes"],
                        spec["window_not_converged"], spec["window_bp_iterations"], failed_shots=np.flatnonzero(spec["result"] & 1),
                        failed_shots_complete=True, **kw)


def host_group_counts(plan, spec, obs, groups):
    """shots whose predicted observables differ from the true ones inside each group (lists of observable indices), from the host
    loop's ``total_e_hat``"""
    import scipy.sparse as sp
    pred = (sp.csr_matrix(spec["total_e_hat"].astype(np.int32)) @ plan.obs.T.astype(np.int32)).toarray() % 2
    wrong = pred != obs
    return {name: int(wrong[:, idx].any(axis=1).sum()) for name, idx in groups.items()}


# ---- 1. MemoryExperiment.phenomenological -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["bb72_z", "surface3_z", "bb72_depol"])
def test_experiment_equals_the_specification(tag):
    plan, det, obs, flips, spec, _ = spec_for(tag)
    shots = EXPERIMENTS[tag][6]
    exp = experiment(tag)
    assert (exp.plan.chk != plan.chk).nnz == 0 and (exp.plan.obs != plan.obs).nnz == 0 and np.array_equal(exp.plan.priors, plan.priors)
    assert np.array_equal(exp.plan.perm, np.arange(plan.chk.shape[1])) and exp.decoder._loop is None
    got = exp.run_batch(shots, seed=SEED, observable_groups={})
    assert "group_errors" not in got
    assert np.array_equal(got["det"], det) and np.array_equal(got["true_flips"], flips)
    bad = np.flatnonzero((got["total"] != spec["total_e_hat"]).any(axis=1))
    assert bad.size == 0, f"total_e_hat of {bad.size} shots differs from the oracle's, the first: shot {bad[0]}"
    assert np.array_equal(got["result"], spec["result"])
    res = exp.run(shots, batch=96, seed=SEED, keep_failures=shots, observable_groups={})
    want = as_result(spec)
    print(res, want)
    for name in ("shots", "logical_errors", "flagged", "observable_mismatches"):
        assert getattr(res, name) == getattr(want, name), name
    for name in ("window_exit_classes", "window_not_converged", "window_bp_iterations", "failed_shots"):
        assert np.array_equal(getattr(res, name), getattr(want, name)), name
    assert res == want and res.group_errors == {}
    assert res.window_exit_classes[:, 2].sum() > 0 and 0 < res.logical_errors < shots  # OSD exits and logical errors among them


def test_guessing_decoder_windows():
    """``decoder="bpgdg_decoder"``: faults, per-shot words and counters against the oracle's host loop; the oracle's guessing decoder
    keeps no exit class or iteration count, so the per-window counts are held against the one-launch ``decode`` of the same shots"""
    tag = "bb72_z_gdg"
    plan, det, obs, flips, spec, converged = spec_for(tag)
    shots = EXPERIMENTS[tag][6]
    exp = experiment(tag)
    got = exp.run_batch(shots, seed=SEED)
    assert np.array_equal(got["det"], det) and np.array_equal(got["true_flips"], flips)
    assert np.array_equal(got["total"], spec["total_e_hat"]) and np.array_equal(got["result"], spec["result"])
    res = exp.run(shots, batch=32, seed=SEED, keep_failures=shots)
    assert (res.shots, res.logical_errors, res.flagged, res.observable_mismatches) == \
        (shots, spec["logical_errors"], spec["flagged"], spec["observable_mismatches"])
    assert np.array_equal(res.failed_shots, np.flatnonzero(spec["result"] & 1)) and res.failed_shots_complete
    exp.decoder.decode(det)
    stats = exp.decoder.last_stats
    assert np.array_equal(res.window_exit_classes, np.stack([np.bincount(stats[:, t, 0] & 7, minlength=8) for t in range(stats.shape[1])]))
    assert np.array_equal(res.window_not_converged, ((stats[:, :, 0] & 0x100) == 0).sum(axis=0))
    assert np.array_equal(res.window_bp_iterations, stats[:, :, 1].astype(np.int64).sum(axis=0))
    assert np.array_equal(res.window_not_converged, (~converged).sum(axis=1))


# ---- 2. RollingMemoryExperiment.phenomenological ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [(3, 1), (3, 2)])
def test_rolling_experiment_equals_the_experiment_of_its_own_length(geometry):
    W, F = geometry
    probe = experiment("bb72_z", rolling=True, geometry=geometry, rounds=W + 8 * F)  # asked for a long run: the smallest template
    T = probe.template
    assert probe.rounds == W + 8 * F and T.R0 < probe.rounds and (probe.rounds - T.R0) % F == 0
    for rounds in (T.min_rounds, T.R0 + F):
        plan, det, obs, flips, spec, _ = spec_for("bb72_z", rounds=rounds, geometry=geometry)
        want = as_result(spec)
        res = probe.run(SHOTS, rounds=rounds, seed=SEED, keep_failures=SHOTS)
        print(rounds, res, want)
        assert (res.rounds, res.windows_per_shot) == (rounds, len(plan.windows))
        for name in ("shots", "logical_errors", "flagged", "observable_mismatches"):
            assert getattr(res, name) == getattr(want, name), name
        for name in ("window_exit_classes", "window_not_converged", "window_bp_iterations"):
            a, b = getattr(res, name), getattr(want, name)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1:-1].sum(axis=0)) and np.array_equal(a[2], b[-1]), name
        assert np.array_equal(res.failed_shots, want.failed_shots) and res.failed_shots_complete
        # and MemoryExperiment on the plan of that many rounds
        fixed = experiment("bb72_z", geometry=geometry, rounds=rounds).run(SHOTS, seed=SEED, keep_failures=SHOTS)
        assert fixed == want
        got = probe.run_batch(SHOTS, rounds=rounds, seed=SEED)
        assert np.array_equal(got["det"], det) and np.array_equal(got["true_flips"], flips) and np.array_equal(got["result"], spec["result"])


def test_rolling_constructor_relays_why_no_template_exists():
    from slidingwindowdecoder_amd import RollingMemoryExperiment
    name, basis, noise, p, q = CASES["bb72_z"]
    with pytest.raises(ValueError, match=r"no rolling template serves 3 rounds with \(W, F\) = \(3, 1\).*a rolling template needs"):
        RollingMemoryExperiment.phenomenological(code_for(name), p, 3, 3, 1, **PARAMS["KW"])


def test_a_pair_of_matrices_is_accepted_where_there_is_no_code():
    code = code_for("surface3")
    from slidingwindowdecoder_amd import MemoryExperiment
    exp = MemoryExperiment.phenomenological((code.hz, code.lz), 0.03, 4, 2, 1, q=0.03, **PARAMS["KW_OSD0"])
    plan, det, obs, flips, spec, _ = spec_for("surface3_z")
    assert (exp.plan.chk != plan.chk).nnz == 0 and exp.observable_groups is None
    assert np.array_equal(exp.run_batch(64, seed=SEED)["result"], spec["result"][:64])
    with pytest.raises(ValueError, match="basis and noise belong to a CSSCode"):
        MemoryExperiment.phenomenological((code.hz, code.lz), 0.03, 4, 2, 1, basis="both", **PARAMS["KW_OSD0"])


# ---- 3. the group kernel ------------------------------------------------------------------------------------------------------------------
MASKS = {
    "single": [1 << 5],
    "bit31": [1 << 31],
    "overlap": [0x0000FFF0, 0x00FF0F00],
    "four": [0x3, 1 << 31, 0xFFFFFFFF, 0x00F00000],
    "zero": [0, 0x10],
}


def numpy_groups(shot, flips, masks):
    diff = shot[:, 0].view(np.uint32) ^ flips
    return np.array([int(((diff & np.uint32(m)) != 0).sum()) for m in masks], np.int64)


def device_groups(shot, flips, masks, into=None):
    import torch
    from slidingwindowdecoder_amd import group_account_device
    dev = torch.device("cuda", 0)
    counters = torch.zeros(len(masks), dtype=torch.int64, device=dev) if into is None else into
    group_account_device(torch.from_numpy(np.array(shot)).to(dev), torch.from_numpy(np.array(flips.view(np.int32))).to(dev), masks, counters)
    torch.cuda.synchronize()
    return counters


def sparse_diffs(B, seed=9):
    """like ``synthetic`` but with predicted flips that differ from the true ones in ONE random bit on half of the shots: every mask
    meets shots it counts and shots it does not"""
    rng = np.random.default_rng([seed, B])
    shot, flips, _ = synthetic(B, 1)
    bit = (np.uint32(1) << rng.integers(0, 32, B).astype(np.uint32)) * (rng.random(B) < 0.5)
    shot = np.array(shot)
    shot[:, 0] = (flips ^ bit.astype(np.uint32)).view(np.int32)
    return shot, flips


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200, 256])
@pytest.mark.parametrize("which", sorted(MASKS))
def test_group_accounting_equals_numpy(B, which):
    masks = MASKS[which]
    for shot, flips in (synthetic(B, 1)[:2], sparse_diffs(B)):
        want = numpy_groups(shot, flips, masks)
        first = device_groups(shot, flips, masks)
        assert np.array_equal(first.cpu().numpy(), want), (first, want)
        if which == "zero":
            assert want[0] == 0
        again = device_groups(shot, flips, masks, into=first)  # a second call adds
        assert np.array_equal(again.cpu().numpy(), 2 * want)
    if B >= 200:
        want = numpy_groups(*sparse_diffs(B), masks)
        assert all(0 < c < B for m, c in zip(masks, want) if m), want


def test_group_accounting_walks_a_grid_stride_and_takes_no_shots():
    """2048 * 256 + 257 shots: the grid-stride loop runs twice, the last workgroup partial; B = 0 leaves the counters alone"""
    import torch
    B = 2048 * 256 + 257
    shot, flips = sparse_diffs(B)
    masks = MASKS["four"]
    assert np.array_equal(device_groups(shot, flips, masks).cpu().numpy(), numpy_groups(shot, flips, masks))
    kept = torch.full((4,), 7, dtype=torch.int64, device="cuda:0")
    assert device_groups(shot[:0], flips[:0], masks, into=kept).cpu().tolist() == [7] * 4


def test_group_errors_are_a_pure_function_of_seed_and_shot_numbers():
    exp = experiment("bb72_z")
    groups = {"first": [0], "low": 0x03F, "high": [6, 7, 8, 9, 10, 11], "all": 0xFFF}
    plan, det, obs, flips, spec, _ = spec_for("bb72_z", shots=512)
    want = host_group_counts(plan, spec, obs, {"first": [0], "low": list(range(6)), "high": list(range(6, 12)), "all": list(range(12))})
    results = [exp.run(512, batch=batch, lanes=lanes, seed=SEED, keep_failures=512, observable_groups=groups)
               for batch in (128, 512) for lanes in (1, 2)]
    print(results[0], want)
    assert results[0].group_errors == want and results[0] == as_result(spec, group_errors=want)
    assert all(r == results[0] for r in results[1:])
    assert want["all"] == spec["observable_mismatches"] and 0 < want["first"] < want["low"] < want["all"]
    assert max(want["low"], want["high"]) <= want["all"] <= want["low"] + want["high"]
    # halves of the run add; results with other groups do not
    a = exp.run(200, seed=SEED, keep_failures=512, observable_groups=groups)
    b = exp.run(312, seed=SEED, first_shot=200, keep_failures=512, observable_groups=groups)
    assert a + b == results[0] and (a + b).group_errors == want
    with pytest.raises(ValueError, match="do not add"):
        a + exp.run(8, seed=SEED, first_shot=200)
    assert exp.run_batch(512, seed=SEED, observable_groups=groups)["group_errors"] == want


def test_two_basis_experiment_counts_z_and_x_errors_apart():
    exp = experiment("bb72_depol")
    k = code_for("bb72").K
    assert exp.observable_groups == {"z": (1 << k) - 1, "x": ((1 << k) - 1) << k}
    plan, det, obs, flips, spec, _ = spec_for("bb72_depol")
    want = host_group_counts(plan, spec, obs, {"z": list(range(k)), "x": list(range(k, 2 * k))})
    res = exp.run(SHOTS, batch=96, seed=SEED, keep_failures=SHOTS)  # the groups of basis="both" by default
    print(res, want)
    assert res.group_errors == want and res == as_result(spec, group_errors=want)
    assert want["z"] > 0 and want["x"] > 0
    assert max(want["z"], want["x"]) <= res.logical_errors <= want["z"] + want["x"]
    # the rolling form counts the same groups by default
    rolling = experiment("bb72_depol", rolling=True, rounds=6)  # (its template has 5 rounds and serves 4)
    assert rolling.observable_groups == exp.observable_groups and rolling.template.serves(4)
    assert rolling.run(SHOTS, rounds=4, seed=SEED).group_errors == want


# ---- 4. rejected inputs and the null result -------------------------------------------------------------------------------------------------
def test_rejected_groups_and_the_run_without_groups():
    from slidingwindowdecoder_amd import MemoryResult
    exp = experiment("bb72_z")
    with pytest.raises(ValueError, match="at most 4 observable groups"):
        exp.run(8, observable_groups={str(i): [i] for i in range(5)})
    for bad in ({"a": [12]}, {"a": 1 << 12}, {"a": [0, 31]}, {"a": [-1]}):
        with pytest.raises(ValueError, match="observable"):
            exp.run(8, observable_groups=bad)
        with pytest.raises(ValueError, match="observable"):
            exp.run_batch(8, observable_groups=bad)
    plan, det, obs, flips, spec, _ = spec_for("bb72_z")
    res = exp.run(SHOTS, seed=SEED, keep_failures=SHOTS)
    assert res.group_errors == {} and exp.observable_groups is None
    assert res == MemoryResult(spec["shots"], spec["logical_errors"], spec["flagged"], spec["observable_mismatches"], spec["window_exit_classes"],
                               spec["window_not_converged"], spec["window_bp_iterations"], failed_shots=np.flatnonzero(spec["result"] & 1))
    assert res != as_result(spec, group_errors={"a": 0})
    import torch
    from slidingwindowdecoder_amd import group_account_device
    z = torch.zeros((4, 2), dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="at most 4 masks"):
        group_account_device(z, z[:, 0].contiguous(), [1] * 5, torch.zeros(5, dtype=torch.int64, device="cuda:0"))
    with pytest.raises(ValueError, match="counters must be int64"):
        group_account_device(z, z[:, 0].contiguous(), [1, 2], torch.zeros(3, dtype=torch.int64, device="cuda:0"))
