"""The osd_window kernels of up to 256 threads take the full graph's register caches from the graph's host-packed image
(csrc/swd_graph.hip, Graph::fill_image; tests/test_cache_image_host.py checks the image itself) and number the far and zero slots by
the wave's role.  Neither changes a result: every case runs in both forms of the node pass -- profiled, and uniform with
SWD_UNIFORM_DEPTH=1; the switch is read when a decoder is created, as in tests/test_gpu_node_depth.py -- and each form is compared
with the oracle bit for bit in total_e_hat / the decoded vectors, the exit class, bp_iteration and min_pm.  The oracle keeps no
record of statistics words 2-6 (pre / post iterations, live nodes, checks and edges of the shortened graph): words 2 + 3 must add up
to its bp_iteration, word 2 must be its bp_iteration capped at pre_max_iter, and words 2-6 must be equal in the two forms, whose
full-graph phases share no cache-building code path on the host (two node parts of the image).

Cases, 64 shots each:
 (1) the [[72,12,6]] (3,1) plan, 6 rounds: the <256, 4, 8, 16> variant has no kind-3 kernel and no profile, every launch is kind 0;
 (2) a two-window [[144,12,12]] (3,1) plan (3 rounds, p = 0.006): seed 8 was chosen on the CPU with the oracle, both of its windows
     leave through pre-processing BP, post-processing BP and the OSD (asserted);
 (3) the 200 x 1500 graph of tests/test_cache_image_host.py: column weights 1 .. 6, columns of weight 1 and 2 in cache rows of depth 3;
 (4) plan (1) through a session, one round per push: every window is a launch of its own (W = 1).
The wave roles (swd_wave_roles) follow the SIMDs the hardware puts a workgroup's waves on; a case where they are not the identity
cannot be forced, so the role permutation of the image rows and of the far / zero slots is exercised only as the hardware deals it."""
import functools

import numpy as np
import pytest

from tests.test_cache_image_host import mixed_matrix
from tests.test_gpu_node_depth import KW144, KW_SYN, oracle_pipeline, synthetic_syndromes
from tests.test_session_host import KW as KW72, chunkings

pytestmark = pytest.mark.gpu

SHOTS = 64
FORMS = ("depth", "uniform")


def in_both_forms(monkeypatch, run):
    """run(form) with the switch set for each form (decoders are created inside); returns {form: what run returned}"""
    out = {}
    for form in FORMS:
        if form == "uniform":
            monkeypatch.setenv("SWD_UNIFORM_DEPTH", "1")
        else:
            monkeypatch.delenv("SWD_UNIFORM_DEPTH", raising=False)
        out[form] = run(form)
    return out


def check_words_2_to_6(stats, its, pre_max_iter, tag):
    assert np.array_equal(stats[..., 2] + stats[..., 3], its), tag
    assert np.array_equal(stats[..., 2], np.minimum(its, pre_max_iter)), tag


@functools.lru_cache(maxsize=None)
def bb72_problem():
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows, sample_dem
    code, A, B = bb_code(72)
    dem = bb_dem(code, A, B, 0.004, 6)
    plan = plan_windows(dem.chk, dem.obs, dem.priors, 36, 3, 1, method=1)
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, SHOTS, seed=13)
    return (plan, det) + oracle_pipeline(plan, det, KW72)


@functools.lru_cache(maxsize=None)
def bb144_two_windows():
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows, sample_dem
    code, A, B = bb_code(144)
    dem = bb_dem(code, A, B, 0.006, 3)
    plan = plan_windows(dem.chk, dem.obs, dem.priors, 72, 3, 1, method=1)
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, SHOTS, seed=8)
    return (plan, det) + oracle_pipeline(plan, det, KW144)


def pipeline_case(monkeypatch, problem, kw, threads, forms_expected, kinds_expected):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, det, want, cls, its, pm = problem

    def run(form):
        dec = SlidingWindowDecoder(plan, **kw)
        assert dec.threads == threads and dec.node_pass == forms_expected[form]
        total = dec.decode(det)
        assert dec.last_form["kind"] == kinds_expected[form] and dec.last_form["depth_launch"] == int(forms_expected[form] == "depth")
        bad = np.flatnonzero((total != want).any(axis=1))
        assert bad.size == 0, f"{form}: shots {bad[:8].tolist()} differ"
        assert np.array_equal(dec.last_stats[:, :, 0] & 0xFF, cls)
        assert np.array_equal(dec.last_stats[:, :, 1], its)
        assert np.array_equal(dec.last_min_pm, pm)
        check_words_2_to_6(dec.last_stats, its, kw["pre_max_iter"], form)
        return dec.last_stats[:, :, 2:7].copy()
    got = in_both_forms(monkeypatch, run)
    assert np.array_equal(got["depth"], got["uniform"])
    return cls


def test_1_bb72_plan_kind0_only(monkeypatch):
    cls = pipeline_case(monkeypatch, bb72_problem(), KW72, 256, dict(depth="uniform", uniform="uniform"), dict(depth=0, uniform=0))
    assert len(np.unique(cls)) >= 2


def test_2_bb144_two_windows_every_exit(monkeypatch):
    plan, det, want, cls, its, pm = bb144_two_windows()
    assert [w.mat.shape for w in plan.windows] == [(216, 1656), (216, 1656)]
    for w in range(2):  # the oracle's own exits, per window: pre-BP, post-BP, OSD -- no form can pass by only ever leaving through PRE
        assert np.bincount(cls[:, w], minlength=3)[:3].min() >= 8, np.bincount(cls[:, w])
    pipeline_case(monkeypatch, (plan, det, want, cls, its, pm), KW144, 256, dict(depth="depth", uniform="uniform"), dict(depth=3, uniform=3))


@functools.lru_cache(maxsize=None)
def mixed_problem():
    from oracle import oracle as O
    H = mixed_matrix()
    cdeg = np.sort(np.asarray(H.sum(axis=0)).ravel())[::-1]
    assert H.shape == (200, 1500) and set(cdeg.tolist()) == {1, 2, 3, 4, 5, 6} and (cdeg[512:1280] == 1).any()  # weight 1 in a row of depth 3
    synd = synthetic_syndromes(H, SHOTS, 10)
    pr = np.full(H.shape[1], 0.01)
    want, res = O.osd_window(H, channel_probs=pr, **KW_SYN).decode_batch(synd)
    for a in (synd, want, res):
        a.setflags(write=False)
    return H, pr, synd, want, res


def test_3_mixed_weights_dead_positions_inside_live_rows(monkeypatch):
    from slidingwindowdecoder_amd import osd_window
    H, pr, synd, want, res = mixed_problem()
    assert len(np.unique(res["exit_class"])) >= 3, np.bincount(res["exit_class"])

    def run(form):
        dev = osd_window(H, channel_probs=pr, **KW_SYN)
        assert dev.node_pass == form
        out = dev.decode_batch(synd)
        bad = np.flatnonzero((out != want).any(axis=1))
        assert bad.size == 0, f"{form}: shots {bad[:8].tolist()} differ, oracle exits {res['exit_class'][bad[:8]].tolist()}"
        assert np.array_equal(dev.last_status & 0xFF, res["exit_class"])
        assert np.array_equal(dev.last_iterations, res["bp_iteration"])
        assert np.array_equal(dev.last_min_pm, res["min_pm"])
        check_words_2_to_6(dev.last_stats, res["bp_iteration"], KW_SYN["pre_max_iter"], form)
        return dev.last_stats[:, 2:7].copy()
    got = in_both_forms(monkeypatch, run)
    assert np.array_equal(got["depth"], got["uniform"])


def test_4_session_one_round_per_push(monkeypatch):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, det, want, cls, its, pm = bb72_problem()
    chunks = chunkings(det)["rounds"]
    assert len(chunks) >= len(plan.windows) > 1

    def run(form):
        dec = SlidingWindowDecoder(plan, **KW72)
        ses = dec.session(SHOTS)
        ses.begin(SHOTS)
        done = []
        for ch in chunks:
            for t, col0, faults, st, wpm in ses.push(ch):
                w = plan.windows[t]
                assert np.array_equal(faults, want[:, w.col0:w.col0 + w.commit]), f"{form}: window {t}"
                assert np.array_equal(st[:, 0] & 0xFF, cls[:, t]) and np.array_equal(st[:, 1], its[:, t]) and np.array_equal(wpm, pm[:, t])
                done.append(t)
        assert done == list(range(len(plan.windows)))
        total, st, wpm = ses.finish()[:3]
        ses.close()
        assert np.array_equal(total, want) and np.array_equal(st[:, :, 0] & 0xFF, cls) and np.array_equal(st[:, :, 1], its)
        assert np.array_equal(wpm, pm)
        check_words_2_to_6(st, its, KW72["pre_max_iter"], form)
        return st[:, :, 2:7].copy()
    got = in_both_forms(monkeypatch, run)
    assert np.array_equal(got["depth"], got["uniform"])
