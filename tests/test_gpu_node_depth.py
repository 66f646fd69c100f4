"""The depth-profiled node pass of the <256, 7, 6, 9> kind-3 kernel (csrc/swd_variants.h, SWD_DEPTH_PROFILES) changes no result:
every case runs in the profiled form and with SWD_UNIFORM_DEPTH=1 (the uniform pass), and BOTH are compared with the oracle bit for
bit -- decoded vectors / total_e_hat, exit classes, BP iterations, min_pm (float ==) -- and the form each handle reports is asserted.

Cases (matrices of tests/test_node_depth_host.py; iteration caps are multiples of four, so the launches take the kind-3 kernels):
 (a) [[144,12,12]] (3,1), 5 rounds, p = 0.006, 48 shots through SlidingWindowDecoder: the first, mid and last window graph;
 (b) the 200 x 1792 boundary matrix, every cache row at its depth and the last row full;
 (c) n = 1030: listed row 4 holds six nodes, rows 5 and 6 are empty;
 (d) (b) with a 513th column of degree above 3: does not fit, must report the uniform form;
 (e) a two-window plan of (b) and (d): one kernel serves a launch, so the whole plan is uniform.
The seeds of (a) and (b) were chosen on the CPU with the oracle so that its own exits cover pre-BP, post-BP and the OSD (asserted);
with new_n = 210 the syndromes of (b) also leave through "setting vn failed" and "peeling failed"."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_node_depth_host import boundary_matrix, misfit_matrix, short_matrix

pytestmark = pytest.mark.gpu

FORMS = ["depth", "uniform"]


@pytest.fixture(params=FORMS)
def form_switch(request, monkeypatch):
    """the switch is read when a decoder is created: every decoder of a test is created inside it"""
    if request.param == "uniform":
        monkeypatch.setenv("SWD_UNIFORM_DEPTH", "1")
    else:
        monkeypatch.delenv("SWD_UNIFORM_DEPTH", raising=False)
    return request.param


KW144 = dict(pre_max_iter=8, post_max_iter=24, ms_scaling_factor=1.0, osd_method="osd_cs", osd_order=4)
KW_SYN = dict(pre_max_iter=4, post_max_iter=12, ms_scaling_factor=0.9, osd_method="osd_cs", osd_order=2, new_n=210)
SEED_A, SEED_B = 13, 10


def oracle_pipeline(plan, det, kw):
    """(total_e_hat, exit class / iterations / min_pm [shots, W]) of the oracle's host loop"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sliding_window_decode_host
    shots, W = det.shape[0], len(plan.windows)
    cls, its, pm = np.full((shots, W), -1, np.int32), np.zeros((shots, W), np.int32), np.zeros((shots, W))

    def tap(wi, j, dec, s, e_hat):
        cls[j, wi], its[j, wi], pm[j, wi] = dec.exit_class, dec.bp_iteration, dec.min_pm
    want, _ = sliding_window_decode_host(plan, det, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **kw), on_decode=tap)
    for a in (det, want, cls, its, pm):
        a.setflags(write=False)
    return want, cls, its, pm


@functools.lru_cache(maxsize=None)
def bb144_problem():
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows, sample_dem
    code, A, B = bb_code(144)
    dem = bb_dem(code, A, B, 0.006, 5)
    plan = plan_windows(dem.chk, dem.obs, dem.priors, 72, 3, 1, method=1)
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, 48, seed=SEED_A)
    return (plan, det) + oracle_pipeline(plan, det, KW144)


def check_pipeline(dec, det, want, cls, its, pm, tag):
    total = dec.decode(det)
    bad = np.flatnonzero((total != want).any(axis=1))
    assert bad.size == 0, f"{tag}: shots {bad[:8].tolist()} differ"
    assert np.array_equal(dec.last_stats[:, :, 0] & 0xFF, cls)
    assert np.array_equal(dec.last_stats[:, :, 1], its)
    assert np.array_equal(dec.last_min_pm, pm)


def test_a_bb144_three_window_graphs(form_switch):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, det, want, cls, its, pm = bb144_problem()
    assert [w.mat.shape for w in plan.windows] == [(216, 1656), (216, 1728), (216, 1728), (216, 1656)]  # first, mid, mid, last
    assert {0, 1, 2} <= set(np.unique(cls).tolist())  # the oracle's own exits: pre-BP, post-BP, OSD
    dec = SlidingWindowDecoder(plan, **KW144)
    assert dec.threads == 256 and dec.node_pass == form_switch
    check_pipeline(dec, det, want, cls, its, pm, form_switch)


def synthetic_syndromes(H, shots, seed):
    """as ragged_problem() of tests/test_gpu_graph_layout.py: a third from sparse errors, the rest random bits of density 0.02 .. 0.5"""
    rng = np.random.default_rng(seed)
    m, n = H.shape
    synd = np.zeros((shots, m), np.uint8)
    for k in range(shots):
        if k % 3 == 0:
            synd[k] = (H @ (rng.random(n) < 0.004 + 0.0004 * k).astype(np.uint8)) % 2
        else:
            synd[k] = rng.random(m) < rng.uniform(0.02, 0.5)
    return synd


@functools.lru_cache(maxsize=None)
def window_problem(name):
    from oracle import oracle as O
    H = {"boundary": boundary_matrix, "short": short_matrix, "misfit": misfit_matrix}[name]()
    synd = synthetic_syndromes(H, 48, SEED_B)
    pr = np.full(H.shape[1], 0.01)
    want, res = O.osd_window(H, channel_probs=pr, **KW_SYN).decode_batch(synd)
    for a in (synd, want, res):
        a.setflags(write=False)
    return H, pr, synd, want, res


def check_window(name, expect_form, form_switch):
    from slidingwindowdecoder_amd import osd_window
    H, pr, synd, want, res = window_problem(name)
    dev = osd_window(H, channel_probs=pr, **KW_SYN)
    assert dev.node_pass == (expect_form if form_switch == "depth" else "uniform")
    out = dev.decode_batch(synd)
    bad = np.flatnonzero((out != want).any(axis=1))
    assert bad.size == 0, f"{name} {form_switch}: shots {bad[:8].tolist()} differ, oracle exits {res['exit_class'][bad[:8]].tolist()}"
    assert np.array_equal(dev.last_status & 0xFF, res["exit_class"])
    assert np.array_equal(dev.last_iterations, res["bp_iteration"])
    assert np.array_equal(dev.last_min_pm, res["min_pm"])
    return res


def test_b_every_row_at_its_depth(form_switch):
    res = check_window("boundary", "depth", form_switch)
    # the oracle's own exits: pre-BP, post-BP, OSD, "setting vn failed", "peeling failed"
    assert set(np.unique(res["exit_class"]).tolist()) >= {0, 1, 2, 3, 4}, np.bincount(res["exit_class"], minlength=5)


def test_c_partly_filled_and_empty_rows(form_switch):
    check_window("short", "depth", form_switch)


def test_d_one_column_too_many_stays_uniform(form_switch):
    check_window("misfit", "uniform", form_switch)


@functools.lru_cache(maxsize=None)
def two_window_problem():
    """window 0 = (b), window 1 = (d), block-diagonal global matrix, every column committed"""
    from slidingwindowdecoder_amd.windows import Window, WindowPlan
    Hb, Hd = boundary_matrix(), misfit_matrix()
    (mb, nb), (md, nd) = Hb.shape, Hd.shape
    chk = sp.block_diag([Hb, Hd], format="csr")
    pri = np.full(nb + nd, 0.01)
    wins = [Window(0, mb, 0, nb, nb, Hb, pri[:nb], False), Window(mb, mb + md, nb, nd, nd, Hd, pri[nb:], True)]
    plan = WindowPlan(chk, None, pri, np.arange(nb + nd), [], wins, None, 0)
    det = np.concatenate([synthetic_syndromes(Hb, 24, SEED_B), synthetic_syndromes(Hd, 24, SEED_B + 1)], axis=1)
    return (plan, det) + oracle_pipeline(plan, det, KW_SYN)


def test_e_plan_with_one_misfit_graph_is_uniform(form_switch):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, det, want, cls, its, pm = two_window_problem()
    dec = SlidingWindowDecoder(plan, **KW_SYN)
    assert dec.threads == 256 and dec.node_pass == "uniform"
    check_pipeline(dec, det, want, cls, its, pm, form_switch)
