"""The bank-conflict-aware message-slot layout (csrc/swd_graph.hip, Graph::optimize_layout) changes no result: each decoder below
runs with the optimised layout and with SWD_NATURAL_LAYOUT set (today's layout), and BOTH are compared with the oracle bit for bit --
total_e_hat / the decoded vectors, exit classes, BP iterations, min_pm (float ==).  Inputs of tests/test_graph_layout.py; no
[[144]]-size graph.

The ragged 48 x 160 matrix, new_n = 50, osd_cs order 2: the syndromes of seed 8 (a third from sparse errors, the rest random bits of
density 0.02 .. 0.5) were chosen on the CPU with the oracle so that the batch leaves through pre-BP (7 shots), post-BP (2), the OSD
(80), "setting vn failed" (1) and "peeling failed" (6)."""
import functools

import numpy as np
import pytest

from tests.test_graph_layout import bb72_window, ragged_matrix

pytestmark = pytest.mark.gpu

LAYOUTS = ["optimised", "natural"]


@pytest.fixture(params=LAYOUTS)
def layout_switch(request, monkeypatch):
    """the switch is read when a decoder is created: every decoder of a test is created inside it"""
    if request.param == "natural":
        monkeypatch.setenv("SWD_NATURAL_LAYOUT", "1")
    else:
        monkeypatch.delenv("SWD_NATURAL_LAYOUT", raising=False)
    return request.param


KW72 = dict(pre_max_iter=8, post_max_iter=24, ms_scaling_factor=1.0, osd_method="osd_cs", osd_order=4)


@functools.lru_cache(maxsize=None)
def pipeline_problem():
    """[[72,12,6]] (3,1), 6 rounds, p = 0.004, 64 shots: (plan, det, the oracle host loop's total_e_hat, exit class / iterations /
    min_pm of every window decode); shared, read-only"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sample_dem, sliding_window_decode_host
    from tests.test_rolling_host import template_plan
    plan = template_plan("w3f1m1")
    shots, W = 64, len(plan.windows)
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, shots, seed=13)
    cls, its, pm = np.full((shots, W), -1, np.int32), np.zeros((shots, W), np.int32), np.zeros((shots, W))

    def tap(wi, j, dec, s, e_hat):
        cls[j, wi], its[j, wi], pm[j, wi] = dec.exit_class, dec.bp_iteration, dec.min_pm
    want, _ = sliding_window_decode_host(plan, det, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW72), on_decode=tap)
    for a in (det, want, cls, its, pm):
        a.setflags(write=False)
    return plan, det, want, cls, its, pm


def test_bb72_pipeline(layout_switch):
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, det, want, cls, its, pm = pipeline_problem()
    assert {0, 1, 2} <= set(np.unique(cls).tolist())  # the oracle's own exits: pre-BP, post-BP, OSD
    dec = SlidingWindowDecoder(plan, **KW72)
    total = dec.decode(det)
    bad = np.flatnonzero((total != want).any(axis=1))
    assert bad.size == 0, f"{layout_switch}: shots {bad[:8].tolist()} differ"
    assert np.array_equal(dec.last_stats[:, :, 0] & 0xFF, cls)
    assert np.array_equal(dec.last_stats[:, :, 1], its)
    assert np.array_equal(dec.last_min_pm, pm)


RAGGED_KW = dict(pre_max_iter=4, post_max_iter=12, ms_scaling_factor=0.9, osd_method="osd_cs", osd_order=2, new_n=50)


@functools.lru_cache(maxsize=None)
def ragged_problem():
    from oracle import oracle as O
    H = ragged_matrix()
    rng = np.random.default_rng(8)
    m, n = H.shape
    synd = np.zeros((96, m), np.uint8)
    for k in range(96):
        if k % 3 == 0:  # syndromes of sparse errors: BP and the OSD have something to find
            synd[k] = (H @ (rng.random(n) < 0.02 + 0.002 * k).astype(np.uint8)) % 2
        else:
            synd[k] = rng.random(m) < rng.uniform(0.02, 0.5)
    pr = np.full(n, 0.03)
    want, res = O.osd_window(H, channel_probs=pr, **RAGGED_KW).decode_batch(synd)
    for a in (synd, want, res):
        a.setflags(write=False)
    return H, pr, synd, want, res


def test_ragged_osd_window_every_exit(layout_switch):
    from slidingwindowdecoder_amd import osd_window
    H, pr, synd, want, res = ragged_problem()
    assert set(np.unique(res["exit_class"]).tolist()) >= {0, 1, 2, 3, 4}, np.bincount(res["exit_class"], minlength=5)
    dev = osd_window(H, channel_probs=pr, **RAGGED_KW)
    out = dev.decode_batch(synd)
    bad = np.flatnonzero((out != want).any(axis=1))
    assert bad.size == 0, f"{layout_switch}: shots {bad[:8].tolist()} differ, oracle exits {res['exit_class'][bad[:8]].tolist()}"
    assert np.array_equal(dev.last_status & 0xFF, res["exit_class"])
    assert np.array_equal(dev.last_iterations, res["bp_iteration"])
    assert np.array_equal(dev.last_min_pm, res["min_pm"])


def test_bb72_gdg_window(layout_switch):
    """one bpgdg_decoder window of the [[72,12,6]] (3,1) plan; the oracle decodes the shots in turn (its bp_iteration counts the
    pre-processing iterations on top of the previous decode's count, and gdg() sets it to 0 once BPGD::reset succeeded)"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import bpgdg_decoder
    from slidingwindowdecoder_amd.windows import sample_dem
    from tests.test_rolling_host import template_plan
    plan = template_plan("w3f1m1")
    w = plan.windows[1]
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, 48, seed=5)
    synd = np.ascontiguousarray(det[:, w.row0:w.row1])  # (raw detector rows of the window: any syndrome serves)
    H = bb72_window()
    assert synd.shape[1] == H.shape[0]
    kw = dict(channel_probs=np.asarray(w.prior), max_iter=8, ms_scaling_factor=1.0, max_iter_per_step=6, max_step=12, max_tree_depth=2,
              max_side_depth=4, max_tree_branch_step=6, max_side_branch_step=6, gdg_factor=1.0)
    dev, ora = bpgdg_decoder(H, **kw), O.bpgdg_decoder(H, **kw)
    out = dev.decode_batch(synd)
    st, pm = dev.last_stats, dev.last_min_pm
    seen, prev_it = set(), 0
    for k in range(len(synd)):
        ora.clear_history()
        want = ora.decode(synd[k])
        res = ora._res
        cls, oc = int(st[k, 0]) & 0xFF, int(res.exit_class)
        tag = f"{layout_switch} shot {k}"
        assert np.array_equal(out[k], want), f"{tag}: vectors differ (device class {cls}, oracle {oc})"
        assert bool(st[k, 0] & 0x100) == bool(ora.converge), f"{tag}: converge"
        assert st[k, 1] == st[k, 2] + st[k, 3], tag
        seen.add(cls)
        if cls != 1:
            assert st[k, 2] == res.bp_iteration - prev_it, f"{tag}: pre iterations {st[k, 2]} vs {res.bp_iteration - prev_it}"
        prev_it = res.bp_iteration
        if cls == 4:  # BPGD::reset failed (the oracle reports it as a post-processing exit that did not converge)
            assert oc == 1 and not ora.converge, tag
            continue
        assert cls == oc, f"{tag}: exit class {cls} vs {oc}"
        if cls == 1:
            assert pm[k] == ora.min_pm, f"{tag}: min_pm {pm[k]} vs {ora.min_pm}"
            assert st[k, 4] == res.reserved, f"{tag}: snapshots {st[k, 4]} vs {res.reserved}"
    assert 1 in seen  # the decimation search ran
