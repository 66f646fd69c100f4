"""What a unit of the persistent pipeline kernel computes must not depend on whether the launch has a min_pm destination, nor on
which units the same workgroup served before it.

Every GPU step runs in a child process of its own (this file run as a script) under a time limit; the tests compare what the
children wrote.  SWD_GRID_PCT is read once per process, so the narrow-grid runs need a fresh process anyway: at 10 % of the resident
grid about 27 units of the recorded [[144,12,12]] run pass through each workgroup (2112 units over ~77 workgroups instead of two
or three each), in every order of exit classes."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120  # seconds; a child takes a few (import, plan, one to two launches)


# ---- child side -----------------------------------------------------------------------------------------------------------

def _problem(case):
    """-> (plan, decoder keywords, det [B, num_det] uint8)"""
    from tests import fixtures as fx
    from tests.test_gpu_pipeline import load_plan
    if case == "bb144":
        f = fx.load("bb144_circuit_p003_w3f1.npz")
        plan = load_plan(f, 11)
        return plan, fx.params(f, "osd10_params"), fx.unpack(f["det"], plan.chk.shape[0])
    if case == "bb288":
        f = fx.load("bb288_circuit_p005_w4f1.npz")
        plan = load_plan(f, 4)
        return plan, fx.params(f, "osd10_params"), fx.unpack(f["det"], plan.chk.shape[0])
    if case == "two_graphs":  # two windows, the first and the last one: no two consecutive units of a shot share a graph
        from slidingwindowdecoder_amd.circuit import bb_dem
        from slidingwindowdecoder_amd.codes import bb_code
        from slidingwindowdecoder_amd.windows import plan_windows, sample_dem
        code, A, B = bb_code(72)
        dem = bb_dem(code, A, B, 0.004, 3)
        plan = plan_windows(dem.chk, dem.obs, dem.priors, 36, 3, 1, method=1)
        det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, 64, seed=77)
        return plan, dict(pre_max_iter=8, post_max_iter=40, ms_scaling_factor=1.0, osd_method="osd_cs", osd_order=4), det
    raise SystemExit(f"unknown case {case}")


def _child(case, modes, out_path):
    import torch
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    plan, kw, det = _problem(case)
    dec = SlidingWindowDecoder(plan, **kw)
    d = torch.from_numpy(np.ascontiguousarray(det)).cuda()
    res = {"threads": np.int64(dec.threads)}
    for mode in modes.split(","):
        sr = torch.zeros((d.shape[0], 2), dtype=torch.int32, device=d.device)
        total, stats, pm = dec.decode_device(d, shot_result=sr, want_min_pm=(mode == "pm"))
        torch.cuda.synchronize()
        dec.check_status()
        assert (pm is not None) == (mode == "pm")
        res[mode + "_total"], res[mode + "_stats"], res[mode + "_shot"] = total.cpu().numpy(), stats.cpu().numpy(), sr.cpu().numpy()
        if pm is not None:
            res[mode + "_min_pm"] = pm.cpu().numpy()
    np.savez(out_path, **res)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child(*sys.argv[1:4])
    sys.exit(0)


# ---- test side ------------------------------------------------------------------------------------------------------------

pytestmark = pytest.mark.gpu


_gpu_fault = []  # a child ended by a signal or a time limit: nothing more is started on the GPU from this module


def run_child(tmp_path, case, modes, grid_pct=None):
    if _gpu_fault:
        pytest.fail(f"not started: an earlier child of this module ended with {_gpu_fault[0]}")
    env = {k: v for k, v in os.environ.items() if k != "SWD_GRID_PCT"}
    if grid_pct is not None:
        env["SWD_GRID_PCT"] = str(grid_pct)
    out = str(tmp_path / f"{case}_{grid_pct}.npz")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), case, modes, out], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _gpu_fault.append("a time limit")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):  # abort, segmentation fault, kill, time limit
        _gpu_fault.append(f"status {r.returncode}")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def bb144_recorded():
    """What the fixture records of the order-10 run: corrections, per window iterations / converge / min_pm, decisions."""
    import scipy.sparse as sp
    from tests import fixtures as fx
    from tests.test_gpu_pipeline import load_plan
    f = fx.load("bb144_circuit_p003_w3f1.npz")
    plan = load_plan(f, 11)
    total = fx.unpack(f["osd10_total"], plan.chk.shape[1])
    tr = [fx.Trace(f, f"osd10_win{wi}_", *plan.windows[wi].mat.shape) for wi in range(11)]
    pred = (sp.csr_matrix(total) @ plan.obs.T.astype(np.int32)).toarray() % 2
    obs = fx.unpack(f["obs_data"], 12)
    sh = np.arange(12, dtype=np.uint32)
    rec = dict(total=total,
               iters=np.stack([t.bp_iteration for t in tr], axis=1), conv=np.stack([t.converge != 0 for t in tr], axis=1),
               min_pm=np.stack([t.min_pm for t in tr], axis=1),
               pred_mask=(pred.astype(np.uint32) << sh).sum(axis=1).astype(np.uint32),
               obs_mask=(obs.astype(np.uint32) << sh).sum(axis=1).astype(np.uint32), logical=f["osd10_logical"] != 0)
    for a in rec.values():
        a.setflags(write=False)
    return rec


@pytest.fixture(scope="module")
def bb144_full_grid(tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("unit_reuse"), "bb144", "pm,nopm")


def check_against_record(r, mode, rec):
    total, st, shot = r[mode + "_total"], r[mode + "_stats"], r[mode + "_shot"]
    bad = np.flatnonzero((total != rec["total"]).any(axis=1))
    assert bad.size == 0, f"{bad.size} shots differ from the recorded corrections: {bad[:8]}"
    assert np.array_equal(st[..., 1], rec["iters"]), "bp_iteration"
    assert np.array_equal((st[..., 0] & 0x100) != 0, rec["conv"]), "converge"
    assert np.array_equal(shot[:, 0].astype(np.uint32), rec["pred_mask"]), "predicted observable flips"
    assert not shot[:, 1].any(), "flagged"
    assert np.array_equal((shot[:, 0].astype(np.uint32) != rec["obs_mask"]) | (shot[:, 1] != 0), rec["logical"]), "decisions"
    if mode + "_min_pm" in r.files:
        assert np.array_equal(r[mode + "_min_pm"], rec["min_pm"]), "min_pm"


def test_recorded_run_with_min_pm_destination(bb144_full_grid, bb144_recorded):
    """The recorded [[144,12,12]] (3,1) run, 192 shots x 11 windows, OSD-CS 10: corrections, iterations, converge, decisions and
    min_pm are those of the record; the units leave through all three exits."""
    r = bb144_full_grid
    assert int(r["threads"]) == 256  # the tuned kernel
    check_against_record(r, "pm", bb144_recorded)
    cls = np.bincount((r["pm_stats"][..., 0] & 0xFF).ravel(), minlength=3)
    assert (cls[:3] > 0).all(), cls


def test_recorded_run_without_min_pm_destination(bb144_full_grid, bb144_recorded):
    """No destination for min_pm: the BP exits skip the path metric.  Corrections, iterations, converge and decisions are those
    of the record; the record holds no more of the statistics, so words 0-7 as a whole (exit class, pre / post iterations, live
    counts, OSD row additions) are compared with what the launch WITH a destination wrote on the same build."""
    r = bb144_full_grid
    check_against_record(r, "nopm", bb144_recorded)
    assert "nopm_min_pm" not in r.files
    assert np.array_equal(r["nopm_stats"], r["pm_stats"])


def test_recorded_run_on_a_tenth_of_the_grid(tmp_path, bb144_full_grid, bb144_recorded):
    """SWD_GRID_PCT=10: every workgroup serves ~27 units of the first, the middle and the last graph, after units of every
    exit class; with and without a min_pm destination.  Against the record as far as it goes (check_against_record); statistics
    words 0-7 as a whole against the full-grid launch of the same build."""
    r = run_child(tmp_path, "bb144", "pm,nopm", grid_pct=10)
    for mode in ("pm", "nopm"):
        check_against_record(r, mode, bb144_recorded)
        assert np.array_equal(r[mode + "_stats"], bb144_full_grid["pm_stats"]), mode


def test_consecutive_units_on_different_graphs(tmp_path):
    """A two-window plan ([[72,12,6]], three rounds, (3,1)): the first and the last window have graphs of their own, so no unit
    finds the graph of the unit before it.  64 shots on a tenth of the grid against the oracle driven through the host loop."""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sliding_window_decode_host
    plan, kw, det = _problem("two_graphs")
    assert len(plan.windows) == 2 and ((plan.windows[0].mat != plan.windows[1].mat).nnz > 0 or (plan.windows[0].prior != plan.windows[1].prior).any())
    r = run_child(tmp_path, "two_graphs", "nopm,pm", grid_pct=10)
    want, _ = sliding_window_decode_host(plan, det, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **kw))
    for mode in ("nopm", "pm"):
        bad = np.flatnonzero((r[mode + "_total"] != want).any(axis=1))
        assert bad.size == 0, f"{mode}: shots {bad.tolist()} differ"
    assert np.array_equal(r["nopm_stats"], r["pm_stats"])
    assert len(np.unique(r["pm_stats"][..., 0] & 0xFF)) >= 2


def test_1024_thread_kernel_without_min_pm_destination(tmp_path):
    """[[288,12,18]] (4,1) at its recorded size (24 shots x 4 windows, OSD-CS 10) runs on a 1024-thread variant: the recorded
    corrections without a min_pm destination."""
    from tests import fixtures as fx
    f = fx.load("bb288_circuit_p005_w4f1.npz")
    r = run_child(tmp_path, "bb288", "nopm")
    assert int(r["threads"]) == 1024
    want = fx.unpack(f["osd10_total"], int(f["chk_shape"][1]))
    bad = np.flatnonzero((r["nopm_total"] != want).any(axis=1))
    assert bad.size == 0, f"shots {bad.tolist()} differ"
