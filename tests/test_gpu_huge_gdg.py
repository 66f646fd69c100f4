"""The guessing decoders on graphs beyond every kernel variant: bpgdg_decoder (single-thread gdg() and the threaded ensemble),
bpgd_decoder and bp_history_decoder take any check matrix up to 4096 checks in the general form (csrc/swd_huge_gdg.hip: one
workgroup per shot, every array in HBM), as osd_window does (tests/test_gpu_huge.py).  Everything is compared with the oracle with
==, floats included: vectors, exit classes, converge flags, iterations, path metrics, snapshots pushed, and the ensemble's winner,
ties and BP blocks."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import fixtures as fx

pytestmark = pytest.mark.gpu

KINDS = [("bpgdg_decoder", False), ("bpgdg_decoder", True), ("bpgd_decoder", False), ("bp_history_decoder", False)]


def _rand_h(rng, m, n, colw=3, ragged=True):
    deg = rng.integers(max(1, colw - 2), colw + 1, size=n) if ragged else np.full(n, colw)
    rows = np.concatenate([rng.choice(m, size=d, replace=False) for d in deg])
    H = sp.csr_matrix((np.ones(len(rows), np.uint8), (rows, np.repeat(np.arange(n), deg))), shape=(m, n))
    H.data[:] = 1
    return H


def _make(name, H, forced=False, **kw):
    import slidingwindowdecoder_amd as S
    if forced:
        os.environ["SWD_FORCE_HUGE"] = "1"
    try:
        return getattr(S, name)(H, **kw)
    finally:
        os.environ.pop("SWD_FORCE_HUGE", None)


def _vs_oracle(name, ens, H, kw, synd, forced=False, min_post=0):
    """device batch against one oracle object decoding the shots in turn; returns the exit classes seen"""
    from oracle import oracle as O
    dev = _make(name, H, forced, multi_thread=ens, **kw) if name == "bpgdg_decoder" else _make(name, H, forced, **kw)
    ora = getattr(O, name)(H, multi_thread=ens, **kw) if name == "bpgdg_decoder" else getattr(O, name)(H, **kw)
    out = dev.decode_batch(synd)
    st, pm = dev.last_stats, dev.last_min_pm
    seen, prev_it = set(), 0
    for k in range(len(synd)):
        ora.clear_history()
        want = ora.decode(synd[k])
        res = ora._res
        cls, oc = int(st[k, 0]) & 0xFF, int(res.exit_class)
        tag = f"{name} ens={ens} shot {k}"
        assert np.array_equal(out[k], want), f"{tag}: vectors differ (device class {cls}, oracle {oc})"
        assert bool(st[k, 0] & 0x100) == bool(ora.converge), f"{tag}: converge"
        assert st[k, 1] == st[k, 2] + st[k, 3], tag
        seen.add(cls)
        # the oracle's bp_iteration counts the pre-processing iterations on top of the previous decode's count; gdg() / gd() set it
        # to 0 once BPGD::reset succeeded
        reset_ok = cls == 1 and not ens
        if not reset_ok:
            assert st[k, 2] == res.bp_iteration - prev_it, f"{tag}: pre iterations {st[k, 2]} vs {res.bp_iteration - prev_it}"
        prev_it = res.bp_iteration
        if cls == 4:  # BPGD::reset failed (the oracle reports it as a post-processing exit that did not converge)
            assert oc == 1 and not ora.converge, tag
            if ens:
                assert not want.any(), tag
            continue
        assert cls == oc, f"{tag}: exit class {cls} vs {oc}"
        if cls != 1:
            assert tuple(st[k, 4:7]) == (H.shape[1], H.shape[0], H.nnz) and st[k, 3] == 0 and pm[k] == 0.0, tag
            continue
        assert pm[k] == ora.min_pm, f"{tag}: min_pm {pm[k]} vs {ora.min_pm}"
        if ens:
            _, winner, ties = ora.ensemble_info()
            assert (st[k, 6], st[k, 7]) == (winner, ties), f"{tag}: winner / ties {tuple(st[k, 6:8])} vs {(winner, ties)}"
            assert st[k, 5] == ora.ensemble_blocks()[0], f"{tag}: BP blocks {st[k, 5]} vs {ora.ensemble_blocks()[0]}"
        else:
            assert st[k, 4] == res.reserved, f"{tag}: snapshots {st[k, 4]} vs {res.reserved}"
            assert st[k, 7] == 0
    post = int(((st[:, 0] & 0xFF) == 1).sum())
    assert post >= min_post, (name, ens, post)
    return seen, dev


@pytest.mark.parametrize("m,n,colw,new_n,p", [(1300, 3000, 4, None, 0.06), (200, 9300, 3, None, 0.012), (40, 100, 11, None, 0.05),
                                              (70, 1500, 5, None, 0.012), (1000, 4000, 3, 3000, 0.05)])
def test_beyond_every_variant_vs_oracle(m, n, colw, new_n, p):
    """shapes no kernel variant takes: more than 1024 checks, 9216 columns, column weight 10, row weight 64 (here < 128), and
    new_n > 2048 -- each guessing decoder against the oracle"""
    rng = np.random.default_rng(m + n)
    H = _rand_h(rng, m, n, colw)
    rw = np.diff(H.indptr)
    if (m, n) == (70, 1500):
        assert 64 < rw.max() < 128
    priors = rng.uniform(0.6 * p, 1.4 * p, size=n)
    e = (rng.random((24, n)) < priors).astype(np.int64)
    synd = ((H @ e.T).T % 2).astype(np.uint8)
    kw = dict(channel_probs=priors, max_iter=6, ms_scaling_factor=1.0, max_iter_per_step=6, max_step=12, max_tree_depth=2,
              max_side_depth=6, max_tree_branch_step=5, max_side_branch_step=5, gdg_factor=1.0)
    if new_n:
        kw["new_n"] = new_n
    for name, ens in KINDS:
        # most shots reach the decimation: post-processing exits for bpgdg / bpgd, the no-OSD exit for bp_history_decoder
        seen, _ = _vs_oracle(name, ens, H, kw, synd, min_post=8 if name != "bp_history_decoder" else 0)
        if name == "bp_history_decoder":
            assert 5 in seen, seen


def _rand_small(rng):
    m, n = int(rng.integers(8, 24)), int(rng.integers(40, 140))
    H = (rng.random((m, n)) < 3.0 / m).astype(np.uint8)
    for c in range(n):
        if H[:, c].sum() == 0:
            H[rng.integers(m), c] = 1
    for r in range(m):
        if H[r].sum() == 0:
            H[r, rng.integers(n)] = 1
    return sp.csr_matrix(H)


def test_forced_general_form_every_exit_and_parameter_shape_vs_oracle():
    """SWD_FORCE_HUGE=1: the general form on small random ragged codes with random parameters -- low_error_mode on and off,
    max_iter_per_step below 4 and not a multiple of 4, tree depths 0-6 (beyond 64 snapshots), max_step > 200 for bpgd, short new_n
    -- against the oracle; the pre-processing, post-processing and failed-reset exits all occur"""
    rng = np.random.default_rng(11)
    seen = set()
    for trial in range(14):
        H = _rand_small(rng)
        m, n = H.shape
        p = rng.uniform(0.02, 0.09, size=n)
        D = trial % 7
        kw = dict(channel_probs=p, max_iter=int(rng.integers(2, 9)), ms_scaling_factor=float(rng.choice([1.0, 0.625])),
                  max_iter_per_step=int(rng.choice([1, 2, 3, 5, 6])), max_step=int(rng.integers(5, 25)), max_tree_depth=D,
                  max_side_depth=int(rng.integers(D, D + 8)), max_tree_branch_step=int(rng.integers(2, 8)),
                  max_side_branch_step=int(rng.integers(3, 12)), gdg_factor=float(rng.choice([1.0, 0.625])),
                  low_error_mode=bool(trial % 2), new_n=int(rng.integers(max(2, m // 2), n + 1)))
        e = (rng.random((48, n)) < p * 1.5).astype(np.int64)
        synd = ((H @ e.T).T % 2).astype(np.uint8)
        for name, ens in KINDS:
            kk = dict(kw)
            if name == "bpgd_decoder" and trial % 3 == 0:
                kk["max_step"] = 300
            s, _ = _vs_oracle(name, ens, H, kk, synd, forced=True)
            seen |= s
    assert {0, 1, 4, 5} <= seen, seen


def _tuned_vs_forced(name, H, priors, kw, synd, ens=False):
    dk = dict(channel_probs=priors, **kw)
    if name == "bpgdg_decoder":
        dk["multi_thread"] = ens
    a, b = _make(name, H, False, **dk), _make(name, H, True, **dk)
    oa, ob = a.decode_batch(synd), b.decode_batch(synd)
    assert np.array_equal(oa, ob), f"{name}: {int((oa != ob).any(axis=1).sum())} vectors differ"
    words = 8 if ens else 7  # (serial word 7: a scheduling diagnostic of the tuned kernels)
    assert np.array_equal(a.last_stats[:, :words], b.last_stats[:, :words]), f"{name} ens={ens}: statistics differ"
    assert np.array_equal(a.last_min_pm, b.last_min_pm)
    return a, b


def test_general_form_equals_the_tuned_kernels_on_the_recorded_fixtures():
    f = fx.load("bb72_capacity.npz")
    for tag in ("gdg", "gdg_low", "gd"):
        mat, priors = fx.graph(f, tag + "_")
        kw = fx.params(f, tag + "_params")
        kw.pop("multi_thread", None)
        tr = fx.Trace(f, tag + "_", *mat.shape)
        name = "bpgd_decoder" if tag == "gd" else "bpgdg_decoder"
        _tuned_vs_forced(name, mat, priors, kw, tr.synd)
        if tag == "gdg":
            _tuned_vs_forced(name, mat, priors, kw, tr.synd, ens=True)
            _tuned_vs_forced("bp_history_decoder", mat, priors, kw, tr.synd)
    g = fx.load("bb144_circuit_p003_w3f1.npz")
    kw = fx.params(g, "gdg_params")
    kw.pop("multi_thread")
    for wi in (0, 5, 10):
        mat, priors = fx.graph(g, f"win{wi}_")
        tr = fx.Trace(g, f"gdg_win{wi}_", *mat.shape)
        _tuned_vs_forced("bpgdg_decoder", mat, priors, kw, tr.synd)
        _tuned_vs_forced("bpgdg_decoder", mat, priors, kw, tr.synd[:64], ens=True)
    h = fx.load("bb288_gdg_p005_w4f1.npz")
    kw = fx.params(h, "d3s10_params")
    kw.pop("multi_thread")
    for wi in (0, 3):
        mat, priors = fx.graph(h, f"win{wi}_")
        tr = fx.Trace(h, f"d3s10_win{wi}_", *mat.shape)
        _tuned_vs_forced("bpgdg_decoder", mat, priors, kw, tr.synd[:48])
        _tuned_vs_forced("bpgdg_decoder", mat, priors, kw, tr.synd[:32], ens=True)


def test_single_decode_sequences_and_the_reused_ensemble_object():
    """decode() one syndrome at a time on the general form equals the tuned kernels: return values, converge, and the reuse_object
    path of the threaded ensemble (the previous decode's position vector after a failed reset)"""
    f = fx.load("bb72_capacity.npz")
    mat, priors = fx.graph(f, "gdg_")
    kw = fx.params(f, "gdg_params")
    kw.pop("multi_thread", None)
    tr = fx.Trace(f, "gdg_", *mat.shape)
    for name, ens in (("bpgdg_decoder", False), ("bpgdg_decoder", True), ("bpgd_decoder", False), ("bp_history_decoder", False)):
        dk = dict(channel_probs=priors, **kw)
        if name == "bpgdg_decoder":
            dk["multi_thread"] = ens
        a, b = _make(name, mat, False, **dk), _make(name, mat, True, **dk)
        for k in range(48):
            ra, rb = a.decode(tr.synd[k]), b.decode(tr.synd[k])
            assert rb.dtype == np.int64 and np.array_equal(ra, rb), (name, ens, k)
            assert a.converge == b.converge, (name, ens, k)


def test_unwindowed_288_model_threaded_ensemble_vs_oracle():
    """the un-windowed 18-round [[288,12,18]] model (2736 x 26 208, new_n 5472), bpgdg_decoder(multi_thread=True) with the
    parameters of the reference's guessing.py, 8 shots against the oracle"""
    import bench
    from slidingwindowdecoder_amd.windows import sample_dem
    plan = bench.build_problem(N=288, p=0.005, rounds=18, W=19, F=1)
    w = plan.windows[0]
    assert w.mat.shape[0] == 2736 and min(w.mat.shape[1], 2 * 2736) == 5472
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, 8, seed=7)
    synd = np.ascontiguousarray(det[:, w.row0:w.row1])
    kw = dict(channel_probs=w.prior, max_iter=8, max_iter_per_step=6, max_step=25, max_tree_depth=3, max_side_depth=10,
              max_tree_branch_step=10, max_side_branch_step=10, low_error_mode=False, gdg_factor=1.0, ms_scaling_factor=1.0)
    _vs_oracle("bpgdg_decoder", True, w.mat, kw, synd, min_post=6)


def test_window_loop_with_the_guessing_decoder_beyond_every_pipeline_kernel():
    """SlidingWindowDecoder(decoder="bpgdg_decoder", multi_thread=True) on the (10,1) windows of the 18-round [[288,12,18]] plan
    (1440 x ~13.5 k each): the host window loop with one device decoder per window equals the same loop over the oracle"""
    import bench
    from oracle import oracle as O
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    from slidingwindowdecoder_amd.windows import sample_dem
    plan = bench.build_problem(N=288, p=0.004, rounds=18, W=10, F=1)
    assert len(plan.windows) > 1 and max(w.mat.shape[0] for w in plan.windows) > 1024
    kw = dict(max_iter=8, max_iter_per_step=6, max_step=25, max_tree_depth=3, max_side_depth=10, max_tree_branch_step=10,
              max_side_branch_step=10, gdg_factor=1.0, ms_scaling_factor=1.0)
    dec = SlidingWindowDecoder(plan, decoder="bpgdg_decoder", multi_thread=True, **kw)
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, 3, seed=5)
    total = dec.decode(det)
    chk_t = sp.csr_matrix(plan.chk.T.astype(np.int32))
    want = np.zeros_like(total)
    cur = det.copy()
    for wi, w in enumerate(plan.windows):
        # one oracle object per window: every ensemble decode starts from a new object's state once the history is cleared; its
        # bp_iteration adds each decode's pre-processing iterations to the previous count
        o, prev_it = O.bpgdg_decoder(w.mat, channel_probs=w.prior, multi_thread=True, **kw), 0
        for k in range(len(det)):
            o.clear_history()
            out = o.decode(cur[k, w.row0:w.row1])
            want[k, w.col0:w.col0 + w.commit] = out[:w.commit]
            assert dec.last_stats[k, wi, 2] == o._res.bp_iteration - prev_it, f"window {wi} shot {k}"
            assert bool(dec.last_stats[k, wi, 0] & 0x100) == bool(o.converge)
            prev_it = o._res.bp_iteration
        cur = ((det + (sp.csr_matrix(want) @ chk_t).toarray()) % 2).astype(np.uint8)
    assert np.array_equal(total, want)
    assert np.array_equal(dec.last_flagged, cur.any(axis=1))
    with pytest.raises(RuntimeError, match="window loop"):
        dec.stream(8)
    with pytest.raises(RuntimeError, match="window loop"):
        next(dec.decode_stream([det]))


def test_window_loop_for_a_plan_beyond_the_large_graph_column_bound():
    """Two 600 x 2100 windows that keep new_n = 2049 columns: too much LDS for the resident kernels, and the large-graph kernels
    of the guessing decoders keep at most 2048 -- a size refusal (SWD_ERR_CAPACITY) like every other, so the plan takes the window
    loop over general-form decoders and equals the same loop over the oracle"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd import SlidingWindowDecoder, _lib, window_forms
    from slidingwindowdecoder_amd.windows import Window, WindowPlan
    rng = np.random.default_rng(11)
    m, n = 600, 2100
    mats = [_rand_h(rng, m, n, 3, ragged=False) for _ in range(2)]
    assert all(np.diff(H.indptr).min() > 0 for H in mats)
    pri = np.full(n, 0.01)  # (the three shots leave by the pre-processing BP, by the tree search, and without converging)
    chk = sp.block_diag(mats, format="csr").astype(np.uint8)
    wins = [Window(k * m, (k + 1) * m, k * n, n, n, mats[k], pri, k == 1) for k in range(2)]
    plan = WindowPlan(chk, sp.csr_matrix((0, 2 * n), dtype=np.uint8), np.tile(pri, 2), np.arange(2 * n), [], wins, None, 0)
    kw = dict(max_iter=8, max_iter_per_step=6, max_step=4, max_tree_depth=2, max_side_depth=4, max_tree_branch_step=4,
              max_side_branch_step=4, gdg_factor=1.0, ms_scaling_factor=1.0, new_n=2049)
    assert window_forms(plan, decoder="bpgdg_decoder", **kw)["general"] == 1
    assert "keep at most 2048 columns" in _lib.last_error() and _lib.last_error_class() == _lib.ERR_CAPACITY
    assert window_forms(plan, decoder="bpgdg_decoder", **dict(kw, new_n=2048))["big"] == 1  # one column fewer: the large-graph kernel
    dec = SlidingWindowDecoder(plan, decoder="bpgdg_decoder", **kw)
    assert dec._loop is not None and len(dec._loop) == 2 and dec.last_form is None
    e = (rng.random((3, 2 * n)) < 0.01).astype(np.int64)
    det = ((chk.astype(np.int64) @ e.T).T % 2).astype(np.uint8)
    total = dec.decode(det)
    chk_t = sp.csr_matrix(chk.T.astype(np.int32))
    want = np.zeros_like(total)
    cur = det.copy()
    for wi, w in enumerate(plan.windows):
        o, prev_it = O.bpgdg_decoder(w.mat, channel_probs=w.prior, **kw), 0
        for k in range(len(det)):
            o.clear_history()
            out = o.decode(cur[k, w.row0:w.row1])
            want[k, w.col0:w.col0 + w.commit] = out[:w.commit]
            assert bool(dec.last_stats[k, wi, 0] & 0x100) == bool(o.converge), f"window {wi} shot {k}"
            if (int(dec.last_stats[k, wi, 0]) & 0xFF) != 1:  # (gdg() sets the oracle's count to 0 once BPGD::reset succeeded: _vs_oracle)
                assert dec.last_stats[k, wi, 2] == o._res.bp_iteration - prev_it, f"window {wi} shot {k}"
            prev_it = o._res.bp_iteration
        cur =((det + (sp.csr_matrix(want) @ chk_t).toarray()) % 2).astype(np.uint8)
    assert np.array_equal(total, want)
    assert np.array_equal(dec.last_flagged, cur.any(axis=1))


def test_device_pointers_on_a_side_stream_equal_the_host_call():
    import torch
    from slidingwindowdecoder_amd import _lib
    rng = np.random.default_rng(3)
    H = _rand_h(rng, 1100, 2400, 3)
    priors = rng.uniform(0.02, 0.05, size=2400)
    e = (rng.random((40, 2400)) < priors).astype(np.int64)
    synd = np.ascontiguousarray(((H @ e.T).T % 2).astype(np.uint8))
    for ens in (False, True):
        dec = _make("bpgdg_decoder", H, channel_probs=priors, max_iter=6, max_step=10, multi_thread=ens)
        want = dec.decode_batch(synd)
        side = torch.cuda.Stream()
        s = torch.from_numpy(synd).cuda()
        out = torch.zeros((40, 2400), dtype=torch.uint8, device="cuda")
        st = torch.zeros((40, 8), dtype=torch.int32, device="cuda")
        pm = torch.zeros(40, dtype=torch.float64, device="cuda")
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            rc = _lib.lib().swd_gdg_decode_batch_dev(dec._h, 40, s.data_ptr(), s.stride(0), out.data_ptr(), out.stride(0),
                                                     st.data_ptr(), pm.data_ptr(), side.cuda_stream)
        assert rc == 0
        side.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
        assert np.array_equal(st.cpu().numpy(), dec.last_stats)
        assert np.array_equal(pm.cpu().numpy(), dec.last_min_pm)


def test_refusals_are_loud_and_bp_history_takes_heavy_checks():
    import slidingwindowdecoder_amd as S
    from oracle import oracle as O
    rng = np.random.default_rng(9)
    H = _rand_h(rng, 1300, 3000, 3)
    p = np.full(3000, 0.02)
    with pytest.raises(RuntimeError, match="hypotheses"):
        S.bpgdg_decoder(H, channel_probs=p, hypotheses=16)
    with pytest.raises(RuntimeError, match="4096 checks"):
        S.bpgdg_decoder(_rand_h(rng, 4100, 5000, 3), channel_probs=np.full(5000, 0.02))
    # a check of weight 130 among 200: the reference's char degrees wrap there -- refused by bpgdg / bpgd, taken by bp_history
    Hd = _rand_h(rng, 200, 1200, 3).tolil()
    Hd[7, :] = 0
    Hd[7, rng.choice(1200, 130, replace=False)] = 1
    Hd = sp.csr_matrix(Hd)
    Hd.eliminate_zeros()
    pd = rng.uniform(0.01, 0.03, size=1200)
    for cls in (S.bpgdg_decoder, S.bpgd_decoder):
        with pytest.raises(RuntimeError, match="weight 130"):
            cls(Hd, channel_probs=pd)
    e = (rng.random((32, 1200)) < pd).astype(np.int64)
    synd = ((Hd @ e.T).T % 2).astype(np.uint8)
    seen, _ = _vs_oracle("bp_history_decoder", False, Hd, dict(channel_probs=pd, max_iter=5), synd)
    assert seen <= {0, 5}
    assert O is not None
