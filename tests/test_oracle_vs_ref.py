"""Oracle vs. the reference's own C/C++ objects (oracle/_ref/libswd_ref.so, built by `make -C oracle ref`
from the reference's sources, which are not part of this repository).
Covers the parts of the path that exist as C/C++ in the reference: rank, index_sort, the sparse LU +
solve behind OSD-0, and the BPGD worker class.  Where the library has not been built, every test replays the reference's answers
recorded under tests/golden/ref_calls/ (tests/ref_replay.py: the oracle's inputs to each call must equal the recorded ones);
SWD_RECORD_REF=1 with the library present records them again."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as O
from tests import fixtures as fx
from tests.ref_replay import GOLDEN, RefCalls

REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libswd_ref.so")
HAVE_REFERENCE = os.path.isdir("/root/reference/src/include")


def test_ref_library_is_built():
    """reference sources present => `make -C oracle ref` (run by __graft_entry__.build()) must have produced the library;
    without them the recorded calls stand in for it"""
    if HAVE_REFERENCE:
        assert os.path.exists(REF), ("oracle/_ref/libswd_ref.so is missing although /root/reference exists: run "
                                     "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C oracle ref`")
    else:
        assert os.path.exists(REF) or len(os.listdir(GOLDEN)) >= 11


@functools.lru_cache(maxsize=None)
def _lib():
    L = C.CDLL(REF)
    vp, i32 = C.c_void_p, C.c_int32
    L.ref_pcm_new.restype = vp
    L.ref_pcm_new.argtypes = [i32, i32, vp, vp]
    L.ref_pcm_free.argtypes = [vp]
    L.ref_rank.argtypes = [vp]
    L.ref_index_sort.argtypes = [vp, vp, i32]
    L.ref_osd0.argtypes = [vp, i32, vp, vp, vp]
    L.ref_bpgd_new.restype = vp
    L.ref_bpgd_new.argtypes = [i32, i32, i32, i32, C.c_double]
    L.ref_bpgd_free.argtypes = [vp]
    L.ref_bpgd_reset.argtypes = [vp, vp, vp, vp, vp]
    L.ref_bpgd_min_sum_log.argtypes = [vp]
    L.ref_bpgd_decimate_vn_reliable.argtypes = [vp, i32, C.c_double]
    L.ref_bpgd_get_pm.restype = C.c_double
    L.ref_bpgd_get_pm.argtypes = [vp]
    L.ref_bpgd_error.argtypes = [vp, vp]
    return L


@pytest.fixture
def R(request):
    """the reference library (live, recording with SWD_RECORD_REF=1) or the replay of its recorded calls for this test"""
    rc = RefCalls(request.node.name, _lib() if os.path.exists(REF) else None, record=os.environ.get("SWD_RECORD_REF") == "1")
    yield rc
    rc.finish()


class Pcm:
    def __init__(self, R, mat):
        csr = sp.csr_matrix(mat)
        csr.sort_indices()
        self.R, self.m, self.n = R, csr.shape[0], csr.shape[1]
        rp, ci = csr.indptr.astype(np.int32), csr.indices.astype(np.int32)
        self.h = R.ref_pcm_new(self.m, self.n, rp.ctypes.data, ci.ctypes.data)

    def __del__(self):
        self.R.ref_pcm_free(self.h)


def window_graphs():
    f = fx.load("bb72_capacity.npz")
    yield "bb72", *fx.graph(f, "osd0_")
    f = fx.load("bb144_circuit_p003_w3f1.npz")
    yield "bb144_last", *fx.graph(f, "win10_")


def test_rank(R):
    for _, mat, _ in window_graphs():
        p = Pcm(R, mat)
        assert R.ref_rank(p.h) == O.osd_window(mat, channel_probs=np.full(mat.shape[1], 0.01)).rank


def test_index_sort_is_stable_ascending(R):
    rng = np.random.default_rng(5)
    v = rng.integers(-3, 4, 500).astype(np.float64)  # many ties
    cols = np.zeros(500, np.int32)
    R.ref_index_sort(v.ctypes.data, cols.ctypes.data, 500)
    assert np.array_equal(cols, np.argsort(v, kind="stable"))


@pytest.mark.parametrize("name", ["bb72", "bb144_last"])
def test_osd0_against_reference_lu(R, name):
    """Non-converging shots: the oracle's OSD-0 solution == the reference's mod2sparse_decomp_osd +
    LU_forward_backward_solve run on the oracle's final LLR order (osd_window.pyx:201-229)."""
    mat, priors = next((m, p) for n_, m, p in window_graphs() if n_ == name)
    m, n = mat.shape
    dec = O.osd_window(mat, channel_probs=priors, pre_max_iter=4, post_max_iter=6, new_n=n, osd_method="osd_0")
    p = Pcm(R, mat)
    rng = np.random.default_rng(11)
    H = sp.csr_matrix(mat).astype(np.int64)
    done = 0
    for _ in range(400):
        e = (rng.random(n) < np.maximum(priors, 0.02) * 2.5).astype(np.int64)
        s = (H @ e % 2).astype(np.uint8)
        dec.clear_history()
        dec.decode(s)
        if dec.converge:
            continue
        h = dec.log_prob_ratios
        llr_sum = np.ascontiguousarray(((h[:, 0] + h[:, 1]) + h[:, 2]) + h[:, 3])
        cols = np.zeros(n, np.int32)
        R.ref_index_sort(llr_sum.ctypes.data, cols.ctypes.data, n)
        out = np.zeros(n, np.uint8)
        R.ref_osd0(p.h, dec.rank, cols.ctypes.data, s.ctypes.data, out.ctypes.data)
        assert np.array_equal(out, dec.osd0_decoding)
        done += 1
        if done >= 40:
            break
    assert done >= 10


def test_bpgd_worker_class(R):
    """bpgd_decoder with max_iter=0 is the bare gd() loop on the identity order (zero history):
    drive the reference's BPGD object through the same steps (bp_guessing_decoder.pyx:517-560)."""
    f = fx.load("bb72_capacity.npz")
    mat, priors = fx.graph(f, "gd_")
    m, n = mat.shape
    T, steps = 6, 25
    dec = O.bpgd_decoder(mat, channel_probs=priors, max_iter=0, max_iter_per_step=T, max_step=steps, new_n=n)
    p = Pcm(R, mat)
    b = R.ref_bpgd_new(m, n, T, 0, 1.0)
    llr = np.log((1 - priors) / priors)
    cols = np.arange(n, dtype=np.int32)
    H = sp.csr_matrix(mat).astype(np.int64)
    rng = np.random.default_rng(3)
    nconv = 0
    for _ in range(60):
        e = (rng.random(n) < 0.04).astype(np.int64)
        s = (H @ e % 2).astype(np.uint8)
        want = dec.decode(s)
        conv, pm = False, 10000.0
        if R.ref_bpgd_reset(b, p.h, cols.ctypes.data, llr.ctypes.data, s.ctypes.data) != -1:
            for depth in range(steps):
                if R.ref_bpgd_min_sum_log(b):
                    conv, pm = True, R.ref_bpgd_get_pm(b)
                    break
                if R.ref_bpgd_decimate_vn_reliable(b, depth, 1.0) == -1:
                    break
        got = np.zeros(n, np.uint8)
        R.ref_bpgd_error(b, got.ctypes.data)
        assert bool(dec.converge) == conv
        assert np.array_equal(got, want)
        if conv:
            assert dec.min_pm == pm
            nconv += 1
    assert nconv >= 20
    R.ref_bpgd_free(b)


def _ensemble_case(R, mat, priors, kw, synds):
    """Oracle ensemble (fixed thread order) vs the reference's real threads on the same column order: every thread's path metric
    must agree bit for bit (those are race free); the shared result must agree whenever the winning metric is unique."""
    m, n = mat.shape
    dec = O.bpgdg_decoder(mat, channel_probs=priors, multi_thread=True, **kw)
    p = Pcm(R, mat)
    llr = np.ascontiguousarray(np.log((1 - priors) / priors))
    new_n = kw.get("new_n") or min(n, 2 * m)
    R.ref_gdg_multi.argtypes = [C.c_void_p] + [C.c_int32] * 9 + [C.c_double] + [C.c_void_p] * 6
    ran = ties = conv = 0
    for s in synds:
        dec.clear_history()
        out = dec.decode(s)
        if dec._res.exit_class == 0:
            continue  # pre-processing BP converged: no ensemble
        pms, winner, nt = dec.ensemble_info()
        cols = np.ascontiguousarray(dec.cols)
        err, rpm, rpms = np.zeros(new_n, np.uint8), C.c_double(), np.zeros(256)
        su = np.ascontiguousarray(s, np.uint8)
        rc = R.ref_gdg_multi(p.h, m, new_n, kw["max_iter_per_step"], kw["max_step"], kw["max_tree_depth"], kw["max_side_depth"],
                             kw["max_tree_branch_step"], kw["max_side_branch_step"], int(kw.get("low_error_mode", False)),
                             float(kw.get("gdg_factor", 1.0)), cols.ctypes.data, llr.ctypes.data, su.ctypes.data, err.ctypes.data,
                             C.byref(rpm), rpms.ctypes.data)
        T, S = rc & 0xFFFF, rc >> 16
        assert len(pms) == 1 + T + S
        assert np.array_equal(pms[1:], rpms[:T + S]), f"per-thread path metrics differ: {pms[1:]} vs {rpms[:T + S]}"
        assert dec.min_pm == rpm.value and bool(dec.converge) == (rpm.value < 9999.0)
        if rpm.value < 9999.0 and pms[0] < 9999.0:
            assert pms[0] >= rpm.value
        ran += 1
        conv += int(dec.converge)
        if nt > 0:
            ties += 1  # another vector with the same metric: the reference's own answer depends on which thread got the lock first
            continue
        ref_out = np.zeros(n, np.uint8)
        ref_out[cols[:new_n]] = err
        assert np.array_equal(out, ref_out), f"ensemble result differs (winner {winner}, pm {dec.min_pm})"
    return ran, conv, ties


def test_threaded_ensemble_bb72(R):
    f = fx.load("bb72_capacity.npz")
    mat, _ = fx.graph(f, "gdg_")
    rng = np.random.default_rng(23)
    priors = rng.uniform(0.03, 0.08, size=72)  # unequal priors: path metrics of different hypotheses rarely tie
    kw = dict(max_iter=8, ms_scaling_factor=1.0, max_iter_per_step=6, max_step=25, max_tree_depth=3, max_side_depth=10,
              max_tree_branch_step=10, max_side_branch_step=10, gdg_factor=1.0)
    H = sp.csr_matrix(mat).astype(np.int64)
    synds = [(H @ (rng.random(72) < priors * 1.3).astype(np.int64) % 2).astype(np.uint8) for _ in range(300)]
    ran, conv, ties = _ensemble_case(R, mat, priors, kw, synds)
    assert ran >= 60 and conv >= 30 and ties < ran // 10, (ran, conv, ties)


def test_threaded_ensemble_bb144_window(R):
    """a circuit-level window of configs[2] with the notebook's parameters (Sliding Window GDG.ipynb cell 3), multi_thread=True"""
    f = fx.load("bb144_circuit_p003_w3f1.npz")
    mat, priors = fx.graph(f, "win5_")
    tr = fx.Trace(f, "gdg_win5_", *mat.shape)
    kw = fx.params(f, "gdg_params")
    kw.pop("multi_thread")
    ran, conv, ties = _ensemble_case(R, mat, priors, kw, list(tr.synd[:192]))
    assert ran >= 40 and conv >= 30, (ran, conv, ties)


def test_gdg_multi_64_hypotheses_bb144_window(R):
    """BASELINE configs[2] as written -- 64 decimation hypotheses per shot: max_tree_depth 5, max_side_depth 6 (main + 31 tree threads
    with two leaves each + one side thread) -- on [[144,12,12]] circuit-level windows: every thread's path metric of the oracle's
    restatement against the reference's REAL threads (ref_gdg_multi), the shared minimum, and the vector wherever it is unique."""
    f = fx.load("bb144_circuit_p003_w3f1.npz")
    kw = fx.params(f, "gdg_params")
    kw.pop("multi_thread")
    kw.update(max_tree_depth=5, max_side_depth=6)
    tot = [0, 0, 0]
    for wi in (0, 5, 10):
        mat, priors = fx.graph(f, f"win{wi}_")
        tr = fx.Trace(f, f"gdg_win{wi}_", *mat.shape)
        r = _ensemble_case(R, mat, priors, kw, list(tr.synd[:64]))
        tot = [a + b for a, b in zip(tot, r)]
    assert tot[0] >= 30 and tot[1] >= 25, tot


def test_threaded_ensemble_bb288_window_d4s20(R):
    """The reference's [[288,12,18]] (4,1) guessing-decoder shape (`Sliding Window GDG.ipynb` cell 8: max_iter 16, max_step 60,
    max_tree_depth 4, max_side_depth 20, branch steps 40 -> 1 + 15 + 16 = 32 threads) on the 576 x 4896 windows of the recorded
    run: every thread's path metric of the oracle's ensemble against the reference's REAL threads."""
    f = fx.load("bb288_gdg_p005_w4f1.npz")
    kw = fx.params(f, "d4s20_params")
    kw.pop("multi_thread")
    tot = [0, 0, 0]
    for wi in (1, 3):
        mat, priors = fx.graph(f, f"win{wi}_")
        tr = fx.Trace(f, f"d4s20_win{wi}_", *mat.shape)
        r = _ensemble_case(R, mat, priors, kw, list(tr.synd[:32]))
        tot = [a + b for a, b in zip(tot, r)]
    assert tot[0] >= 20 and tot[1] >= 15, tot


def test_threaded_ensemble_main_thread_scans_a_block_that_converged_early(R):
    """A window found by tests/fuzz_pipeline.py (seed 13000, `ens`; dumped with SWD_FUZZ_DUMP): the main thread's fifth block
    converges in its second iteration and the thread runs select_vn on it BEFORE testing convergence (bpgd.cpp:630-633), i.e. on a
    history whose slots 2 and 3 are the previous block's and on a syndrome that is met.  The reference's real threads, the oracle
    and the stored vector agree (round 4's device walk did not: it recorded the last four iterations of a block only)."""
    import json
    f = np.load(os.path.join(os.path.dirname(__file__), "golden", "ens_main_early_convergence.npz"))
    mat = sp.csr_matrix((np.ones(len(f["indices"]), np.uint8), f["indices"], f["indptr"]), shape=tuple(f["shape"]))
    kw = json.loads(str(f["kw"]))
    kw.pop("multi_thread")
    ran, conv, ties = _ensemble_case(R, mat, f["prior"], kw, [f["synd"]])
    assert (ran, conv, ties) == (1, 1, 0)
    dec = O.bpgdg_decoder(mat, channel_probs=f["prior"], multi_thread=True, **kw)
    assert np.array_equal(dec.decode(f["synd"]), f["expect"]) and dec.min_pm == float(f["expect_pm"])


def test_threaded_ensemble_weight2_known_answer():
    """`Syndrome code.ipynb` cell 6 (:233-234): with multi_thread=True only the syndromes (0,72) and (1,73) of the [[288,12,18]] hx
    converge, both with 14 flipped variable nodes -- that stored output is the ensemble's, and the oracle's ensemble reproduces it
    (the reference's own run, recorded in the fixture, agrees)."""
    f = fx.load("bb288_hx_wt2_kat.npz")
    from slidingwindowdecoder_amd.codes import bb_code
    code, _, _ = bb_code(288)
    kw = fx.params(f, "params")
    dec = O.bpgdg_decoder(code.hx, channel_probs=np.ones(288) * 0.01, multi_thread=True, **kw)
    ok = []
    for i, j in f["pairs"]:
        s = np.zeros(144, np.uint8)
        s[i] = s[j] = 1
        dec.clear_history()
        e = dec.decode(s)
        if dec.converge:
            ok.append((int(i), int(j), int(e.sum())))
    assert ok == [tuple(int(x) for x in r) for r in f["multi"]] == [(0, 72, 14), (1, 73, 14)]


def test_reused_ensemble_object_keeps_its_previous_vector_when_reset_fails(R):
    """The documented deviation, measured (include/swd.h, swd_gdg_params.multi_thread): the reference's bpgdg_decoder keeps ONE
    BPGD_main_thread for its lifetime (bp_guessing_decoder.pyx:238-251).  do_work clears min_pm but not min_pm_error
    (bpgd.cpp:597-599) and returns early when BPGD::reset fails (:619-625), so a RE-USED object returns its previous decode's vector
    there (converge False), while a freshly built object -- ref_gdg_multi, the oracle, the device -- returns zeros.  Everything else
    (every thread's path metric, the shared minimum, the vector of every decode whose reset succeeds) is the same on the re-used
    object as on fresh ones when max_iter_per_step >= 4 (no stale history slot is ever read)."""
    f = fx.load("bb72_capacity.npz")
    mat, _ = fx.graph(f, "gdg_")
    m, n = mat.shape
    rng = np.random.default_rng(5)
    priors = rng.uniform(0.03, 0.08, size=n)
    new_n = 24  # a short kept set: some checks keep one column, and an inconsistent syndrome makes the peeling in reset fail
    kw = dict(max_iter=8, ms_scaling_factor=1.0, max_iter_per_step=6, max_step=25, max_tree_depth=3, max_side_depth=10,
              max_tree_branch_step=10, max_side_branch_step=10, gdg_factor=1.0, new_n=new_n)
    H = sp.csr_matrix(mat).astype(np.int64)
    synds = [(H @ (rng.random(n) < priors * 1.3).astype(np.int64) % 2).astype(np.uint8) for _ in range(120)]
    synds += [(rng.random(m) < 0.3).astype(np.uint8) for _ in range(120)]  # random syndromes: mostly outside the kept columns' span
    order = rng.permutation(len(synds))
    dec = O.bpgdg_decoder(mat, channel_probs=priors, multi_thread=True, **kw)
    p = Pcm(R, mat)
    llr = np.ascontiguousarray(np.log((1 - priors) / priors))
    vp, i32 = C.c_void_p, C.c_int32
    R.ref_gdg_multi_new.restype = vp
    R.ref_gdg_multi_new.argtypes = [i32] * 9 + [C.c_double]
    R.ref_gdg_multi_free.argtypes = [vp]
    R.ref_gdg_multi_decode.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    obj = R.ref_gdg_multi_new(m, new_n, kw["max_iter_per_step"], kw["max_step"], kw["max_tree_depth"], kw["max_side_depth"],
                              kw["max_tree_branch_step"], kw["max_side_branch_step"], 0, 1.0)
    prev = np.zeros(new_n, np.uint8)  # min_pm_error of a new object: zeros (vector<char>(n))
    ran = fails = kept_stale = ties = 0
    for k in order:
        s = synds[k]
        dec.clear_history()
        out = dec.decode(s)
        if dec._res.exit_class == 0:
            continue  # pre-processing BP converged: the ensemble object is not touched
        cols = np.ascontiguousarray(dec.cols)
        err, rpm, rpms = np.zeros(new_n, np.uint8), C.c_double(), np.zeros(256)
        su = np.ascontiguousarray(s, np.uint8)
        rc = R.ref_gdg_multi_decode(obj, p.h, m, new_n, cols.ctypes.data, llr.ctypes.data, su.ctypes.data, err.ctypes.data,
                                    C.byref(rpm), rpms.ctypes.data)
        T, S = rc & 0xFFFF, rc >> 16
        ran += 1
        if dec.ensemble_blocks()[0] == 0:  # BPGD::reset failed: no thread ran a BP block
            fails += 1
            assert rpm.value > 9999.0 and not dec.converge
            assert not out.any(), "fresh-object semantics: the zero vector"
            assert np.array_equal(err, prev), "the re-used reference object hands back its previous decode's vector"
            kept_stale += int(prev.any())
            continue
        pms, winner, nt = dec.ensemble_info()
        assert np.array_equal(pms[1:], rpms[:T + S]), "per-thread path metrics differ between a re-used and a fresh object"
        assert dec.min_pm == rpm.value
        if nt == 0:
            ref_out = np.zeros(n, np.uint8)
            ref_out[cols[:new_n]] = err
            assert np.array_equal(out, ref_out)
        else:
            ties += 1
        prev = err.copy()
    R.ref_gdg_multi_free(obj)
    print(f"re-used BPGD_main_thread: {ran} ensemble decodes, {fails} reset failures, {kept_stale} of them returned a stale non-zero vector, {ties} ties")
    assert ran >= 80 and fails >= 5 and kept_stale >= 3, (ran, fails, kept_stale)
