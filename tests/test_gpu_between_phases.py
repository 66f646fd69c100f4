"""The passes between the two BP phases of the tuned osd_window kernels of up to 256 threads (csrc/swd_osdw_kernel.h, decode_window:
column select, live masks, peeling rounds without a backup, compaction, the shortened graph's caches) change no result.  Every case
compares with ==, against oracle.osd_window or the oracle's host window loop: the decoded vectors / total_e_hat, the exit class, the BP
iterations, min_pm, and the statistics words 4 to 6 (live variable nodes, live checks, live edges of the shortened graph).

The oracle keeps no count of the live nodes.  Words 4 to 6 are worked out here from what it does keep: an oracle with post_max_iter = 0
leaves the LLR history of the iterations in front; its sums, sorted as the oracle sorts them, give the decided set, and the closure of
the degree-1 checks (which does not depend on the order, and is only asked for when the oracle's own run met no contradiction) gives the
live graph.  Exits in front of the compaction report the full graph.

Cases:
 (a) [[72,12,6]] circuit-level (3,1) windows, 300 shots at p = 0.006, OSD-CS 10 and OSD-0, with iteration caps that are multiples of
     four and with odd ones.  The windows (108 x 864) take the <256, 4, 8, 16> kernels, which exist as kind 0 only: both caps run the
     kind-0 kernel.  Kind 3 is covered by (c) and (d).
 (b) small random matrices (m <= 64, n <= 448, column weight <= 6) on random syndromes; the seed was chosen on the CPU so that the
     oracle alone leaves at least 8 times through "setting vn failed", 8 times through "peeling failed", 50 times through the post-phase
     BP and 20 times through the OSD (asserted on the oracle's output).
 (c) boundary ties: a block of checks with random syndromes beside many identical one-check components with better priors and a zero
     syndrome, whose columns all end with the same -- largest -- history sum; more than n - new_n columns share the boundary sum (asserted
     on the oracle's history), so the decided set is settled by node number.  "tie_depth" takes the depth-profiled kind-3 kernel, whose
     threads hold the nodes in descending-degree order, not in node order; "tie_small" a 64-thread kernel.  "no_select" has
     new_n = n; "odd_slots" a slot table whose length is no multiple of four (asserted through the graph layout).
 (d) one [[144,12,12]] (3,1) plan, 64 shots, through SlidingWindowDecoder.decode_device: the headline graphs, kind 3 (depth profile)
     and kind 0."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


# ---- statistics words 4 to 6 from the oracle's history ---------------------------------------------------------------------------
def history_sums(aux, synd):
    """history sums in front of the shortening step: `aux` is an oracle with post_max_iter = 0 (its history is that of the first phase)"""
    aux.clear_history()
    aux.decode(synd)
    h = aux.log_prob_ratios
    with np.errstate(over="ignore"):  # (a sum may overflow to inf, as the oracle's own does)
        return ((h[:, 0] + h[:, 1]) + h[:, 2]) + h[:, 3]


def live_words(H, sums, new_n):
    """(live nodes, live checks, live edges) once the columns behind position new_n of the stable order are decided and the degree-1
    checks are peeled"""
    H = sp.csr_matrix(H)
    live = np.ones(H.shape[1], bool)
    live[np.argsort(sums, kind="stable")[new_n:]] = False
    while True:
        deg = H @ live.astype(np.int64)
        ones = np.flatnonzero(deg == 1)
        if ones.size == 0:
            return int(live.sum()), int((deg > 0).sum()), int(deg.sum())
        cols = H[ones].indices
        live[cols[live[cols]]] = False


def aux_oracle(H, pr, kw):
    from oracle import oracle as O
    return O.osd_window(H, channel_probs=pr, **dict(kw, post_max_iter=0, osd_method="osd_0", osd_order=0))


def default_new_n(H, kw):
    m, n = H.shape
    return min(int(kw["new_n"]), n) if kw.get("new_n") else min(n, 2 * m)


def expected_words(H, pr, kw, synd, cls):
    """[shots, 3] words 4 to 6 for one window's syndromes and the oracle's exit classes"""
    H = sp.csr_matrix(H)
    aux, new_n = aux_oracle(H, pr, kw), default_new_n(H, kw)
    out = np.tile(np.array([H.shape[1], H.shape[0], H.nnz], np.int64), (len(synd), 1))
    for k in np.flatnonzero((cls == 1) | (cls == 2)):
        out[k] = live_words(H, history_sums(aux, synd[k]), new_n)
    return out


# ---- single windows through osd_window -------------------------------------------------------------------------------------------
def check_window(H, pr, kw, synd, want, res, tag, kind=None):
    from slidingwindowdecoder_amd import osd_window
    dev = osd_window(H, channel_probs=pr, **kw)
    out = dev.decode_batch(synd)
    if kind is not None:
        assert dev.last_form["kind"] == kind, f"{tag}: kernel kind {dev.last_form['kind']}"
    bad = np.flatnonzero((out != want).any(axis=1))
    assert bad.size == 0, f"{tag}: shots {bad[:8].tolist()} differ, oracle exits {res['exit_class'][bad[:8]].tolist()}"
    assert np.array_equal(dev.last_status & 0xFF, res["exit_class"]), tag
    assert np.array_equal(dev.last_iterations, res["bp_iteration"]), tag
    assert np.array_equal(dev.last_min_pm, res["min_pm"]), tag
    words = expected_words(H, pr, kw, synd, res["exit_class"])
    assert np.array_equal(dev.last_stats[:, 4:7], words), f"{tag}: statistics words 4..6"
    return dev


# ---- window plans through SlidingWindowDecoder ------------------------------------------------------------------------------------
def oracle_plan(plan, det, kw):
    """(total_e_hat, exit class / iterations / min_pm [shots, W], words 4..6 [shots, W, 3]) of the oracle's host loop"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sliding_window_decode_host
    shots, W = det.shape[0], len(plan.windows)
    cls, its, pm = np.full((shots, W), -1, np.int32), np.zeros((shots, W), np.int32), np.zeros((shots, W))
    words = np.zeros((shots, W, 3), np.int64)
    aux = [aux_oracle(w.mat, w.prior, kw) for w in plan.windows]

    def tap(wi, j, dec, s, e_hat):
        cls[j, wi], its[j, wi], pm[j, wi] = dec.exit_class, dec.bp_iteration, dec.min_pm
        w = plan.windows[wi]
        words[j, wi] = (w.mat.shape[1], w.mat.shape[0], w.mat.nnz)
        if dec.exit_class in (1, 2):
            words[j, wi] = live_words(w.mat, history_sums(aux[wi], s), default_new_n(w.mat, kw))
    want, _ = sliding_window_decode_host(plan, det, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **kw), on_decode=tap)
    for a in (want, cls, its, pm, words):
        a.setflags(write=False)
    return want, cls, its, pm, words


@functools.lru_cache(maxsize=None)
def bb_plan(N, shots, seed):
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows, sample_dem
    code, A, B = bb_code(N)
    dem = bb_dem(code, A, B, 0.006, 5)
    plan = plan_windows(dem.chk, dem.obs, dem.priors, N // 2, 3, 1, method=1)
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, shots, seed=seed)
    det.setflags(write=False)
    return plan, det


def check_plan(plan, det, kw, tag, kind, nt_vf=None):
    import torch
    from slidingwindowdecoder_amd import SlidingWindowDecoder
    want, cls, its, pm, words = oracle_plan(plan, np.array(det), kw)
    dec = SlidingWindowDecoder(plan, **kw)
    total, stats, min_pm = dec.decode_device(torch.from_numpy(np.array(det)).cuda())
    torch.cuda.synchronize()
    total, stats, min_pm = total.cpu().numpy(), stats.cpu().numpy(), min_pm.cpu().numpy()
    form = dec.last_form
    assert form["kind"] == kind, f"{tag}: kernel kind {form['kind']}"
    if nt_vf is not None:
        assert (form["nt"], form["vf"]) == nt_vf, f"{tag}: variant {form['nt']}, {form['vf']}"
    bad = np.flatnonzero((total != want).any(axis=1))
    assert bad.size == 0, f"{tag}: shots {bad[:8].tolist()} differ"
    assert np.array_equal(stats[:, :, 0] & 0xFF, cls), tag
    assert np.array_equal(stats[:, :, 1], its), tag
    assert np.array_equal(min_pm, pm), tag
    assert np.array_equal(stats[:, :, 4:7], words), f"{tag}: statistics words 4..6"
    return cls


CAPS = {"m4": dict(pre_max_iter=8, post_max_iter=24), "odd": dict(pre_max_iter=7, post_max_iter=23)}
OSD = {"cs10": dict(osd_method="osd_cs", osd_order=10), "osd0": dict(osd_method="osd_0", osd_order=0)}


@pytest.mark.parametrize("osd", ["cs10", "osd0"])
@pytest.mark.parametrize("caps", ["m4", "odd"])
def test_a_bb72_windows(caps, osd):
    plan, det = bb_plan(72, 300, 5)
    cls = check_plan(plan, det, dict(CAPS[caps], ms_scaling_factor=1.0, **OSD[osd]), f"bb72 {caps} {osd}", 0, (256, 4))
    assert {0, 1, 2} <= set(np.unique(cls).tolist())  # the oracle's own exits: pre-BP, post-BP, OSD


@pytest.mark.parametrize("caps,kind", [("m4", 3), ("odd", 0)])
def test_d_bb144_plan_64_shots(caps, kind):
    plan, det = bb_plan(144, 64, 13)
    cls = check_plan(plan, det, dict(CAPS[caps], ms_scaling_factor=1.0, osd_method="osd_cs", osd_order=10), f"bb144 {caps}", kind, (256, 7))
    assert {0, 1, 2} <= set(np.unique(cls).tolist())


# ---- (b) the rare exits -------------------------------------------------------------------------------------------------------------
RARE_SEED, RARE_TRIALS, RARE_SHOTS = 33, 10, 120


def rare_problems(seed, trials, shots):
    """the generator of test_failed_decimation_and_peel_exits_vs_oracle (tests/test_gpu_osdw.py) with m <= 64, n <= 448 and column
    weight <= 6"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < trials:
        m, n = int(rng.integers(10, 65)), int(rng.integers(60, 449))
        H = (rng.random((m, n)) < 2.5 / m).astype(np.uint8)
        for c in range(n):
            if H[:, c].sum() == 0:
                H[rng.integers(m), c] = 1
        for r in range(m):
            if H[r].sum() == 0:
                H[r, rng.integers(n)] = 1
        if H.sum(axis=0).max() > 6 or H.sum(axis=1).max() > 60:
            continue
        p = rng.uniform(0.01, 0.08, size=n)
        kw = dict(pre_max_iter=int(rng.integers(1, 5)), post_max_iter=int(rng.integers(1, 20)), ms_scaling_factor=1.0, osd_method="osd_0",
                  osd_order=0, new_n=int(rng.integers(m, 2 * m)))
        synd = (rng.random((shots, m)) < rng.choice([0.05, 0.15, 0.35])).astype(np.uint8)
        out.append((H, p, kw, synd))
    return out


@functools.lru_cache(maxsize=None)
def rare_oracle():
    from oracle import oracle as O
    out = []
    for H, p, kw, synd in rare_problems(RARE_SEED, RARE_TRIALS, RARE_SHOTS):
        want, res = O.osd_window(H, channel_probs=p, **kw).decode_batch(synd)
        for a in (synd, want, res):
            a.setflags(write=False)
        out.append((H, p, kw, synd, want, res))
    return out


def test_b_rare_exits_on_small_random_matrices():
    probs = rare_oracle()
    counts = sum(np.bincount(res["exit_class"], minlength=5) for *_, res in probs)
    assert counts[3] >= 8 and counts[4] >= 8 and counts[1] >= 50 and counts[2] >= 20, counts  # the oracle's exits alone
    for t, (H, p, kw, synd, want, res) in enumerate(probs):
        assert H.shape[0] <= 64 and H.shape[1] <= 448 and H.sum(axis=0).max() <= 6
        check_window(H, p, kw, synd, want, res, f"trial {t}")


# ---- (c) ties on the boundary sum, no select, a slot table of odd length ---------------------------------------------------------------
def tie_problem(m_a, n_a, m_b, per_b, seed, shots):
    """m_a checks on n_a columns of degree 3 (prior 0.08) with random syndromes, beside m_b checks of per_b columns of degree 1 each
    (prior 0.001) with a zero syndrome; the columns are shuffled, so the blocks interleave in node order"""
    rng = np.random.default_rng(seed)
    n_b = m_b * per_b
    A = np.zeros((m_a, n_a), np.uint8)
    for c in range(n_a):
        A[rng.choice(m_a, 3, replace=False), c] = 1
    for r in np.flatnonzero(A.sum(axis=1) == 0):
        A[r, rng.integers(n_a)] = 1
    B = np.kron(np.eye(m_b, dtype=np.uint8), np.ones((1, per_b), np.uint8))
    H = np.block([[A, np.zeros((m_a, n_b), np.uint8)], [np.zeros((m_b, n_a), np.uint8), B]])
    pr = np.concatenate([np.full(n_a, 0.08), np.full(n_b, 0.001)])
    cp = rng.permutation(n_a + n_b)
    H, pr = H[:, cp], pr[cp]
    synd = np.zeros((shots, m_a + m_b), np.uint8)
    synd[:, :m_a] = rng.random((shots, m_a)) < rng.uniform(0.05, 0.4, size=(shots, 1))
    return sp.csr_matrix(H), pr, synd


def random_problem(m, n, seed, shots):
    rng = np.random.default_rng(seed)
    H = np.zeros((m, n), np.uint8)
    for c in range(n):
        H[rng.choice(m, int(rng.integers(2, 4)), replace=False), c] = 1
    for r in np.flatnonzero(H.sum(axis=1) == 0):
        H[r, rng.integers(n)] = 1
    pr = rng.uniform(0.01, 0.06, size=n)
    synd = np.zeros((shots, m), np.uint8)
    for k in range(shots):
        synd[k] = (H @ (rng.random(n) < 0.03).astype(np.uint8)) % 2 if k % 2 else rng.random(m) < 0.2
    return sp.csr_matrix(H), pr, synd


TIE_KW = dict(ms_scaling_factor=0.9, osd_method="osd_cs", osd_order=3)
# name: (problem, decoder arguments, kernel kind, (threads, nodes per thread), boundary ties asserted)
EDGE = {
    "tie_depth": (lambda: tie_problem(100, 400, 100, 8, 1, 24), dict(TIE_KW, pre_max_iter=4, post_max_iter=12, new_n=500), 3, (256, 7), True),
    "tie_small": (lambda: tie_problem(30, 90, 20, 6, 2, 24), dict(TIE_KW, pre_max_iter=3, post_max_iter=11, new_n=120), 0, (64, 4), True),
    "no_select": (lambda: random_problem(40, 150, 3, 24), dict(TIE_KW, pre_max_iter=3, post_max_iter=11, new_n=150), 0, (64, 4), False),
    "odd_slots": (lambda: random_problem(41, 151, 7, 24), dict(TIE_KW, pre_max_iter=3, post_max_iter=11), 0, (64, 4), False),
}


@functools.lru_cache(maxsize=None)
def edge_oracle(name):
    from oracle import oracle as O
    make, kw, kind, variant, ties = EDGE[name]
    H, pr, synd = make()
    want, res = O.osd_window(H, channel_probs=pr, **kw).decode_batch(synd)
    tied = 0
    if ties:  # shots that reach the select with more columns on the boundary sum than are decided
        aux, new_n = aux_oracle(H, pr, kw), default_new_n(H, kw)
        for k in np.flatnonzero(res["exit_class"] != 0):
            sums = history_sums(aux, synd[k])
            tied += int((sums == np.sort(sums, kind="stable")[new_n]).sum() > H.shape[1] - new_n)
    for a in (synd, want, res):
        a.setflags(write=False)
    return H, pr, synd, want, res, tied


@pytest.mark.parametrize("name", list(EDGE))
def test_c_boundary_ties_no_select_odd_slot_table(name):
    from slidingwindowdecoder_amd import window_forms
    _, kw, kind, variant, ties = EDGE[name]
    H, pr, synd, want, res, tied = edge_oracle(name)
    form = window_forms([(H, pr)], **kw)
    assert (form["nt"], form["vf"]) == variant, form
    if ties:
        assert tied >= 8, tied
    if name == "no_select":
        assert kw["new_n"] == H.shape[1]
    if name == "odd_slots":
        assert (H.nnz + form["windows"][0]["pads"]) % 4 != 0  # message slots of the layout: edges and pad cells
    if name == "tie_depth":
        assert form["depth_fit"] == 1
    assert (res["exit_class"] != 0).sum() >= 8  # shots that go through the passes between the phases
    check_window(H, pr, kw, synd, want, res, name, kind)
