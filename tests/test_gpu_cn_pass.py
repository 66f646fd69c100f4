"""The check pass of bp_run (csrc/swd_osdw_kernel.h) in the tuned osd_window kernels of up to 256 threads: the groups of four
positions form a chain that is left behind the wave's last live group (scalar compares against the wave's walk bound) and the sign
registers are aligned by one shift behind the chain.  Neither changes a result: every case runs osd_window through the C ABI and
compares with the oracle by == -- decoded vectors, exit class, bp_iteration, min_pm -- and asserts through the form report which
tuned 256-thread kernel and which post form were taken.

Shapes.  The issue of this round set m <= 64, n <= 448 and column weight <= 6 for cases (a) - (d) and asked for the sorted post form.
No graph has both: the first variant that fits such a graph (csrc/swd_variants.h) is <256, 2, 8, 16> for 256 < n <= 448 -- a tuned
256-thread kernel with sixteen groups and two sign registers -- and the sorted form is built for more than two nodes per thread only
(swd_post_sorted_built).  So (a) - (d) run at two shapes: "small", 64 x 320, the issue's shape, which takes the live-slot lists, and
"sorted", 64 x 600, which takes <256, 4, 8, 16> and the sorted form; the post form is asserted for each.

Cases:
 (a) group boundaries: row weights 1, 3, 4, 5, 8, 9, 12, 13, 32, 33, 36 (and others) in one graph, rows shuffled; syndromes from
     sparse errors and random bits, so that the oracle leaves through pre-processing BP, post-processing BP and the OSD (asserted).
     With m <= 64 every check of the full graph is served by the first wave (walk bound 36: nine of sixteen groups) and the other
     three waves walk no group at all; the post phase deals the live checks by decreasing live weight, so its waves differ.
 (b) quad sharing: the same graph with priors and new_n chosen so that the shortened graph keeps checks heavier than the split bound
     T; the live weights are recomputed here from the oracle's history and the rule of cn_assign is restated to assert that checks
     served by two and by four threads occur.
 (c) exact zeros: uniform priors, scaling factor 1, syndromes of weight 1 - 3.  A node of weight 2 beside an unsatisfied check whose
     other messages are all positive receives -L and sends L + (-L) = +0.0 to its other check; the reference counts x <= 0 as
     negative, so the sign bit alone would be wrong.  min_sum_messages() restates the first three iterations; at least a quarter of
     the syndromes must hold an exactly-zero variable-to-check message (asserted here, checked on the CPU when the inputs were chosen).
 (d) a check of weight 1 in the last lane of a wave (row 63): its minimum runs over no other edge.  The issue of this round asked for
     such a check in the shortened graph; there is none to be had -- the peeling step in front of the post phase runs to closure
     (oracle/swd_oracle.c, osdw_peel), so no live check of the shortened graph has one live edge, which the test asserts from the
     oracle's history -- and the full graph is where `cn.live == 1` is met.
 (e) nine groups and a partly filled second sign register: a 200 x 1100 graph takes the <256, 7, 6, 9> kernels (K4 = 36); its rows are
     ordered so that the three waves holding checks have walk bounds 36, 12 and 5."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_gpu_between_phases import aux_oracle, default_new_n, history_sums

pytestmark = pytest.mark.gpu

WEIGHTS_A = (1, 3, 4, 5, 8, 9, 12, 13, 32, 33, 36)


def weighted_graph(row_w, n, seed, max_col=6):
    """rows of the given weights on n columns, every column used, no column heavier than max_col: each row takes the lightest
    columns, ties broken at random"""
    rng = np.random.default_rng(seed)
    m = len(row_w)
    assert n <= sum(row_w) <= max_col * n
    H = np.zeros((m, n), np.uint8)
    cw = np.zeros(n, np.int64)
    for r in np.argsort(-np.asarray(row_w), kind="stable"):  # heavy rows first: they need the most distinct columns
        cols = np.lexsort((rng.random(n), cw))[:row_w[r]]
        H[r, cols] = 1
        cw[cols] += 1
    assert cw.min() >= 1 and cw.max() <= max_col and np.array_equal(H.sum(axis=1), row_w)
    return H


def mixed_syndromes(H, shots, seed, p_err=0.01):
    """three in four from sparse errors of rate p_err .. 2 p_err, the rest random bits"""
    rng = np.random.default_rng(seed)
    m, n = H.shape
    synd = np.zeros((shots, m), np.uint8)
    for k in range(shots):
        if k % 4:
            synd[k] = (H @ (rng.random(n) < p_err * (1 + k / shots)).astype(np.uint8)) % 2
        else:
            synd[k] = rng.random(m) < rng.uniform(0.02, 0.4)
    return synd


def live_check_weights(H, sums, new_n):
    """live weight of every check of the shortened graph (0: cleared), as live_words of tests/test_gpu_between_phases.py"""
    H = sp.csr_matrix(H)
    live = np.ones(H.shape[1], bool)
    live[np.argsort(sums, kind="stable")[new_n:]] = False
    while True:
        deg = H @ live.astype(np.int64)
        ones = np.flatnonzero(deg == 1)
        if ones.size == 0:
            return deg
        cols = H[ones].indices
        live[cols[live[cols]]] = False


def split_of(deg, nt, kg):
    """(T, checks served by four threads, by two) for the live weights `deg`: the rule of cn_assign (csrc/swd_osdw_kernel.h)"""
    d = deg[deg > 0]
    for T in (3, 4, 6, 8, 12, 16, 24, 32):
        need = int(np.where(d <= T, 1, np.where(d <= 2 * T, 2, 4)).sum())
        if d.max() <= 4 * T and need <= nt and T <= 4 * kg:
            return T, int((d > 2 * T).sum()), int(((d > T) & (d <= 2 * T)).sum())
    return 64, 0, 0


def min_sum_messages(H, llr, synd, iters):
    """variable-to-check messages in front of the check passes 2 .. iters + 1 of the full graph, [iters, edges]: one flooding
    iteration as minsum_iteration of oracle/swd_oracle.c (scaling factor 1)"""
    H = sp.csr_matrix(H)
    m, n = H.shape
    rows = [H.indices[H.indptr[r]:H.indptr[r + 1]] for r in range(m)]
    b2c = {(r, int(v)): float(llr[v]) for r in range(m) for v in rows[r]}
    Hc = H.tocsc()
    colrows = [Hc.indices[Hc.indptr[v]:Hc.indptr[v + 1]] for v in range(n)]
    out = []
    for _ in range(iters):
        c2b = {}
        for r in range(m):
            x = np.clip(np.array([b2c[(r, int(v))] for v in rows[r]]), -50.0, 50.0)
            a, neg = np.abs(x), x <= 0
            par = (int(synd[r]) + int(neg.sum())) & 1
            for j, v in enumerate(rows[r]):
                others = np.delete(a, j)
                mag = others.min() if others.size else 1e308
                c2b[(r, int(v))] = -mag if (par ^ int(neg[j])) else mag
        for v in range(n):
            tot = llr[v]
            pre = []
            for r in colrows[v]:
                pre.append(tot)
                tot = tot + c2b[(int(r), v)]
            suf = 0.0
            for k in range(len(colrows[v]) - 1, -1, -1):
                r = int(colrows[v][k])
                b2c[(r, v)] = pre[k] + suf
                suf = suf + c2b[(r, v)]
        out.append(np.array([b2c[k] for k in sorted(b2c)]))
    return np.array(out)


SHAPES = {"small": (320, (256, 2, 16), "lists"), "sorted": (600, (256, 4, 16), "sorted")}


def run_case(H, pr, kw, synd, want, res, variant, tag, post="sorted"):
    from slidingwindowdecoder_amd import osd_window
    dev = osd_window(H, channel_probs=pr, **kw)
    out = dev.decode_batch(synd)
    form = dev.last_form
    assert (form["nt"], form["vf"], form["kg"]) == variant and form["big"] == 0 and form["kind"] in (0, 3), f"{tag}: {form}"
    assert form["windows"][0]["post"] == post, f"{tag}: {form['windows'][0]}"
    bad = np.flatnonzero((out != want).any(axis=1))
    assert bad.size == 0, f"{tag}: shots {bad[:8].tolist()} differ, oracle exits {res['exit_class'][bad[:8]].tolist()}"
    assert np.array_equal(dev.last_status & 0xFF, res["exit_class"]), tag
    assert np.array_equal(dev.last_iterations, res["bp_iteration"]), tag
    assert np.array_equal(dev.last_min_pm, res["min_pm"]), tag


def with_oracle(H, pr, kw, synd):
    from oracle import oracle as O
    want, res = O.osd_window(H, channel_probs=pr, **kw).decode_batch(synd)
    for a in (synd, want, res):
        a.setflags(write=False)
    return H, pr, kw, synd, want, res


@functools.lru_cache(maxsize=None)
def graph_a(n):
    rng = np.random.default_rng(3)
    lo, hi = (2, 11) if n <= 448 else (6, 15)
    w = list(WEIGHTS_A) + rng.integers(lo, hi, size=64 - len(WEIGHTS_A)).tolist()
    w = [w[i] for i in rng.permutation(64)]
    k = w.index(1)
    w[k], w[63] = w[63], w[k]  # (d): the check of weight 1 in the last lane of the first wave
    return weighted_graph(w, n, 4)


KW_A = dict(pre_max_iter=4, post_max_iter=24, ms_scaling_factor=0.9, osd_method="osd_cs", osd_order=2)


@functools.lru_cache(maxsize=None)
def problem_a(shape):
    H = graph_a(SHAPES[shape][0])
    pr = np.random.default_rng(5).uniform(0.01, 0.08, size=H.shape[1])
    if shape == "small":
        return with_oracle(H, pr, KW_A, mixed_syndromes(H, 400, 6, 0.008))
    # 64 x 600: BP converges within three iterations or not at all, so the post phase gets its chance after one iteration
    return with_oracle(H, pr, dict(KW_A, pre_max_iter=1), mixed_syndromes(H, 400, 6, 0.001))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_group_boundaries_every_exit(shape):
    H, pr, kw, synd, want, res = problem_a(shape)
    n, variant, post = SHAPES[shape]
    assert H.shape == (64, n) and H.sum(axis=0).max() <= 6 and set(WEIGHTS_A) <= set(H.sum(axis=1).tolist())
    hist = np.bincount(res["exit_class"], minlength=3)
    assert hist[:3].min() >= 4, hist  # pre-processing BP, post-processing BP, OSD (the post phase seldom converges on these graphs)
    run_case(H, pr, kw, synd, want, res, variant, "a " + shape, post)


@functools.lru_cache(maxsize=None)
def problem_b(shape):
    H = graph_a(SHAPES[shape][0])
    pr = np.random.default_rng(7).uniform(0.02, 0.1, size=H.shape[1])
    kw = dict(KW_A, post_max_iter=12, new_n=H.shape[1] * 5 // 8)
    return with_oracle(H, pr, kw, mixed_syndromes(H, 64, 8, p_err=0.03))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_b_checks_shared_by_two_and_four_threads(shape):
    H, pr, kw, synd, want, res = problem_b(shape)
    n, variant, post = SHAPES[shape]
    aux, new_n = aux_oracle(H, pr, kw), default_new_n(H, kw)
    pairs = quads = 0
    for k in np.flatnonzero((res["exit_class"] == 1) | (res["exit_class"] == 2)):
        T, nq, np_ = split_of(live_check_weights(H, history_sums(aux, synd[k]), new_n), 256, 16)
        quads += nq > 0
        pairs += np_ > 0
    assert pairs >= 8 and quads >= 8, (pairs, quads)
    run_case(H, pr, kw, synd, want, res, variant, "b " + shape, post)


KW_C = dict(pre_max_iter=4, post_max_iter=8, ms_scaling_factor=1.0, osd_method="osd_cs", osd_order=2)


@functools.lru_cache(maxsize=None)
def problem_c(shape):
    n = SHAPES[shape][0]
    rng = np.random.default_rng(11)
    H = weighted_graph(rng.integers(n // 40, n // 20, size=48).tolist(), n, 12)
    pr = np.full(n, 0.03)
    synd = np.zeros((48, 48), np.uint8)
    for k in range(48):
        synd[k, rng.choice(48, 1 + k % 3, replace=False)] = 1
    return with_oracle(H, pr, KW_C, synd)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_c_exact_zero_messages(shape):
    H, pr, kw, synd, want, res = problem_c(shape)
    n, variant, post = SHAPES[shape]
    llr = np.log((1 - pr) / pr)
    half = range(0, len(synd), 2)  # every other syndrome
    zeros = sum(bool((min_sum_messages(H, llr, synd[k], 3) == 0.0).any()) for k in half)
    assert 4 * zeros >= len(half), zeros
    assert (res["bp_iteration"] >= 4).sum() >= len(synd) // 2  # ... and the device runs the check passes that read them
    run_case(H, pr, kw, synd, want, res, variant, "c " + shape, post)


@functools.lru_cache(maxsize=None)
def problem_d(shape):
    H, pr, kw, synd, *_ = problem_a(shape)
    synd = synd[:48].copy()
    synd[:, 63] = 1  # the check of weight 1 unsatisfied in every shot
    return with_oracle(H, pr, kw, synd)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_d_weight_one_check_in_the_last_lane(shape):
    H, pr, kw, synd, want, res = problem_d(shape)
    n, variant, post = SHAPES[shape]
    assert H[63].sum() == 1
    aux, new_n = aux_oracle(H, pr, kw), default_new_n(H, kw)
    for k in np.flatnonzero((res["exit_class"] == 1) | (res["exit_class"] == 2))[:16]:
        assert not (live_check_weights(H, history_sums(aux, synd[k]), new_n) == 1).any()  # peeled to closure: see (d) above
    run_case(H, pr, kw, synd, want, res, variant, "d " + shape, post)


KW_E = dict(pre_max_iter=4, post_max_iter=24, ms_scaling_factor=0.9, osd_method="osd_cs", osd_order=2)


@functools.lru_cache(maxsize=None)
def problem_e():
    rng = np.random.default_rng(21)
    w = [36, 35, 33, 32, 29, 28] + rng.integers(5, 25, size=58).tolist() + [12] + rng.integers(3, 13, size=63).tolist() \
        + [5] + rng.integers(1, 6, size=71).tolist()
    H = weighted_graph(w, 1100, 22)
    pr = rng.uniform(0.005, 0.04, size=1100)
    return with_oracle(H, pr, KW_E, mixed_syndromes(H, 96, 23, p_err=0.0015))


def test_e_nine_groups_three_walk_bounds():
    H, pr, kw, synd, want, res = problem_e()
    rw = H.sum(axis=1)
    assert H.shape == (200, 1100) and (rw[:64].max(), rw[64:128].max(), rw[128:].max()) == (36, 12, 5)
    hist = np.bincount(res["exit_class"], minlength=3)
    assert hist[:3].min() >= 4, hist
    run_case(H, pr, kw, synd, want, res, (256, 7, 9), "e")
