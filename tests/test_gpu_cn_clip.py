"""The check pass of bp_run (csrc/swd_osdw_kernel.h) in the tuned osd_window kernels of up to 256 threads clips once per check: the walk
keeps the two smallest |x| and min(., 50) is applied to the two minima behind the quad merges (tests/test_cn_clip_host.py restates the
argument on the CPU).  Here osd_window runs through the C ABI on priors that make the clip engage and is compared with the oracle by
== -- decoded vectors, exit class, bp_iteration, min_pm -- with the kernel and the post form asserted through the form report.

Shapes: the three of tests/test_gpu_cn_pass.py (its helpers are imported, the file is not edited): 64 x 320 (<256, 2, 16>, live-slot
lists), 64 x 600 (<256, 4, 16>, sorted form), 200 x 1100 (<256, 7, 9>: 36 positions, a partly filled second sign register); 64
syndromes each.  Priors: seven columns in ten have channel probability 1e-25 or 1e-30 (LLR 57.6 and 69.1, the second above the far
slot's 64.0) -- nineteen in twenty of the columns of the heaviest checks, the ones that get shared --, the rest 0.01 .. 0.1.

Situations, asserted on the CPU from a restatement of the messages in front of the check passes (messages_before_passes, an extension
of min_sum_messages of tests/test_gpu_cn_pass.py by the scaling factor):
 1. min1 < 50 <= min2, unclipped: a check with exactly one position below the clip;
 2. both minima >= 50: a check whose positions all hold |x| >= 50;
 3. a walked dead position beside live values in (50, 64) and above 64: a check of the full graph whose weight is no multiple of four
    -- groups are walked whole, so the positions behind its weight read the far slot whichever wave serves it -- with both kinds of value;
 4. a shared check, served by two or four threads, one of whose partial walks sees only values >= 50: the first check pass of the post
    phase reads the priors of the live nodes; the live weights and the split bound T are recomputed from the oracle's history with the
    rule of cn_assign, and a check served by g threads with fewer than g live positions below the clip has such a partial walk
    whichever order its positions are walked in (g walks, fewer than g small values), so the assertion does not depend on the form
    of the shortened graph's caches.
1 - 3 must occur in the first check pass of the pre phase (it reads the priors) and, where the pre phase has a second one (CASES), in that
one too; 4 needs a shot that reaches the post phase and is asserted per shape.  All three exits -- pre, post, OSD -- must occur."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_gpu_between_phases import aux_oracle, default_new_n, history_sums
from tests.test_gpu_cn_pass import SHAPES, graph_a, problem_e, run_case, split_of, with_oracle

pytestmark = pytest.mark.gpu

CLIP, FAR = 50.0, 64.0
P_HIGH = (1e-25, 1e-30)
SHOTS = 64


def clip_priors(H, seed):
    """seven columns in ten far above the clip, nineteen in twenty of those the heaviest checks touch (they are the shared ones)"""
    rng = np.random.default_rng(seed)
    n = H.shape[1]
    rw = H.sum(axis=1)
    heavy = H[rw >= min(20, int(rw.max()))].any(axis=0)
    pr = rng.uniform(0.01, 0.1, size=n)
    high = rng.random(n) < np.where(heavy, 0.95, 0.7)
    pr[high] = rng.choice(P_HIGH, size=int(high.sum()))
    return pr


def messages_before_passes(H, llr, synd, passes, alpha):
    """variable-to-check messages in front of check passes 1 .. passes of the full graph, a list of [edges] arrays in CSR order: the
    flooding iteration of min_sum_messages (tests/test_gpu_cn_pass.py) with the scaling factor alpha"""
    H = sp.csr_matrix(H)
    m, n = H.shape
    Hc = sp.csc_matrix(H)
    pos = sp.csr_matrix((np.arange(1, H.nnz + 1), H.indices, H.indptr), shape=H.shape).tocsc()  # CSR edge number + 1, by column
    b2c = llr[H.indices].astype(np.float64)
    out = [b2c.copy()]
    for _ in range(passes - 1):
        c2b = np.empty_like(b2c)
        for r in range(m):
            e = slice(H.indptr[r], H.indptr[r + 1])
            x = np.clip(b2c[e], -CLIP, CLIP)
            a, neg = np.abs(x), x <= 0
            par = (int(synd[r]) + int(neg.sum())) & 1
            order = np.argsort(a, kind="stable")
            mag = np.full(a.size, a[order[0]] if a.size else 1e308)
            if a.size:
                mag[order[0]] = a[order[1]] if a.size > 1 else 1e308
            c2b[e] = np.where((par ^ neg.astype(np.int64)) == 1, -mag, mag) * alpha
        for v in range(n):
            es = pos.data[Hc.indptr[v]:Hc.indptr[v + 1]] - 1  # the node's edges by increasing row
            tot, pre = llr[v], []
            for e in es:
                pre.append(tot)
                tot = tot + c2b[e]
            suf = 0.0
            for k in range(len(es) - 1, -1, -1):
                b2c[es[k]] = pre[k] + suf
                suf = suf + c2b[es[k]]
        out.append(b2c.copy())
    return out


def situations(H, msgs):
    """which of the situations 1 - 3 the check pass that reads `msgs` holds (one flag each)"""
    H = sp.csr_matrix(H)
    got = [False, False, False]
    for r in range(H.shape[0]):
        a = np.sort(np.abs(msgs[H.indptr[r]:H.indptr[r + 1]]))
        if a.size >= 2:
            got[0] |= bool(a[0] < CLIP <= a[1])
            got[1] |= bool(a[0] >= CLIP)
        # (whole groups are walked, so a weight that is no multiple of four has far-slot positions in its last group whichever wave and
        # walk bound the check is dealt to)
        got[2] |= bool(a.size % 4 != 0 and ((a > CLIP) & (a < FAR)).any() and (a > FAR).any())
    return got


def live_columns(H, sums, new_n):
    """live nodes of the shortened graph and the live weight of every check, as live_check_weights of tests/test_gpu_cn_pass.py"""
    H = sp.csr_matrix(H)
    live = np.ones(H.shape[1], bool)
    live[np.argsort(sums, kind="stable")[new_n:]] = False
    while True:
        deg = H @ live.astype(np.int64)
        ones = np.flatnonzero(deg == 1)
        if ones.size == 0:
            return live, deg
        cols = H[ones].indices
        live[cols[live[cols]]] = False


def shared_walk_all_high(H, llr, live, deg, kg):
    """situation 4 for one shot: (a check served by two threads, by four threads) has a partial walk over values >= 50 only"""
    T, nq, np_ = split_of(deg, 256, kg)
    small = sp.csr_matrix(H) @ (live & (np.abs(llr) < CLIP)).astype(np.int64)  # live positions below the clip, per check
    pair = (deg > T) & (deg <= 2 * T) & (small < 2) & (deg - small >= 1)
    quad = (deg > 2 * T) & (small < 4) & (deg - small >= 1)
    return bool(pair.any()), bool(quad.any())


def assert_situations(H, pr, kw, synd, res, kg, tag):
    llr = np.log((1 - pr) / pr)
    assert ((llr > CLIP) & (llr < FAR)).any() and (llr > FAR).any() and (llr < CLIP).any()
    passes = min(3, kw["pre_max_iter"])
    first, later = [False] * 3, [passes == 1] * 3
    for k in range(0, len(synd), 16):  # four syndromes: the first pass is the same for all of them
        msgs = messages_before_passes(H, llr, synd[k], passes, kw["ms_scaling_factor"])
        first = [a or b for a, b in zip(first, situations(H, msgs[0]))]
        for mm in msgs[1:]:
            later = [a or b for a, b in zip(later, situations(H, mm))]
    assert all(first) and all(later), (tag, first, later)
    assert (res["bp_iteration"] >= 3).sum() >= len(synd) // 4, tag  # ... and the device runs check passes beyond the first
    aux, new_n = aux_oracle(H, pr, kw), default_new_n(H, kw)
    shared = 0
    for k in np.flatnonzero((res["exit_class"] == 1) | (res["exit_class"] == 2)):
        live, deg = live_columns(H, history_sums(aux, synd[k]), new_n)
        shared += any(shared_walk_all_high(H, llr, live, deg, kg))
    assert shared >= 4, (tag, shared)
    hist = np.bincount(res["exit_class"], minlength=3)
    assert hist[:3].min() >= 3, (tag, hist)  # pre-processing BP, post-processing BP, OSD


KW = dict(pre_max_iter=2, post_max_iter=24, ms_scaling_factor=0.9, osd_method="osd_cs", osd_order=2)
# (pre-phase iterations, error rate as a multiple of the priors, seed of the syndromes): chosen on the CPU so that every exit occurs; on the 64 x 600 graph BP
# converges within two iterations or not at all, so its post phase gets its chance after one -- its later passes are those of the post phase
CASES = {"small": (2, 0.6, 32), "sorted": (1, 0.2, 32), "nine": (2, 0.35, 35)}


def clip_syndromes(H, pr, shots, seed, scale):
    """one in eight random bits, the rest from errors on the columns with an ordinary prior, at scale x (0.5 .. 2) x their prior"""
    rng = np.random.default_rng(seed)
    m, n = H.shape
    low = pr > 1e-3
    synd = np.zeros((shots, m), np.uint8)
    for k in range(shots):
        if k % 8 == 0:
            synd[k] = rng.random(m) < rng.uniform(0.02, 0.4)
        else:
            synd[k] = (H @ ((rng.random(n) < pr * scale * (0.5 + 1.5 * k / shots)) & low).astype(np.uint8)) % 2
    return synd


@functools.lru_cache(maxsize=None)
def problem(shape):
    H = problem_e()[0] if shape == "nine" else graph_a(SHAPES[shape][0])
    pr = clip_priors(H, 31)
    kw = dict(KW, pre_max_iter=CASES[shape][0])
    if shape != "nine":  # (200 x 1100 keeps the default, 2 m nodes: the sorted form, as in tests/test_gpu_cn_pass.py)
        kw["new_n"] = H.shape[1] * 5 // 8
    return with_oracle(H, pr, kw, clip_syndromes(H, pr, SHOTS, CASES[shape][2], CASES[shape][1]))


@pytest.mark.parametrize("shape", ["small", "sorted", "nine"])
def test_clip_engaged_every_exit(shape):
    H, pr, kw, synd, want, res = problem(shape)
    n, variant, post = SHAPES[shape] if shape in SHAPES else (1100, (256, 7, 9), "sorted")
    assert H.shape[1] == n and len(synd) <= 64
    assert_situations(H, pr, kw, synd, res, variant[2], shape)
    run_case(H, pr, kw, synd, want, res, variant, "clip " + shape, post)
