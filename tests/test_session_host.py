"""The online form of the window loop on the host: ``sliding_window_decode_online_host`` (zero residual syndrome, XOR on arrival,
decode when ready, commit into rows that have not arrived yet) against ``sliding_window_decode_host`` with the oracle in the
windows -- the executable specification of ``SlidingWindowDecoder.session`` (tests/test_gpu_session.py)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

KW = dict(pre_max_iter=8, post_max_iter=40, ms_scaling_factor=1.0, osd_method="osd_cs", osd_order=4)
PLANS = {"w3f3m0": (3, 3, 0), "w3f1m1": (3, 1, 1)}


def chunkings(det, rows_per_round=36):
    """all rows at once; one round (``rows_per_round`` rows) per push; an irregular list with a one-row piece, one that ends a round,
    one that spans more than a round and ends off the word grid, an empty one and, where a round is no whole number of 32-bit
    words, a three-row piece"""
    n, h = det.shape[1], int(rows_per_round)

    def cut(sizes):
        out, r = [], 0
        for k in sizes:
            out.append(det[:, r:r + k])
            r += k
        assert r == n
        return out
    irregular = [1, h - 1, h + 14, 0, 22] + ([3] if h % 4 else [])  # (36 rows per round: 1, 35, 50, 0, 22)
    assert n % h == 0 and sum(irregular) <= n
    return {"whole": cut([n]), "rounds": cut([h] * (n // h)), "irregular": cut(irregular + [n - sum(irregular)])}


@functools.lru_cache(maxsize=None)
def experiment(tag, shots=16, seed=7):
    """[[72,12,6]], 6 rounds, p = 0.004: (plan, det, total_e_hat of the offline host loop with the oracle)"""
    from oracle import oracle as O
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows, sample_dem, sliding_window_decode_host
    code, A, B = bb_code(72)
    dem = bb_dem(code, A, B, 0.004, 6)
    W, F, method = PLANS[tag]
    plan = plan_windows(dem.chk, dem.obs, dem.priors, 36, W, F, method=method)
    assert plan.chk.shape == (252, 2232)
    det, _, _ = sample_dem(plan.chk, plan.obs, plan.priors, shots, seed=seed)
    want, _ = sliding_window_decode_host(plan, det, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW))
    want.setflags(write=False)
    det.setflags(write=False)
    return plan, det, want


def test_commit_reaches_rows_that_have_not_arrived():
    """(3, 3, method 0): window 0 is ready after 108 rows and its committed columns touch rows up to 143 -- the XOR into rows that
    arrive later is exercised; (3, 1, method 1) never needs it (its commits stay inside the rows received)."""
    plan = experiment("w3f3m0")[0]
    assert [(w.row0, w.row1) for w in plan.windows] == [(0, 108), (108, 216), (216, 252)]
    w0 = plan.windows[0]
    cols = sp.csc_matrix(plan.chk)[:, w0.col0:w0.col0 + w0.commit]
    assert cols.indices.max() >= w0.row1
    plan1 = experiment("w3f1m1")[0]
    for w in plan1.windows:
        assert sp.csc_matrix(plan1.chk)[:, w.col0:w.col0 + w.commit].indices.max() < w.row1


@pytest.mark.parametrize("chunking", ["whole", "rounds", "irregular"])
@pytest.mark.parametrize("tag", sorted(PLANS))
def test_online_host_loop_equals_the_offline_loop(tag, chunking):
    from oracle import oracle as O
    from slidingwindowdecoder_amd.windows import sliding_window_decode_online_host
    plan, det, want = experiment(tag)
    chunks = chunkings(det)[chunking]
    total, events, resid = sliding_window_decode_online_host(plan, chunks, lambda w: O.osd_window(w.mat, channel_probs=w.prior, **KW))
    assert np.array_equal(total, want)
    # every chunk returned exactly the windows it completed, with the faults they committed
    rows, nxt = 0, 0
    for ch, ev in zip(chunks, events):
        rows += ch.shape[1]
        ready = []
        while nxt < len(plan.windows) and rows >= plan.windows[nxt].row1:
            ready.append(nxt)
            nxt += 1
        assert [e[0] for e in ev] == ready
        for t, col0, faults in ev:
            w = plan.windows[t]
            assert col0 == w.col0 and np.array_equal(faults, want[:, w.col0:w.col0 + w.commit])
    assert nxt == len(plan.windows)
    # the residual syndrome of the whole run (flagged = any, osd.py:184-187)
    full = (det.astype(np.int32) + (sp.csr_matrix(want) @ sp.csr_matrix(plan.chk.T.astype(np.int32))).toarray()) % 2
    assert np.array_equal(resid, full.astype(np.uint8))
    assert want.any()
