"""Rolling memory experiments on the host: ``windows.extend_template`` -- the detector error model of R rounds built from a template
of R0 rounds -- against ``plan_windows(bb_dem(R))`` itself, ``windows.rolling_schedule`` against the rolling host loop, and the numpy
restatement of the rolling DEM sampler (``rows_ref``: tests/philox_ref.py on the extension, drawn column block by column block)
that tests/test_gpu_rolling_experiment.py holds the device to.  [[72,12,6]], p = 0.004, and a hand-made periodic model in which
nothing is aligned to four."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from tests import philox_ref
from tests.test_rolling_host import TEMPLATES, plan_for, template_plan

H = 36


@functools.lru_cache(maxsize=None)
def xplan(rounds, z_basis=False):
    """the (3, 1) plan of the X-basis experiment (the templates of tests/test_rolling_host.py are all Z-basis)"""
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows
    code, A, B = bb_code(72)
    dem = bb_dem(code, A, B, 0.004, rounds, z_basis=z_basis)
    return plan_windows(dem.chk, dem.obs, dem.priors, H, 3, 1, method=1, z_basis=z_basis)


def same(a, b):
    return a.shape == b.shape and (sp.csr_matrix(a) != sp.csr_matrix(b)).nnz == 0


@pytest.mark.parametrize("tag", sorted(TEMPLATES) + ["xbasis"])
def test_extension_equals_the_plan_of_the_experiments_own_length(tag):
    from slidingwindowdecoder_amd.windows import extend_template, extended_block_cols, rolling_template, template_blocks
    tp = xplan(6) if tag == "xbasis" else template_plan(tag)
    T = rolling_template(tp)
    j0, j1, cols = template_blocks(T)
    assert cols[j0] == T.body.col0 and cols[j1] == T.tail.col0 and len(cols) == T.R0 + 2
    for R in range(T.min_rounds, T.R0 + 2 * T.F + 1):
        plan = xplan(R) if tag == "xbasis" else plan_for(tag, R)
        chk, obs, priors = extend_template(T if R & 1 else tp, R)  # (a template and a plan are both taken)
        assert same(chk, plan.chk) and same(obs, plan.obs), (tag, R)
        assert np.array_equal(priors, plan.priors), (tag, R)
        assert np.array_equal(extended_block_cols(cols, j0, j1, R), [a[1] for a in plan.anchors]), (tag, R)
    with pytest.raises(ValueError, match="this template serves"):
        extend_template(T, T.min_rounds - 1)


@pytest.mark.parametrize("tag", sorted(TEMPLATES))
def test_schedule_is_head_then_strides_then_tail(tag):
    from slidingwindowdecoder_amd.windows import rolling_schedule, rolling_template, sliding_window_decode_rolling_host
    W, F, method, R0 = TEMPLATES[tag]
    T = rolling_template(template_plan(tag))

    class Zero:  # a window decoder that commits nothing: the loop's bookkeeping alone
        def __init__(self, w):
            self.n = w.mat.shape[1]

        def decode(self, s):
            return np.zeros(self.n, np.uint8)

    for R in (T.min_rounds, R0, R0 + F, R0 + 5 * F):
        sched = rolling_schedule(T if R & 1 else template_plan(tag), R)
        assert sched[0] == (0, W) and all(n == F for _, n in sched[1:-1]) and sched[-1][1] >= 1
        assert [b for b, _ in sched] == list(np.cumsum([0] + [n for _, n in sched[:-1]])) and sum(n for _, n in sched) == R + 1
        assert len(sched) == len(plan_for(tag, R).windows)
        det = np.zeros((1, H * (R + 1)), np.uint8)
        chunks = [det[:, H * b:H * (b + n)] for b, n in sched[:-1]]
        b, n = sched[-1]
        events, _, _ = sliding_window_decode_rolling_host(T, chunks, det[:, H * b:H * (b + n)], Zero)
        assert [t for t, _ in events] == list(range(len(sched)))  # the non-final entries make the windows before finish, finish the tail
        # ... one window per entry: entry k ends on the last row of window k of the plan of the experiment's own length
        assert [H * (b0 + n0) for b0, n0 in sched[:-1]] == [w.row1 for w in plan_for(tag, R).windows[:-1]]
    for R in (T.min_rounds - F, T.min_rounds - 1, 0) + ((R0 + 1,) if F > 1 else ()):
        with pytest.raises(ValueError) as e:
            rolling_schedule(T, R)
        assert T.lengths() in str(e.value)


# ---- the hand-made periodic model and the restatement of the rolling sampler --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def handmade():
    """(chk, obs, priors, n_half, j0, j1, anchor_cols): 6 row blocks of h = 5 rows (R0 = 5); column blocks of 3 | 7 7 7 | 6 4 columns:
    c0 = 3, cs = 7, so no block starts on a multiple of four; every column of block b touches rows of blocks b and b + 1 only (the
    last block: its own), the body blocks are translates; 3 observables; priors 0.25 .. 0.35, so that every column faults often"""
    rng = np.random.default_rng(20240318)
    h, lens, j0, j1 = 5, [3, 7, 7, 7, 6, 4], 1, 4
    nblk = len(lens)

    def block(n, last):
        cols = []
        for i in range(n):
            rows = rng.choice(h if last else 2 * h, size=int(rng.integers(1, 4)), replace=False)
            if i == 0:
                rows[0] = 0  # (the block's first column reaches its anchor row)
            if i == 1:
                rows[0] = (h if last else 2 * h) - 1  # ... and another one the last row it may: that of the next block
            cols.append((np.unique(rows), int(rng.integers(0, 8)), float(rng.uniform(0.25, 0.35))))
        return cols

    body = block(7, False)
    blocks = [block(lens[0], False)] + [body] * 3 + [block(lens[4], False), block(lens[5], True)]
    r, c, masks, priors, col = [], [], [], [], 0
    for b, blk in enumerate(blocks):
        for rows, mask, p in blk:
            r += [b * h + int(x) for x in rows]
            c += [col] * len(rows)
            masks.append(mask)
            priors.append(p)
            col += 1
    chk = sp.csr_matrix((np.ones(len(r), np.uint8), (r, c)), shape=(nblk * h, col))
    m = np.array(masks)
    obs = sp.csr_matrix(((m[None, :] >> np.arange(3)[:, None]) & 1).astype(np.uint8))
    anchor_cols = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return chk, obs, np.array(priors), h, j0, j1, anchor_cols


def flips_of(obs_bits):
    return (obs_bits.astype(np.uint32) << np.arange(obs_bits.shape[1], dtype=np.uint32)).sum(axis=1).astype(np.uint32)


def rows_ref(ext, block_cols, h, block0, nblocks, shots, seed, first_shot=0):
    """What one call of the rolling sampler returns, restated: only the column blocks ``block0 - 1 .. block0 + nblocks - 1`` of the
    extension ``ext = (chk, obs, priors)`` are drawn (Philox on the GLOBAL column number); -> (rows [shots, nblocks * h] of row
    blocks ``block0 ..``, observable masks uint32 [shots] of the faults in column blocks ``block0 .. block0 + nblocks - 1``, those
    faults [shots, columns of these blocks])"""
    chk, obs, priors = ext
    e = philox_ref.sample_faults(priors, shots, seed, first_shot)
    lo, mid, hi = int(block_cols[max(block0 - 1, 0)]), int(block_cols[block0]), int(block_cols[block0 + nblocks])
    drawn = np.zeros_like(e)
    drawn[:, lo:hi] = e[:, lo:hi]
    det = (sp.csr_matrix(drawn.astype(np.int32)) @ sp.csr_matrix(chk).T.astype(np.int32)).toarray() % 2
    counted = sp.csr_matrix(e[:, mid:hi].astype(np.int32))
    ob = (counted @ sp.csr_matrix(obs)[:, mid:hi].T.astype(np.int32)).toarray() % 2
    return det[:, block0 * h:(block0 + nblocks) * h].astype(np.uint8), flips_of(ob), e[:, mid:hi]


def whole_ref(ext, shots, seed, first_shot=0):
    """``DemSampler``'s restatement on the whole extension: (det, observable masks, faults)"""
    chk, obs, priors = ext
    e = philox_ref.sample_faults(priors, shots, seed, first_shot)
    s = sp.csr_matrix(e.astype(np.int32))
    det = (s @ sp.csr_matrix(chk).T.astype(np.int32)).toarray() % 2
    ob = (s @ sp.csr_matrix(obs).T.astype(np.int32)).toarray() % 2
    return det.astype(np.uint8), flips_of(ob), e


def chunked(nblocks_total, kind):
    """block ranges that cover ``0 .. nblocks_total``: one at a time, two at a time, uneven pieces"""
    if kind == "ones":
        sizes = [1] * nblocks_total
    elif kind == "twos":
        sizes = [2] * (nblocks_total // 2) + [1] * (nblocks_total % 2)
    else:
        sizes, left, k = [], nblocks_total, 0
        while left:
            sizes.append(min(left, (3, 1, 4, 2)[k % 4]))
            left, k = left - sizes[-1], k + 1
    starts = np.cumsum([0] + sizes[:-1])
    return [(int(b), int(n)) for b, n in zip(starts, sizes)]


@pytest.mark.parametrize("rounds", [2, 5, 6, 11])
def test_restated_sampler_is_chunk_invariant_on_the_handmade_model(rounds):
    """rounds = 2: every body block gone (head block, two tail blocks); 5: the model itself; 11: nine body blocks"""
    from slidingwindowdecoder_amd.windows import extend_periodic, extended_block_cols
    chk, obs, priors, h, j0, j1, cols = handmade()
    ext = extend_periodic(chk, obs, priors, h, j0, j1, cols, rounds)
    bc = extended_block_cols(cols, j0, j1, rounds)
    assert ext[0].shape == ((rounds + 1) * h, bc[-1]) and len(bc) == rounds + 2 and ext[1].shape == (3, bc[-1])
    if rounds == 5:
        assert same(ext[0], chk) and same(ext[1], obs) and np.array_equal(ext[2], priors) and np.array_equal(bc, cols)
    assert cols[j0] == 3 and cols[j0 + 1] - cols[j0] == 7 and (bc[1:-1] % 4 != 0).any()
    # the property everything rests on: column block b touches row blocks b and b + 1 only
    c = sp.csc_matrix(ext[0])
    for b in range(rounds + 1):
        idx = c.indices[c.indptr[bc[b]]:c.indptr[bc[b + 1]]]
        assert idx.min() == b * h and idx.max() == min(b + 2, rounds + 1) * h - 1  # (both halves of its rows are reached)
    shots, seed, first = 64, 99, 2 ** 32 + 5
    det, flips, faults = whole_ref(ext, shots, seed, first)
    assert 0.2 < faults.mean() < 0.4 and faults.any(axis=0).all() and det[:, ::h].any(axis=0).all() and flips.any()
    for kind in ("ones", "twos", "uneven"):
        got_flips = np.zeros(shots, np.uint32)
        for b0, n in chunked(rounds + 1, kind):
            rows, fl, fa = rows_ref(ext, bc, h, b0, n, shots, seed, first)
            assert np.array_equal(rows, det[:, b0 * h:(b0 + n) * h]), (kind, b0, n)
            assert np.array_equal(fa, faults[:, bc[b0]:bc[b0 + n]])
            got_flips ^= fl
        assert np.array_equal(got_flips, flips), kind
    with pytest.raises(ValueError, match="cannot lose more than its 3 body rounds"):
        extend_periodic(chk, obs, priors, h, j0, j1, cols, 1)
