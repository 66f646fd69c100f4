"""(W, F) sliding-window geometry over a BB detector error model.

Counterpart of the window-extraction half of the reference's harness
(/root/reference/osd.py:42-121, identical code in guessing.py:49-126 and the notebooks):

1. columns are permuted into "regions" keyed by the first and last detector round they
   touch (osd.py:42-68);
2. ``anchors`` = (first detector row, first column) of every round block (osd.py:70-77);
3. window t spans rows of W consecutive blocks; for ``method=1`` every non-final window
   keeps the faults local to its last block and replaces the faults that reach into the
   next block by an h x h identity ("noisy syndrome") with the merged prior
   ``sum(chk[c0:b0, c1:b1] * priors[c1:b1])`` (osd.py:79-89, 103-113);
4. ``num_win = ceil((len(anchors) - W + F - 1) / F)`` (osd.py:91);
5. after decoding window t the first ``anchors[t+F].col - anchors[t].col`` entries of the
   estimate are committed (whole estimate for the last window) (osd.py:140, 170-173).

Everything here is host-side setup that runs once per experiment; matrices are kept
sparse (CSR) because the decoder consumes CSR edge lists.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp


@dataclass
class Window:
    row0: int          # a[0]
    row1: int          # b[0]
    col0: int          # a[1]   first global column of the window
    ncols_global: int  # how many leading window columns are global DEM columns
    commit: int        # number of leading columns committed after decoding
    mat: sp.csr_matrix  # (row1-row0) x n_window check matrix (incl. identity block)
    prior: np.ndarray   # n_window fault probabilities
    is_last: bool


@dataclass
class WindowPlan:
    chk: sp.csr_matrix      # region-permuted global check matrix
    obs: sp.csr_matrix
    priors: np.ndarray
    perm: np.ndarray        # new column j = old column perm[j]
    anchors: list
    windows: list
    noisy_prior: float | None
    n_half: int


def region_permutation(chk: sp.spmatrix, n_half: int) -> np.ndarray:
    """Column order of osd.py:42-68: regions enumerated as (i, i+h), (i, i+2h) for
    i = 0, h, 2h, ...; inside a region the original order is kept."""
    chk = sp.csc_matrix(chk)
    num_row, num_col = chk.shape
    n = 2 * n_half
    bounds = []
    i = 0
    while i < num_row:
        bounds.append((i, i + n_half))
        if i + n > num_row:
            break
        bounds.append((i, i + n))
        i += n_half
    region_of = {lu: k for k, lu in enumerate(bounds)}
    keys = np.empty(num_col, dtype=np.int64)
    for j in range(num_col):
        r = chk.indices[chk.indptr[j]:chk.indptr[j + 1]]
        lo = int(r.min()) // n_half * n_half
        hi = (int(r.max()) // n_half + 1) * n_half
        keys[j] = region_of[(lo, hi)]
    return np.argsort(keys, kind="stable")


def find_anchors(chk: sp.spmatrix, n_half: int) -> list:
    """osd.py:70-77."""
    chk = sp.csc_matrix(chk)
    num_row, num_col = chk.shape
    anchors = []
    j = 0
    for i in range(num_col):
        r = chk.indices[chk.indptr[i]:chk.indptr[i + 1]]
        if r.min() >= j:
            anchors.append((j, i))
            j += n_half
    anchors.append((num_row, num_col))
    return anchors


def plan_windows(chk, obs, priors, n_half: int, W: int, F: int, method: int = 1,
                 z_basis: bool = True, noisy_prior=None) -> WindowPlan:
    perm = region_permutation(chk, n_half)
    chk = sp.csc_matrix(chk)[:, perm]
    obs = sp.csc_matrix(obs)[:, perm]
    priors = np.asarray(priors, dtype=np.float64)[perm]
    anchors = find_anchors(chk, n_half)
    n = 2 * n_half
    chk_r = sp.csr_matrix(chk)

    def shifted(c):
        if method == 1:
            return (c[0], c[1] + (n_half * 3 if z_basis else n))
        return c

    # osd.py:79-89: one merged prior PER ROW of the identity block (np.sum(..., axis=1)); the rows agree for
    # the BB circuits (the reference prints element 0) but not e.g. for SHYPS.  A caller-given scalar is broadcast.
    noisy_vec = None
    if noisy_prior is None and method != 0:
        b = anchors[W]
        c = shifted(anchors[W - 1])
        block = chk_r[c[0]:b[0], c[1]:b[1]]
        noisy_vec = np.asarray(block.multiply(priors[c[1]:b[1]]).sum(axis=1)).ravel()
        noisy_prior = float(noisy_vec[0])
    elif method != 0:
        noisy_vec = np.ones(n_half) * np.asarray(noisy_prior, dtype=np.float64)
        noisy_prior = float(noisy_vec[0])

    num_win = math.ceil((len(anchors) - W + F - 1) / F)
    windows = []
    top_left = 0
    for i in range(num_win):
        a = anchors[top_left]
        b = anchors[min(top_left + W, len(anchors) - 1)]
        last = i == num_win - 1
        if not last and method != 0:
            c = shifted(anchors[top_left + W - 1])
            sub = chk_r[a[0]:b[0], a[1]:c[1]]
            nrow = b[0] - a[0]
            ident = sp.csr_matrix((np.ones(n_half, np.uint8),
                                   (np.arange(nrow - n_half, nrow), np.arange(n_half))),
                                  shape=(nrow, n_half))
            mat = sp.hstack((sub, ident), format="csr")
            prior = np.concatenate((priors[a[1]:c[1]], noisy_vec))
            ncg = c[1] - a[1]
        else:
            mat = sp.csr_matrix(chk_r[a[0]:b[0], a[1]:b[1]])
            prior = priors[a[1]:b[1]].copy()
            ncg = b[1] - a[1]
        commit = ncg if last else anchors[top_left + F][1] - a[1]
        mat.sort_indices()
        windows.append(Window(a[0], b[0], a[1], ncg, commit, mat, prior, last))
        top_left += F
    return WindowPlan(sp.csr_matrix(chk), sp.csr_matrix(obs), priors, perm, anchors, windows,
                      noisy_prior, n_half)


def sample_dem(chk, obs, priors, num_shots: int, seed: int = 20240318):
    """Bernoulli(priors) fault sampling -> (det_data, obs_data, faults); what
    ``dem.compile_sampler().sample`` provides to the reference harness (osd.py:124-125)."""
    rng = np.random.default_rng(seed)
    chk = sp.csr_matrix(chk)
    obs = sp.csr_matrix(obs)
    e = (rng.random((num_shots, chk.shape[1])) < priors).astype(np.uint8)
    det = (sp.csr_matrix(e) @ chk.T.astype(np.int32)).toarray() % 2
    ob = (sp.csr_matrix(e) @ obs.T.astype(np.int32)).toarray() % 2
    return det.astype(np.uint8), ob.astype(np.uint8), e


def sliding_window_decode_host(plan: WindowPlan, det_data: np.ndarray, decoder_factory,
                               on_decode=None):
    """Host-side window loop with the commit rule of osd.py:130-179.

    ``decoder_factory(window) -> object with .decode(syndrome)``; any decoder with the
    reference's class surface fits (the product's classes, the oracle, or the reference
    itself).  Returns (total_e_hat[shots, num_col] uint8, flagged_per_window).
    ``on_decode(win_idx, shot, decoder, syndrome, e_hat)`` is an optional tap used by the
    fixture generator and the parity tests.
    """
    num_shots = det_data.shape[0]
    num_col = plan.chk.shape[1]
    chk_t = sp.csr_matrix(plan.chk.T.astype(np.int32))
    total = np.zeros((num_shots, num_col), dtype=np.uint8)
    cur = det_data.copy()
    flagged = []
    for wi, w in enumerate(plan.windows):
        dec = decoder_factory(w)
        nflag = 0
        mat_i = w.mat.astype(np.int32)
        for j in range(num_shots):
            s = cur[j, w.row0:w.row1]
            e_hat = np.asarray(dec.decode(s))
            if on_decode is not None:
                on_decode(wi, j, dec, s, e_hat)
            nflag += int(((mat_i @ e_hat + s) % 2).any())
            total[j, w.col0:w.col0 + w.commit] = e_hat[:w.commit]
        flagged.append(nflag)
        cur = ((det_data + (sp.csr_matrix(total) @ chk_t).toarray()) % 2).astype(np.uint8)
    return total, flagged


def sliding_window_decode_online_host(plan: WindowPlan, chunks, decoder_factory):
    """The same loop driven by the ARRIVAL of detector rows -- the executable specification of the online sessions
    (``SlidingWindowDecoder.session``).  ``chunks``: arrays [shots, k] (k >= 0), the detector rows in row order.  The residual
    syndrome starts as zero; arriving rows are XORed into it; window t is decoded once ``rows received >= row1`` and window
    t - 1 has committed; every committed fault XORs its column of ``chk`` into the residual syndrome, rows that have not
    arrived yet included.  The loop of osd.py:130-179 is causal (window t reads rows < row1 of det ^ chk @ total_e_hat), so the
    result is that of ``sliding_window_decode_host`` whatever the chunking.
    Returns (total_e_hat, events, resid): ``events`` = per chunk the list of ``(t, col0, faults[shots, commit])`` it committed;
    ``resid`` = det ^ chk @ total_e_hat (flagged = ``resid.any(axis=1)``, osd.py:184-187)."""
    chk_c = sp.csc_matrix(plan.chk)
    num_det, num_col = chk_c.shape
    decs = {}
    total = resid = None
    rows, nxt, events = 0, 0, []
    for ch in chunks:
        ch = np.asarray(ch, dtype=np.uint8)
        if total is None:
            total = np.zeros((ch.shape[0], num_col), np.uint8)
            resid = np.zeros((ch.shape[0], num_det), np.uint8)
        if nxt == len(plan.windows) or rows + ch.shape[1] > num_det:
            raise ValueError("rows pushed after the last window / beyond the experiment")
        resid[:, rows:rows + ch.shape[1]] ^= ch & 1
        rows += ch.shape[1]
        ready = []
        while nxt < len(plan.windows) and rows >= plan.windows[nxt].row1:
            w = plan.windows[nxt]
            dec = decs.setdefault(nxt, decoder_factory(w))
            for j in range(total.shape[0]):
                e_hat = np.asarray(dec.decode(resid[j, w.row0:w.row1].copy()))[:w.commit].astype(np.uint8)
                total[j, w.col0:w.col0 + w.commit] = e_hat
                for c in np.flatnonzero(e_hat):
                    resid[j, chk_c.indices[chk_c.indptr[w.col0 + c]:chk_c.indptr[w.col0 + c + 1]]] ^= 1
            ready.append((nxt, w.col0, total[:, w.col0:w.col0 + w.commit].copy()))
            nxt += 1
        events.append(ready)
    return total, events, resid


def logical_error_stats(plan: WindowPlan, det_data, obs_data, total_e_hat):
    """osd.py:184-191: flagged = residual syndrome non-zero; logical = any observable wrong."""
    t = sp.csr_matrix(total_e_hat)
    resid = (det_data + (t @ plan.chk.T.astype(np.int32)).toarray()) % 2
    flagged = resid.any(axis=1)
    logical = ((obs_data + (t @ plan.obs.T.astype(np.int32)).toarray()) % 2).any(axis=1)
    return flagged, np.logical_or(flagged, logical)


def memory_experiment_host(plan: WindowPlan, det_data, obs_data, decoder_factory):
    """The whole of the reference's ``sliding_window_decoder`` after sampling (osd.py:130-191) on the host -- the executable
    specification of ``MemoryExperiment``: ``sliding_window_decode_host``, then ``logical_error_stats``.  ``obs_data`` [shots,
    num_obs]: the true observable flips.  Returns a dict: the counters ``shots``, ``logical_errors`` (flagged or a wrong
    observable), ``flagged``, ``observable_mismatches``; ``result`` [shots], the per-shot words of include/swd.h (bit 0 logical
    error, bit 1 flagged, bit 2 observable mismatch); ``total_e_hat``; and, when the factory's decoders expose ``exit_class``,
    ``converge`` and ``bp_iteration``, the per-window counts ``window_exit_classes`` [W, 8], ``window_not_converged`` [W] and
    ``window_bp_iterations`` [W] (None otherwise)."""
    det_data, obs_data = np.asarray(det_data, dtype=np.uint8), np.asarray(obs_data, dtype=np.uint8)
    W = len(plan.windows)
    cls, ncv, its = np.zeros((W, 8), np.int64), np.zeros(W, np.int64), np.zeros(W, np.int64)
    seen = []

    def tap(wi, j, dec, s, e_hat):
        if all(hasattr(dec, a) for a in ("exit_class", "converge", "bp_iteration")):
            cls[wi, int(dec.exit_class) & 7] += 1
            ncv[wi] += 0 if dec.converge else 1
            its[wi] += int(dec.bp_iteration)
            seen.append(wi)

    total, _ = sliding_window_decode_host(plan, det_data, decoder_factory, on_decode=tap)
    flagged, logical = logical_error_stats(plan, det_data, obs_data, total)
    wrong = ((obs_data + (sp.csr_matrix(total) @ plan.obs.T.astype(np.int32)).toarray()) % 2).any(axis=1)
    assert np.array_equal(logical, flagged | wrong)
    have = len(seen) == W * det_data.shape[0] and W > 0
    return dict(shots=int(det_data.shape[0]), logical_errors=int(logical.sum()), flagged=int(flagged.sum()),
                observable_mismatches=int(wrong.sum()),
                result=(logical.astype(np.int32) | (flagged.astype(np.int32) << 1) | (wrong.astype(np.int32) << 2)),
                total_e_hat=total, window_exit_classes=cls if have else None, window_not_converged=ncv if have else None,
                window_bp_iterations=its if have else None)


def distinct_windows(plan: WindowPlan) -> list:
    """For every window the index of the FIRST window with the same matrix and the same priors (bit for bit): the decoders a window
    loop needs to build (``SlidingWindowDecoder(window_loop="device")`` builds one per distinct window; a BB plan of 4 windows has 3).
    ``len(set(distinct_windows(plan)))`` is their number."""
    seen, first = {}, []
    for t, w in enumerate(plan.windows):
        a = sp.csr_matrix(w.mat, copy=True)
        a.eliminate_zeros()
        a.sort_indices()
        key = (a.shape, a.indptr.astype(np.int64).tobytes(), a.indices.astype(np.int64).tobytes(),
               np.ascontiguousarray(w.prior, np.float64).tobytes())
        first.append(seen.setdefault(key, t))
    return first


def commit_row_spans(plan: WindowPlan) -> list:
    """Per window ``(lo, hi)``: the detector rows ``[lo, hi)`` of ``plan.chk`` that its committed columns ``[col0, col0 + commit)``
    reach -- what a commit has to fold into the residual syndrome (osd.py:170-178); ``(0, 0)`` when they reach none.  On the BB plans
    the span lies inside the window's own rows."""
    c = sp.csc_matrix(plan.chk)
    c.eliminate_zeros()
    spans = []
    for w in plan.windows:
        rows = c.indices[c.indptr[w.col0]:c.indptr[w.col0 + w.commit]]
        spans.append((int(rows.min()), int(rows.max()) + 1) if rows.size else (0, 0))
    return spans


@dataclass
class RollingTemplate:
    """What a rolling session keeps of a template ``WindowPlan`` of R0 rounds (``rolling_template``): the head, body and tail
    windows, the strides between body windows and the committed columns of ``chk`` / ``obs`` in FRAME rows (row 0 = first row of
    the window that is decoded next).  It serves every experiment of ``R = R0 (mod F)`` rounds with ``R >= min_rounds``."""
    plan: WindowPlan
    head: Window
    body: Window
    tail: Window
    n_half: int
    W: int               # row blocks per window
    F: int               # row blocks the frame moves per window
    R0: int              # syndrome rounds of the template (its detector rows: (R0 + 1) * n_half)
    min_rounds: int      # the shortest experiment with a head and a tail window
    row_stride: int      # F * n_half
    col_stride: int
    frame_rows: int      # rows of residual syndrome kept per shot
    head_chk: sp.csc_matrix   # frame_rows x commit, per kind of window
    body_chk: sp.csc_matrix
    tail_chk: sp.csc_matrix
    head_obs: sp.csc_matrix   # num_obs x commit
    body_obs: sp.csc_matrix
    tail_obs: sp.csc_matrix

    def serves(self, rounds: int) -> bool:
        return rounds >= self.min_rounds and (rounds - self.R0) % self.F == 0

    def lengths(self) -> str:
        return (f"R = {self.R0} (mod {self.F}) syndrome rounds, R >= {self.min_rounds}: {self.min_rounds}, "
                f"{self.min_rounds + self.F}, {self.min_rounds + 2 * self.F}, ... (plus the final block of {self.n_half} rows)")


def _same_matrix(a, b):
    a, b = sp.csr_matrix(a), sp.csr_matrix(b)
    a.sort_indices()
    b.sort_indices()
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and \
        np.array_equal(a.data != 0, b.data != 0)


def rolling_template(plan: WindowPlan) -> RollingTemplate:
    """Checks that ``plan`` is periodic between its first and its last window -- every body window a translate of window 1,
    ``chk``, ``obs`` and ``priors`` periodic over the body column blocks -- and extracts head (window 0), body (window 1) and tail
    (last window) for a rolling session.  Raises ValueError naming what is not periodic."""
    wins = plan.windows
    h = int(plan.n_half)
    if len(wins) < 3:
        raise ValueError(f"a rolling template needs a first, a body and a last window; this plan has {len(wins)} windows (build it "
                         f"for more rounds)")
    head, body, tail = wins[0], wins[1], wins[-1]
    if not tail.is_last or any(w.is_last for w in wins[:-1]):
        raise ValueError("the last window of the plan, and only the last, must be marked is_last")
    num_det, num_col = plan.chk.shape
    if num_det % h or any(w.row0 % h or (w.row1 - w.row0) % h for w in wins):
        raise ValueError(f"detector rows and window rows must come in blocks of n_half = {h}")
    row_stride, col_stride = wins[2].row0 - body.row0, wins[2].col0 - body.col0
    W, F = (head.row1 - head.row0) // h, row_stride // h
    if row_stride <= 0 or col_stride <= 0 or head.row0 != 0 or head.col0 != 0 or body.row0 != row_stride:
        raise ValueError(f"windows do not advance by a constant positive stride from row 0 (rows {[w.row0 for w in wins]})")
    if body.row1 - body.row0 != W * h:
        raise ValueError("the first window and window 1 differ in their number of rows")
    for k in range(2, len(wins)):
        w, last = wins[k], k == len(wins) - 1
        if w.row0 - wins[k - 1].row0 != row_stride or w.col0 - wins[k - 1].col0 != col_stride:
            raise ValueError(f"window {k} is not placed one stride ({row_stride} rows, {col_stride} columns) after window {k - 1}")
        if last:
            break
        if w.commit != body.commit or w.ncols_global != body.ncols_global:
            raise ValueError(f"window {k} commits {w.commit} of {w.ncols_global} columns, window 1 commits {body.commit} of {body.ncols_global}")
        if not _same_matrix(w.mat, body.mat):
            raise ValueError(f"the matrix of window {k} is not periodic: it differs from that of window 1")
        if not np.array_equal(np.asarray(w.prior), np.asarray(body.prior)):
            j = np.flatnonzero(np.asarray(w.prior) != np.asarray(body.prior))
            raise ValueError(f"the priors of window {k} are not periodic: {len(j)} differ from those of window 1, the first at its column {int(j[0])}")
    if body.commit != col_stride:
        raise ValueError(f"body windows commit {body.commit} columns and advance by {col_stride}")
    if head.col0 + head.commit != body.col0:
        raise ValueError("the first window does not commit up to the first column of window 1")
    if tail.col0 + tail.commit != num_col or tail.row1 != num_det:
        raise ValueError("the last window does not close the experiment (rows and columns up to the end)")
    # chk, obs and priors over the body column blocks: the per-round blocks of plan.anchors that the body windows commit.  At least
    # two of them, or nothing shows that they are translates of one another: two body windows, or one that commits F >= 2 rounds
    anchors = [tuple(int(x) for x in a) for a in plan.anchors]
    col_at = {a[1]: i for i, a in enumerate(anchors)}
    if body.col0 not in col_at or tail.col0 not in col_at:
        raise ValueError("window columns do not start at the plan's anchors")
    j0, j1 = col_at[body.col0], col_at[tail.col0]
    if j1 - j0 < 2:
        raise ValueError(f"a rolling template needs at least two body windows (or one that commits two rounds or more) for its "
                         f"periodicity to be checked; this plan has {len(wins) - 2} body window(s) committing {j1 - j0} round(s): build it "
                         f"for more rounds")
    chk_c, obs_c, priors = sp.csc_matrix(plan.chk), sp.csc_matrix(plan.obs), np.asarray(plan.priors)
    chk_c.sort_indices()
    obs_c.sort_indices()

    def block(m, j, shift):
        c = m[:, anchors[j][1]:anchors[j + 1][1]]
        return c.indptr, c.indices - shift * (j - j0), c.data != 0

    for j in range(j0 + 1, j1):
        if anchors[j][0] - anchors[j - 1][0] != h:
            raise ValueError(f"anchors are not periodic: round {j} starts {anchors[j][0] - anchors[j - 1][0]} rows after round {j - 1}")
        for name, m, shift in (("chk", chk_c, h), ("obs", obs_c, 0)):
            a, b = block(m, j0, shift), block(m, j, shift)
            if not (len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a, b))):
                raise ValueError(f"{name} is not periodic: the columns of round {j} are no translate of those of round {j0}")
        pa, pb = priors[anchors[j0][1]:anchors[j0 + 1][1]], priors[anchors[j][1]:anchors[j + 1][1]]
        if not np.array_equal(pa, pb):
            d = np.flatnonzero(pa != pb)
            raise ValueError(f"priors are not periodic: {len(d)} of the columns of round {j} differ from those of round {j0}, the first "
                             f"at global column {int(anchors[j][1] + d[0])}")
    # committed columns in frame rows; the frame covers every row a window reads or a committed column can touch
    frame_rows, parts = 0, {}
    for name, w in (("head", head), ("body", body), ("tail", tail)):
        cols = chk_c[:, w.col0:w.col0 + w.commit]
        if cols.nnz and cols.indices.min() < w.row0:
            raise ValueError(f"the {name} window commits columns that touch rows before its first row: they would have left the frame")
        frame_rows = max(frame_rows, w.row1 - w.row0, int(cols.indices.max()) + 1 - w.row0 if cols.nnz else 0)
        parts[name] = (cols, obs_c[:, w.col0:w.col0 + w.commit], w.row0)
    if frame_rows > num_det:
        raise ValueError("the committed columns do not fit the frame")

    def in_frame(cols, row0):
        c = sp.csc_matrix((np.ones(cols.nnz, np.uint8), cols.indices - row0, cols.indptr), shape=(frame_rows, cols.shape[1]))
        return c

    R0 = num_det // h - 1
    n0 = len(wins) - 1                                   # non-last windows of the template: ceil((R0 + 1 - W) / F)
    min_rounds = R0 - (n0 - 1) * F                       # the same residue with one non-last window (the head)
    return RollingTemplate(plan, head, body, tail, h, W, F, R0, min_rounds, row_stride, col_stride, frame_rows,
                           *[in_frame(parts[k][0], parts[k][2]) for k in ("head", "body", "tail")],
                           *[sp.csc_matrix(parts[k][1]) for k in ("head", "body", "tail")])


def sliding_window_decode_rolling_host(template_plan, chunks, final_rows, decoder_factory):
    """The window loop on a FRAME of residual rows -- the executable specification of the rolling sessions
    (``SlidingWindowDecoder.rolling_session``).  ``template_plan``: a ``WindowPlan`` (or its ``RollingTemplate``) of R0 rounds;
    ``chunks``: arrays [shots, k] (k >= 0), the rows of the SYNDROME rounds in row order, as many rounds as the experiment has;
    ``final_rows`` [shots, k]: the rest, which must hold the final data-measurement block (a piece of it would do, as long as
    it is not empty: ``chunks`` are taken for syndrome rounds, a whole block among them completes a window).
    Per shot: a frame of ``frame_rows`` residual rows, row 0 = first row of the next window.  Arriving rows are XORed in; when
    the frame holds the next window's rows it is decoded (head, then bodies), its first ``commit`` columns are committed and
    their ``chk`` columns folded into the frame; the ``F * n_half`` rows that scroll out are ORed into the sticky ``flagged`` bit
    (committed columns of window t only touch row blocks >= t, arrivals come later still), and the frame moves on.  ``final_rows``
    closes the experiment: the tail window is decoded and committed whole.  The result is that of ``sliding_window_decode_host``
    on ``plan_windows`` of the experiment's own length R, for every ``R = R0 (mod F)``.
    Returns (events, obs_flips [shots, num_obs], flagged [shots]); ``events`` = ``(t, faults [shots, commit_t])`` per window."""
    T = template_plan if isinstance(template_plan, RollingTemplate) else rolling_template(template_plan)
    final_rows = np.asarray(final_rows, dtype=np.uint8)
    B = final_rows.shape[0]
    frame = np.zeros((B, T.frame_rows), np.uint8)
    flagged = np.zeros(B, bool)
    obs_flips = np.zeros((B, T.head_obs.shape[0]), np.uint8)
    decs, events = {}, []
    fill, t, received = 0, 0, 0
    need = T.head.row1 - T.head.row0

    def step(kind, w, chk_f, obs_f, shift):
        dec = decs.setdefault(kind, decoder_factory(w))
        faults = np.zeros((B, w.commit), np.uint8)
        for j in range(B):
            e_hat = np.asarray(dec.decode(frame[j, :w.row1 - w.row0].copy()))[:w.commit].astype(np.uint8)
            faults[j] = e_hat
            for c in np.flatnonzero(e_hat):
                frame[j, chk_f.indices[chk_f.indptr[c]:chk_f.indptr[c + 1]]] ^= 1
                obs_flips[j, obs_f.indices[obs_f.indptr[c]:obs_f.indptr[c + 1]]] ^= 1
        events.append((t, faults))
        flagged[:] |= frame[:, :shift].any(axis=1)
        frame[:, :T.frame_rows - shift] = frame[:, shift:].copy()
        frame[:, T.frame_rows - shift:] = 0

    for ch in chunks:
        ch = np.asarray(ch, dtype=np.uint8)
        r = 0
        while r < ch.shape[1]:
            k = min(ch.shape[1] - r, T.frame_rows - fill)
            frame[:, fill:fill + k] ^= ch[:, r:r + k] & 1
            fill, r, received = fill + k, r + k, received + k
            while fill >= need:
                step("head" if t == 0 else "body", T.head if t == 0 else T.body, T.head_chk if t == 0 else T.body_chk,
                     T.head_obs if t == 0 else T.body_obs, T.row_stride)
                fill, t = fill - T.row_stride, t + 1
    k = final_rows.shape[1]
    tail_rows = T.tail.row1 - T.tail.row0
    total = received + k
    if t == 0 or k == 0 or fill + k != tail_rows:
        rounds = f"{total // T.n_half - 1} syndrome rounds" if total % T.n_half == 0 else "no whole number of rounds"
        raise ValueError(f"{total} detector rows ({received} pushed, {k} final) make {rounds}; this template serves {T.lengths()}"
                         + ("; the final block must go to the closing call, not to a push" if k == 0 else ""))
    frame[:, fill:fill + k] ^= final_rows & 1
    step("tail", T.tail, T.tail_chk, T.tail_obs, T.frame_rows)
    return events, obs_flips, flagged


def _as_template(template_or_plan) -> RollingTemplate:
    return template_or_plan if isinstance(template_or_plan, RollingTemplate) else rolling_template(template_or_plan)


def template_blocks(template_or_plan):
    """``(j0, j1, anchor_cols)`` of a rolling template: the column blocks (one per round, ``plan.anchors``) ``j0 .. j1 - 1`` are the body
    rounds, the translates of one another that an experiment of another length repeats; ``anchor_cols`` [R0 + 2]: the first column of
    every block and the number of columns.  What ``extend_periodic`` and the rolling DEM sampler take."""
    T = _as_template(template_or_plan)
    cols = [int(a[1]) for a in T.plan.anchors]
    return cols.index(int(T.body.col0)), cols.index(int(T.tail.col0)), np.asarray(cols, dtype=np.int64)


def extend_periodic(chk, obs, priors, n_half: int, j0: int, j1: int, anchor_cols, rounds: int):
    """The model of ``rounds`` rounds that a periodic model of R0 rounds stands for: the head columns ``[0, c0)`` as they are, the
    body block ``[c0, c1)`` -- column block ``j0`` -- ``(j1 - j0) + (rounds - R0)`` times, copy k with its rows moved down by
    ``k * n_half`` (observables and priors as they are), then the tail columns ``[c2, end)`` with their rows moved down by
    ``(rounds - R0) * n_half``.  -> (chk, obs, priors) as scipy CSC matrices and a numpy vector."""
    chk, priors = sp.csc_matrix(chk), np.asarray(priors, dtype=np.float64)
    obs = sp.csc_matrix(obs) if obs is not None else sp.csc_matrix((0, chk.shape[1]), dtype=np.uint8)
    a = [int(x) for x in anchor_cols]
    h, R0 = int(n_half), len(a) - 2
    nbody = (j1 - j0) + (int(rounds) - R0)
    if not 0 <= j0 < j1 <= R0 or chk.shape[0] != (R0 + 1) * h or a[-1] != chk.shape[1]:
        raise ValueError("anchor columns, body blocks and matrix shape do not describe a model of whole rounds")
    if nbody < 0:
        raise ValueError(f"{rounds} rounds: the model of {R0} rounds cannot lose more than its {j1 - j0} body rounds")
    c0, c1, c2 = a[j0], a[j0 + 1], a[j1]
    num_det = (int(rounds) + 1) * h

    def moved(m, lo, hi, shift):
        c = sp.csc_matrix(m[:, lo:hi])
        c.sort_indices()
        return sp.csc_matrix((np.ones(c.nnz, np.uint8), c.indices + shift, c.indptr), shape=(num_det, hi - lo))

    parts = [moved(chk, 0, c0, 0)] + [moved(chk, c0, c1, k * h) for k in range(nbody)] + [moved(chk, c2, a[-1], (int(rounds) - R0) * h)]
    oparts = [obs[:, :c0]] + [obs[:, c0:c1]] * nbody + [obs[:, c2:]]
    pparts = [priors[:c0]] + [priors[c0:c1]] * nbody + [priors[c2:]]
    return sp.hstack(parts, format="csc"), sp.hstack(oparts, format="csc"), np.concatenate(pparts)


def extended_block_cols(anchor_cols, j0: int, j1: int, rounds: int) -> np.ndarray:
    """[rounds + 2]: the first column of every column block of ``extend_periodic``'s model of ``rounds`` rounds, and its number of
    columns.  Block b holds the faults that first show in row block b; they reach into row block b + 1 at most."""
    a = np.asarray(anchor_cols, dtype=np.int64)
    R0 = len(a) - 2
    nbody, cs = (j1 - j0) + (int(rounds) - R0), int(a[j0 + 1] - a[j0])
    if nbody < 0:
        raise ValueError(f"{rounds} rounds: the model of {R0} rounds cannot lose more than its {j1 - j0} body rounds")
    return np.concatenate([a[:j0], a[j0] + cs * np.arange(nbody, dtype=np.int64), a[j1:] + cs * (int(rounds) - R0)])


def extend_template(template_or_plan, rounds: int):
    """The region-permuted ``chk``, ``obs`` and ``priors`` of ``plan_windows`` of the SAME circuit with ``rounds`` syndrome rounds,
    built from the template of R0 rounds alone (``extend_periodic`` on its blocks): equal to them for every ``rounds >=
    min_rounds``, whatever its residue mod F.  Together with the Philox restatement of the sampler's stream this is the executable
    specification of ``RollingDemSampler``.  ValueError below ``min_rounds``."""
    T = _as_template(template_or_plan)
    if int(rounds) < T.min_rounds:
        raise ValueError(f"{rounds} rounds are fewer than the template's shortest experiment; this template serves {T.lengths()}")
    j0, j1, cols = template_blocks(T)
    return extend_periodic(T.plan.chk, T.plan.obs, T.plan.priors, T.n_half, j0, j1, cols, rounds)


def rolling_schedule(template_or_plan, rounds: int):
    """``[(block0, nblocks), ...]``: the row blocks (of ``n_half`` detector rows) in the order a rolling experiment of ``rounds``
    rounds hands them to its session -- the head window's W blocks, then F blocks per body window (each entry but the last
    completes one window), and last what ``finish`` takes: the rest, the final block included.  ValueError naming the lengths
    served when the template does not serve ``rounds``."""
    T = _as_template(template_or_plan)
    if not T.serves(int(rounds)):
        raise ValueError(f"{rounds} syndrome rounds: this template serves {T.lengths()}")
    blocks, tail = int(rounds) + 1, (T.tail.row1 - T.tail.row0) // T.n_half
    # the tail window starts where the last head / body window's frame ends up: F blocks of it are new
    out, b = [(0, T.W)], T.W
    while blocks - b > tail - (T.W - T.F):
        out.append((b, T.F))
        b += T.F
    out.append((b, blocks - b))
    return out
