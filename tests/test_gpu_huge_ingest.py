"""The CSR ingest of the general forms (csrc/swd_huge.hip, csrc/swd_huge_gdg.hip; the row check and the transpose are shared with
Graph::build, csrc/swd_graph.hip) on raw graph descriptions: the Python classes normalise a matrix before the library sees it, so
malformed and unsorted rows reach the library through ctypes only.  SWD_FORCE_HUGE=1 routes a 12 x 40 graph to the general forms."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, N, COLW = 12, 40, 3


def _graph():
    """a random 12 x 40 check matrix of column weight 3 as a sorted CSR, with priors"""
    rng = np.random.default_rng(41)
    H = np.zeros((M, N), np.uint8)
    for v in range(N):
        H[rng.choice(M, COLW, replace=False), v] = 1
    assert H.sum(axis=1).min() >= 3
    row_ptr = np.concatenate([[0], np.cumsum(H.sum(axis=1))]).astype(np.int32)
    col_idx = np.concatenate([np.flatnonzero(H[r]) for r in range(M)]).astype(np.int32)
    return H, row_ptr, col_idx, rng.uniform(0.03, 0.08, size=N)


def _osdw_params():
    from slidingwindowdecoder_amd import _lib
    return _lib.OsdwParams(3, 8, 1.0, 0, 2, 2)  # pre 3, post 8, osd_cs of order 2


def _gdg_params():
    from slidingwindowdecoder_amd import _lib
    return _lib.GdgParams(4, 1.0, 3, 12, 2, 6, 5, 5, 1.0, 0, 0, 0, 0)  # bpgdg_decoder, single thread, tree depth 2


def _create(which, row_ptr, col_idx, probs):
    """swd_osdw_create / swd_gdg_create on the raw arrays: (handle or None, message)"""
    from slidingwindowdecoder_amd import _lib
    L = _lib.lib()
    row_ptr, col_idx = np.ascontiguousarray(row_ptr, np.int32), np.ascontiguousarray(col_idx, np.int32)
    desc = _lib.GraphDesc(M, N, len(col_idx), row_ptr.ctypes.data, col_idx.ctypes.data, probs.ctypes.data)
    p = _osdw_params() if which == "osdw" else _gdg_params()
    h = (L.swd_osdw_create if which == "osdw" else L.swd_gdg_create)(C.byref(desc), C.byref(p), 0)
    return h, _lib.last_error()


def _decode(which, h, synd):
    from slidingwindowdecoder_amd import _lib
    L = _lib.lib()
    B = len(synd)
    out, st, pm = np.zeros((B, N), np.uint8), np.zeros((B, _lib.STAT_WORDS), np.int32), np.zeros(B, np.float64)
    if which == "osdw":
        rc = L.swd_osdw_decode_batch(h, B, synd.ctypes.data, out.ctypes.data, st.ctypes.data, pm.ctypes.data, None, 0, None, None)
    else:
        rc = L.swd_gdg_decode_batch(h, B, synd.ctypes.data, out.ctypes.data, st.ctypes.data, pm.ctypes.data, None, 0)
    assert rc == 0, _lib.last_error()
    return out, st, pm


def _destroy(which, h):
    from slidingwindowdecoder_amd import _lib
    (_lib.lib().swd_osdw_destroy if which == "osdw" else _lib.lib().swd_gdg_destroy)(h)


@pytest.mark.parametrize("which", ["osdw", "gdg"])
@pytest.mark.parametrize("defect,text", [("duplicate", "duplicate entry in row 4"), ("range", "column index out of range in row 4"),
                                         ("row_ptr", "row_ptr not monotone at row 4")])
def test_general_forms_refuse_malformed_rows(monkeypatch, which, defect, text):
    """one defect per description: a row with a duplicated column, a column index equal to n, a row_ptr that decreases once (its
    ends still span nnz) -- no handle, and the message names the defect and its row"""
    monkeypatch.setenv("SWD_FORCE_HUGE", "1")
    _, row_ptr, col_idx, probs = _graph()
    row_ptr, col_idx = row_ptr.copy(), col_idx.copy()
    if defect == "duplicate":
        col_idx[row_ptr[4] + 1] = col_idx[row_ptr[4]]
    elif defect == "range":
        col_idx[row_ptr[4] + 1] = N
    else:
        row_ptr[5] = row_ptr[4] - 1
    h, msg = _create(which, row_ptr, col_idx, probs)
    if h:
        _destroy(which, h)
    assert not h and text in msg, msg


@pytest.mark.parametrize("which", ["osdw", "gdg"])
def test_general_forms_take_unsorted_rows(monkeypatch, which):
    """the column indices shuffled inside each row: the ingest's sort makes that legal -- the decoder builds and decodes 16 syndromes
    to the vectors, statistics words and path metrics of the decoder built from the sorted CSR"""
    monkeypatch.setenv("SWD_FORCE_HUGE", "1")
    H, row_ptr, col_idx, probs = _graph()
    rng = np.random.default_rng(43)
    shuffled = col_idx.copy()
    for r in range(M):
        rng.shuffle(shuffled[row_ptr[r]:row_ptr[r + 1]])
    assert not np.array_equal(shuffled, col_idx)
    e = (rng.random((16, N)) < 0.08).astype(np.uint8)
    synd = np.ascontiguousarray((e @ H.T) % 2, dtype=np.uint8)
    res = []
    for ci in (col_idx, shuffled):
        h, msg = _create(which, row_ptr, ci, probs)
        assert h, msg
        res.append(_decode(which, h, synd))
        _destroy(which, h)
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    assert len(np.unique(res[0][1][:, 0] & 0xFF)) > 1  # (more than one exit class among the 16 shots)
