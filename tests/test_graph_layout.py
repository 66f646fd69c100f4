"""Message-slot layout of a window graph (csrc/swd_graph.hip: Graph::build, Graph::optimize_layout) through the host-only entry point
``swd_graph_layout``: no GPU needed.  The layout may permute a check's edges over its positions, trade the lanes of checks of one
degree and put pad cells between diagonals; every table must still describe the CSR input, and the natural layout -- restated here in
numpy, never taken from the library -- must come back byte for byte when SWD_NATURAL_LAYOUT is set.

Inputs: a mid window of the [[72,12,6]] (3,1) plan; a ragged matrix with rows of degree 1, tied degrees and a row of degree 40
(K > 32); a matrix of 64 checks of degree 6, whose diagonals all start on bank 0 (jptr[j] = 64 j), as the headline window's collapse
onto four banks."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from slidingwindowdecoder_amd import _lib

PAD_EDGE = 0xFFFFFFFF


def ragged_matrix():
    """48 x 160: four checks of degree 1, one of degree 40 and one of 36, the rest of degree 3, 5 or 7 (ties); every column used"""
    rng = np.random.default_rng(20240611)
    m, n = 48, 160
    deg = np.array([1, 1, 1, 1, 40, 36] + [int(d) for d in rng.choice([3, 5, 5, 7], size=m - 6)])
    rng.shuffle(deg)
    H = np.zeros((m, n), np.uint8)
    for r in range(m):
        H[r, rng.choice(n, size=deg[r], replace=False)] = 1
    for v in np.flatnonzero(H.sum(axis=0) == 0):  # an unused column joins a check of degree >= 3 (its degree stays tied with others or not: both occur)
        H[rng.choice(np.flatnonzero(deg >= 3)), v] = 1
    assert H.sum(axis=0).max() <= 8 and H.sum(axis=1).max() >= 40 and (H.sum(axis=1) == 1).sum() == 4
    return sp.csr_matrix(H)


def collapsed_matrix():
    """64 x 128, every check of degree 6: jptr[j] = 64 j, so in the natural layout every position of every check starts on bank 0"""
    m, n = 64, 128
    H = np.zeros((m, n), np.uint8)
    for r in range(m):
        H[r, (2 * r + np.array([0, 1, 5, 17, 40, 77])) % n] = 1
    return sp.csr_matrix(H)


@functools.lru_cache(maxsize=None)
def bb72_window():
    from tests.test_rolling_host import template_plan
    return sp.csr_matrix(template_plan("w3f1m1").windows[1].mat)


CASES = {"bb72_w3f1": bb72_window, "ragged": ragged_matrix, "collapsed": collapsed_matrix}


def layout(H, pads):
    """the library's tables for H with up to `pads` pad cells (SWD_NATURAL_LAYOUT is read by the call)"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libswd_hip.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    H = sp.csr_matrix(H)
    H.sort_indices()
    m, n = H.shape
    rp, ci = H.indptr.astype(np.int32), H.indices.astype(np.int32)
    pr = np.full(n, 0.01)
    desc = _lib.GraphDesc(m, n, int(H.nnz), rp.ctypes.data, ci.ctypes.data, pr.ctypes.data)
    info = np.zeros(8, np.int32)
    assert L.swd_graph_layout(C.byref(desc), pads, info.ctypes.data, *([None] * 8)) == 0, _lib.last_error()
    S, K, D = (int(x) for x in info[:3])
    t = dict(jptr=np.zeros(K + 1, np.uint16), row_col=np.zeros(S, np.uint16), perm=np.zeros(m, np.uint16), iperm=np.zeros(m, np.uint16),
             row_deg=np.zeros(m, np.uint8), vn_edge=np.zeros(D * n, np.uint32), vn_edge_s=np.zeros(D * n, np.uint32), vperm=np.zeros(n, np.uint16))
    info2 = np.zeros(8, np.int32)
    assert L.swd_graph_layout(C.byref(desc), pads, info2.ctypes.data, *[a.ctypes.data for a in t.values()]) == 0
    assert np.array_equal(info, info2)
    t.update(S=S, K=K, D=D, cost=int(info[3]) + int(info[4]), cost_natural=int(info[5]) + int(info[6]), pads=int(info[7]),
             loads=(int(info[3]), int(info[5])), stores=(int(info[4]), int(info[6])))
    return t


def natural_tables(H):
    """today's layout, restated: lanes by decreasing degree (stable in the check), positions in ascending column order, no pads"""
    H = sp.csr_matrix(H)
    H.sort_indices()
    m, n = H.shape
    rp, ci = H.indptr, H.indices
    deg = np.diff(rp)
    K, cdeg = int(deg.max()), np.bincount(ci, minlength=n)
    D = int(cdeg.max())
    perm = np.argsort(-deg, kind="stable")
    iperm = np.empty(m, np.int64)
    iperm[perm] = np.arange(m)
    jptr = np.concatenate([[0], np.cumsum([(deg > j).sum() for j in range(K)])])
    row_col = np.zeros(H.nnz, np.uint16)
    vn_edge = np.full(D * n, PAD_EDGE, np.uint32)
    fill = np.zeros(n, np.int64)
    for r in range(m):
        for e in range(rp[r], rp[r + 1]):
            j, v, l = e - rp[r], ci[e], iperm[r]
            slot = jptr[j] + l
            row_col[slot] = v
            vn_edge[fill[v] * n + v] = slot | (l << 16) | (j << 26)
            fill[v] += 1
    vperm = np.argsort(-((cdeg + 1) // 2), kind="stable")
    vn_edge_s = vn_edge.reshape(D, n)[:, vperm].reshape(-1)
    return dict(jptr=jptr.astype(np.uint16), row_col=row_col, perm=perm.astype(np.uint16), iperm=iperm.astype(np.uint16),
                row_deg=deg[perm].astype(np.uint8), vn_edge=vn_edge, vn_edge_s=vn_edge_s, vperm=vperm.astype(np.uint16))


def model_cost(t, n):
    """the cost model, restated: loads in aligned groups of 32 columns and 32 banks of 8 bytes, stores in groups of 16 and 16 banks;
    a group costs the largest number of cells on one bank"""
    ve = t["vn_edge"].reshape(t["D"], n)
    cost = 0
    for width in (32, 16):
        for k in range(t["D"]):
            for v0 in range(0, n, width):
                e = ve[k, v0:v0 + width]
                e = e[e != PAD_EDGE]
                if e.size:
                    cost += int(np.bincount((e & 0xFFFF) % width).max())
    return cost


def check_tables(H, t):
    H = sp.csr_matrix(H)
    H.sort_indices()
    m, n = H.shape
    S, K, D = t["S"], t["K"], t["D"]
    assert S == H.nnz + t["pads"] and int(t["jptr"][K]) == S and t["jptr"][0] == 0
    deg = np.diff(H.indptr)
    # lanes: a permutation of the checks, degrees descending
    assert sorted(t["perm"].tolist()) == list(range(m)) and np.array_equal(t["iperm"][t["perm"]], np.arange(m))
    assert np.array_equal(t["row_deg"], deg[t["perm"]]) and (np.diff(t["row_deg"].astype(int)) <= 0).all()
    # a diagonal holds the checks of degree > j, then its pad cells
    cnt = np.array([(deg > j).sum() for j in range(K)])
    assert (np.diff(t["jptr"].astype(int)) >= cnt).all()
    ve = t["vn_edge"].reshape(D, n)
    slots = set()
    seen = [set() for _ in range(m)]  # positions used per lane
    Hc = sp.csc_matrix(H)
    Hc.sort_indices()
    for v in range(n):
        rows = Hc.indices[Hc.indptr[v]:Hc.indptr[v + 1]]
        for k in range(D):
            e = int(ve[k, v])
            if k >= len(rows):
                assert e == PAD_EDGE
                continue
            slot, lane, j = e & 0xFFFF, (e >> 16) & 0x3FF, e >> 26
            assert t["perm"][lane] == rows[k], "k-th edge of a column: its k-th check in ascending order"
            assert j < t["row_deg"][lane] and j not in seen[lane]
            seen[lane].add(j)
            assert slot == int(t["jptr"][j]) + lane and slot < S and slot not in slots
            assert slot < int(t["jptr"][j]) + cnt[j], "an edge names a pad slot"
            slots.add(slot)
            assert t["row_col"][slot] == v
    assert len(slots) == H.nnz and all(len(seen[l]) == t["row_deg"][l] for l in range(m))
    pad_slots = sorted(set(range(S)) - slots)
    assert len(pad_slots) == t["pads"] and all(t["row_col"][s] == 0 for s in pad_slots)
    # the listed order is the natural one's, and vn_edge_s follows the final vn_edge
    assert np.array_equal(t["vn_edge_s"].reshape(D, n), ve[:, t["vperm"]])
    assert model_cost(t, n) == t["cost"]


@pytest.mark.parametrize("pads", [0, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_layout_describes_the_graph_and_costs_no_more(case, pads, monkeypatch):
    monkeypatch.delenv("SWD_NATURAL_LAYOUT", raising=False)
    H = CASES[case]()
    t = layout(H, pads)
    assert t["pads"] <= pads
    check_tables(H, t)
    nat = dict(natural_tables(H), S=H.nnz, K=t["K"], D=t["D"])
    assert t["cost_natural"] == model_cost(nat, H.shape[1])
    assert t["cost"] <= t["cost_natural"]
    print(f"{case} pads {pads}: loads {t['loads'][1]} -> {t['loads'][0]}, stores {t['stores'][1]} -> {t['stores'][0]} cycles per node pass")
    again = layout(H, pads)
    for k, a in t.items():
        assert np.array_equal(a, again[k]), f"{k} differs on a second build"


def test_collapsed_diagonals_are_spread(monkeypatch):
    """every diagonal on bank 0: the natural layout serialises, permuted positions and pad cells must not"""
    monkeypatch.delenv("SWD_NATURAL_LAYOUT", raising=False)
    t = layout(collapsed_matrix(), 5)
    assert t["cost"] < t["cost_natural"]


@pytest.mark.parametrize("case", list(CASES))
def test_switch_restores_the_natural_layout_byte_for_byte(case, monkeypatch):
    monkeypatch.setenv("SWD_NATURAL_LAYOUT", "1")
    H = CASES[case]()
    t = layout(H, 8)
    assert t["pads"] == 0 and t["S"] == H.nnz and t["cost"] == t["cost_natural"]
    for k, a in natural_tables(H).items():
        assert a.dtype == t[k].dtype and a.tobytes() == t[k].tobytes(), k
