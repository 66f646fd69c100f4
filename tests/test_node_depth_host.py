"""Depth order of a window graph's variable nodes and the fit test of a depth profile (csrc/swd_graph.hip: Graph::fill_depth,
Graph::fits_depth, the listed-order model of Graph::layout_cost / optimize_layout) through the host-only entry point
``swd_graph_node_depth``: no GPU needed.  The order and the cost model are restated here in numpy, never taken from the library.

The matrices are the smallest ones that reach the <256, 7, 6, 9> kernels (1024 < n <= 1792, column weight <= 6, row weight <= 36) at
the bounds of its profile {6, 6, 3, 3, 3, 3, 2}: 256 listed nodes per cache row, at most 512 nodes of degree above 3 and 1536 of
degree above 2.  tests/test_gpu_node_depth.py decodes on them."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np
import pytest
import scipy.sparse as sp

from slidingwindowdecoder_amd import _lib
from tests.test_graph_layout import CASES, PAD_EDGE, layout

NT, VF, PROFILE = 256, 7, (6, 6, 3, 3, 3, 3, 2)


def matrix_with_column_degrees(m, degs, seed, cap=36):
    """m x len(degs), column v of weight degs[v], the rows filled evenly (each column takes the least-loaded rows, ties broken at
    random), columns shuffled; no row above `cap`"""
    rng = np.random.default_rng(seed)
    degs = np.asarray(degs)
    degs = degs[rng.permutation(len(degs))]
    load = np.zeros(m, np.int64)
    H = np.zeros((m, len(degs)), np.uint8)
    for v, d in enumerate(degs):
        rows = np.lexsort((rng.random(m), load))[:d]
        H[rows, v] = 1
        load[rows] += 1
    assert load.max() <= cap and load.min() >= 1 and (H.sum(axis=0) == degs).all()
    return sp.csr_matrix(H)


BOUNDARY_DEGS = [4] * 256 + [5] * 128 + [6] * 128 + [3] * 1024 + [2] * 128 + [1] * 128


@functools.lru_cache(maxsize=None)
def boundary_matrix():
    """(b) 200 x 1792: exactly 512 columns of degree 4 to 6, 1024 of degree 3, 256 of degree 1 or 2 -- every cache row of the profile
    at its depth, the last one full"""
    return matrix_with_column_degrees(200, BOUNDARY_DEGS, 11)


@functools.lru_cache(maxsize=None)
def short_matrix():
    """(c) 120 x 1030: listed row 4 holds six nodes (of degree 3, its depth), rows 5 and 6 are empty"""
    return matrix_with_column_degrees(120, [6] * 100 + [5] * 150 + [4] * 262 + [3] * 518, 12)


@functools.lru_cache(maxsize=None)
def misfit_matrix():
    """(d) the matrix of (b) with one of its degree-3 columns raised to degree 4 (n stays 1792, the most the kernel takes): 513
    columns of degree above 3, so the 513th listed node sits in a row of depth 3"""
    H = boundary_matrix().toarray()
    v = int(np.flatnonzero(H.sum(axis=0) == 3)[500])
    r = int(np.flatnonzero((H[:, v] == 0) & (H.sum(axis=1) < 36))[0])
    H[r, v] = 1
    assert (H.sum(axis=0) > 3).sum() == 513 and H.sum(axis=1).max() <= 36
    return sp.csr_matrix(H)


def priors_for(n):
    """distinct priors: a permuted prior table is then told from the table in column order"""
    return 0.002 + 0.03 * ((np.arange(n) * 37) % 101) / 101.0


def node_depth(H, pads=0, nt=NT, vf=VF, depth=PROFILE):
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libswd_hip.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    H = sp.csr_matrix(H)
    H.sort_indices()
    m, n = H.shape
    rp, ci = H.indptr.astype(np.int32), H.indices.astype(np.int32)
    pr = priors_for(n)
    desc = _lib.GraphDesc(m, n, int(H.nnz), rp.ctypes.data, ci.ctypes.data, pr.ctypes.data)
    dep = np.asarray(depth, np.int32)
    assert len(dep) == vf
    info = np.zeros(8, np.int32)
    assert L.swd_graph_node_depth(C.byref(desc), pads, nt, vf, dep.ctypes.data, info.ctypes.data, *([None] * 5)) == 0, _lib.last_error()
    D = int(info[2])
    t = dict(vdord=np.zeros(n, np.uint16), vn_edge_d=np.zeros(D * n, np.uint32), llr_d=np.zeros(n), vn_edge=np.zeros(D * n, np.uint32),
             llr=np.zeros(n))
    info2 = np.zeros(8, np.int32)
    assert L.swd_graph_node_depth(C.byref(desc), pads, nt, vf, dep.ctypes.data, info2.ctypes.data, *[a.ctypes.data for a in t.values()]) == 0
    assert np.array_equal(info, info2)
    t.update(fits=bool(info[0]), S=int(info[1]), D=D, loads=(int(info[3]), int(info[5])), stores=(int(info[4]), int(info[6])),
             pads=int(info[7]), prior=pr)
    return t


def listed_model_cost(vn_edge_d, D, n):
    """the cost model in listed order, restated: thread t serves listed positions t, t + NT, ...; loads go in aligned groups of 32
    listed positions over 32 banks of 8 bytes, stores in groups of 16 over 16 banks; a group costs its busiest bank"""
    ve = vn_edge_d.reshape(D, n)
    cost = []
    for width in (32, 16):
        c = 0
        for k in range(D):
            for i0 in range(0, n, width):
                e = ve[k, i0:i0 + width]
                e = e[e != PAD_EDGE]
                if e.size:
                    c += int(np.bincount((e & 0xFFFF) % width).max())
        cost.append(c)
    return tuple(cost)


MATRICES = {"boundary": boundary_matrix, "short": short_matrix, "misfit": misfit_matrix, "ragged": CASES["ragged"]}


@pytest.mark.parametrize("case", list(MATRICES))
def test_depth_order_and_listed_tables(case, monkeypatch):
    monkeypatch.delenv("SWD_NATURAL_LAYOUT", raising=False)
    H = MATRICES[case]()
    m, n = H.shape
    t = node_depth(H, pads=8)
    cdeg = np.asarray(H.sum(axis=0)).ravel().astype(np.int64)
    # a permutation, non-increasing in the exact degree, stable in the column index
    assert sorted(t["vdord"].tolist()) == list(range(n))
    dl = cdeg[t["vdord"]]
    assert (np.diff(dl) <= 0).all()
    assert all((np.diff(t["vdord"][dl == d].astype(int)) > 0).all() for d in np.unique(dl))
    assert np.array_equal(t["vdord"], np.argsort(-cdeg, kind="stable"))
    # the listed tables are the final tables in column order, permuted
    D = t["D"]
    assert D == cdeg.max()
    assert np.array_equal(t["vn_edge_d"].reshape(D, n), t["vn_edge"].reshape(D, n)[:, t["vdord"]])
    assert np.array_equal(t["llr"], np.log((1 - t["prior"]) / t["prior"]))
    assert t["llr_d"].tobytes() == t["llr"][t["vdord"]].tobytes()
    # ... which still describe the graph: column v has its degree's worth of edges at the front, each in a message slot of its own
    ve = t["vn_edge"].reshape(D, n)
    assert np.array_equal((ve != PAD_EDGE).sum(axis=0), cdeg) and all((ve[:cdeg[v], v] != PAD_EDGE).all() for v in range(n))
    slots = ve[ve != PAD_EDGE] & 0xFFFF
    assert len(set(slots.tolist())) == H.nnz and slots.max() < t["S"] and t["S"] == H.nnz + t["pads"] and t["pads"] <= 8


@pytest.mark.parametrize("natural", [False, True])
@pytest.mark.parametrize("case", list(MATRICES))
def test_listed_order_cost_model(case, natural, monkeypatch):
    if natural:
        monkeypatch.setenv("SWD_NATURAL_LAYOUT", "1")
    else:
        monkeypatch.delenv("SWD_NATURAL_LAYOUT", raising=False)
    H = MATRICES[case]()
    t = node_depth(H, pads=8)
    loads, stores = listed_model_cost(t["vn_edge_d"], t["D"], H.shape[1])
    assert (loads, stores) == (t["loads"][0], t["stores"][0])
    if natural:
        assert t["loads"][0] == t["loads"][1] and t["stores"][0] == t["stores"][1] and t["pads"] == 0
    else:
        nat = node_depth(H, pads=0)  # (pads 0 and the switch off: the descent may still permute positions and lanes)
        assert t["loads"][1] == nat["loads"][1] and t["stores"][1] == nat["stores"][1]
        assert sum(t["loads"][:1] + t["stores"][:1]) <= t["loads"][1] + t["stores"][1]
    print(f"{case} natural={natural}: loads {t['loads'][1]} -> {t['loads'][0]}, stores {t['stores'][1]} -> {t['stores'][0]} (listed order)")


def test_fit_decision_on_the_boundary_graphs():
    assert node_depth(boundary_matrix())["fits"]      # 512 above 3, 1536 above 2: every row at its depth
    assert node_depth(short_matrix())["fits"]
    assert not node_depth(misfit_matrix())["fits"]    # the 513th node of degree above 3 is listed in a row of depth 3
    # one row deeper and it fits again; one row of depth 2 too early and (b) does not
    assert node_depth(misfit_matrix(), depth=(6, 6, 4, 3, 3, 3, 2))["fits"]
    assert not node_depth(boundary_matrix(), depth=(6, 6, 3, 3, 3, 2, 2))["fits"]
    assert node_depth(boundary_matrix(), depth=(6, 4, 3, 3, 3, 3, 2))["fits"]      # (its second row lists the 256 nodes of degree 4)
    assert not node_depth(boundary_matrix(), depth=(5, 6, 3, 3, 3, 3, 2))["fits"]  # (its first row the nodes of degree 6 and 5)
    # more nodes than cache entries never fit; a last row that is partly filled does
    assert not node_depth(boundary_matrix(), vf=6, depth=(6,) * 6)["fits"]
    assert node_depth(short_matrix(), vf=5, depth=(6, 6, 3, 3, 3))["fits"]
    assert not node_depth(short_matrix(), vf=5, depth=(6, 6, 3, 3, 2))["fits"]  # (its six nodes of row 4 have degree 3)


def small_degree_matrix(degs):
    return matrix_with_column_degrees(8, degs, 3, cap=64)


@pytest.mark.parametrize("degs,fits", [
    ([3, 3, 3, 3, 2, 2, 2, 2, 1, 1, 1, 1], True),      # every row of four full and at its depth
    ([3, 3, 3, 3, 2, 2, 2, 2, 2, 1, 1, 1], False),     # a fifth node of degree 2 falls into the row of depth 1
    ([3, 3, 3, 3, 3, 2, 2, 2, 1, 1, 1, 1], False),     # a fifth node of degree 3 falls into the row of depth 2
    ([1, 2, 3, 1, 2, 3], True),                        # listed 3 3 2 2 | 1 1: shuffled columns, second row half full, third empty
    ([1] * 13, False),                                 # thirteen nodes, twelve entries
])
def test_fit_decision_small(degs, fits):
    assert node_depth(small_degree_matrix(degs), nt=4, vf=3, depth=(3, 2, 1))["fits"] == fits


# sha256 over the outputs of swd_graph_layout (tests/test_graph_layout.py, layout(): every table and figure, keys sorted) as the
# library computed them before the depth order existed
LAYOUT_PINS = {
    ("bb72_w3f1", 0): "77e7cbaed5e5e805b372f0336672a973d387fe6b40b68ef696c93e4d1825836e",
    ("bb72_w3f1", 8): "9306f204b492fb7b1e659de3af6cc1f8a177a6b228cad87f876896b41ff6cd58",
    ("ragged", 0): "90cb1dbc1673857e7fda398fd1e79f2a531976c07962cc530751d32b15827f1f",
    ("ragged", 8): "56a02b1e5e4ea1edf9dab65b8591d3a618bcef621c055f6e63bb4bf7a0a14226",
    ("collapsed", 0): "673415a13024c2e2996c03c00e6f6880b87783f9142f1a69cedd6dfdf223e0d1",
    ("collapsed", 8): "c6d059846f311b17d2c8e95281e93deb3e68a45ec80492bd3fffadcdbd4fecb1",
}


def layout_digest(t):
    h = hashlib.sha256()
    for k in sorted(t):
        h.update(k.encode())
        h.update(np.asarray(t[k]).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("case,pads", list(LAYOUT_PINS))
def test_graph_layout_outputs_are_unchanged(case, pads, monkeypatch):
    """swd_graph_layout keeps the column-order model and the tiers-of-two order: its outputs are byte-identical to those of the
    library without the depth order, before and after the listed-order path ran on the same matrix, and with the switch set"""
    monkeypatch.delenv("SWD_NATURAL_LAYOUT", raising=False)
    monkeypatch.delenv("SWD_UNIFORM_DEPTH", raising=False)
    H = CASES[case]()
    assert layout_digest(layout(H, pads)) == LAYOUT_PINS[case, pads]
    node_depth(H, pads=pads, nt=64, vf=4, depth=(8, 8, 8, 8))
    assert layout_digest(layout(H, pads)) == LAYOUT_PINS[case, pads]
    monkeypatch.setenv("SWD_UNIFORM_DEPTH", "1")
    assert layout_digest(layout(H, pads)) == LAYOUT_PINS[case, pads]
