"""Cache image of a window graph (csrc/swd_graph.hip: Graph::fill_image) through the host-only entry point ``swd_graph_cache_image``:
no GPU needed.  The image holds, per thread role, the registers the osd_window kernels of up to 256 threads used to build in every
unit from the graph's tables (csrc/swd_osdw_kernel.h: the former vn_cache_pack / vn_cache_pack_depth and cn_cache_load<FULL>).  What
those routines produce is restated here in Python from the tables the entry point returns beside the image -- edge words, priors,
jptr, degrees by lane -- and compared with the image word for word; the packing is never taken from the library.  The tables
themselves are compared with those of ``swd_graph_node_depth`` where that entry builds the same layout.

Cases: a mid window of the headline [[144,12,12]] (3,1) plan (n = 1728 = 6.75 x 256: the last cache row is partly empty), profiled and
uniform; a 200 x 1500 graph of column weights 1 .. 6 whose columns of weight 1 and 2 are listed in rows of depth 3 (dead positions
inside a live row; m = 200: the last wave serves eight checks); a 65 x 300 graph (wave 1 serves one check, waves 2 and 3 none) with a
check of degree 36 = 4 KG, checks of degree 5 and 7 and a check of degree 1; the ragged matrix of tests/test_graph_layout.py in the
<256, 2, 8, 16> and <64, 4, 8, 16> forms (one wave, K = 40); n = 1030 with empty cache rows."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from slidingwindowdecoder_amd import _lib
from tests.test_graph_layout import CASES, PAD_EDGE
from tests.test_node_depth_host import matrix_with_column_degrees, node_depth, priors_for, short_matrix

PROFILE = (6, 6, 3, 3, 3, 3, 2)
HEADLINE = (256, 7, 6, 9)


@functools.lru_cache(maxsize=None)
def headline_mid_window():
    from slidingwindowdecoder_amd.circuit import bb_dem
    from slidingwindowdecoder_amd.codes import bb_code
    from slidingwindowdecoder_amd.windows import plan_windows
    code, A, B = bb_code(144)
    dem = bb_dem(code, A, B, 0.006, 5)
    plan = plan_windows(dem.chk, dem.obs, dem.priors, 72, 3, 1, method=1)
    H = sp.csr_matrix(plan.windows[1].mat)
    assert H.shape == (216, 1728)
    return H


MIXED_DEGS = [4] * 150 + [5] * 150 + [6] * 150 + [3] * 400 + [2] * 350 + [1] * 300


@functools.lru_cache(maxsize=None)
def mixed_matrix():
    """200 x 1500, column weights 1 .. 6: 450 columns above weight 3 (cache rows 0 and 1, depth 6), the others -- weights 3, 2 and 1 --
    at listed positions 450 .. 1499, rows 1 to 5: columns of weight 1 in rows of depth 3 and 6.  tests/test_gpu_cache_image.py
    decodes on it."""
    return matrix_with_column_degrees(200, MIXED_DEGS, 21)


@functools.lru_cache(maxsize=None)
def few_checks_matrix():
    """65 x 300: check 0 of degree 36, check 1 of degree 1, the others of degree 5 and 7 in turn; every column used, weight <= 6"""
    rng = np.random.default_rng(65)
    m, n = 65, 300
    deg = [36, 1] + [5, 7] * 31 + [5]
    H = np.zeros((m, n), np.uint8)
    load = np.zeros(n, np.int64)
    for r in range(m):
        cols = np.lexsort((rng.random(n), load))[:deg[r]]  # the least-loaded columns, ties at random
        H[r, cols] = 1
        load[cols] += 1
    assert load.min() >= 1 and load.max() <= 6 and (H.sum(axis=1) == deg).all()
    return sp.csr_matrix(H)


def cache_image(H, variant, depth=None, pads=8):
    """the library's image of H for the kernel variant (nt, vf, dm, kg) and the tables it was packed from"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libswd_hip.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    nt, vf, dm, kg = variant
    H = sp.csr_matrix(H)
    H.sort_indices()
    m, n = H.shape
    rp, ci = H.indptr.astype(np.int32), H.indices.astype(np.int32)
    pr = priors_for(n)
    desc = _lib.GraphDesc(m, n, int(H.nnz), rp.ctypes.data, ci.ctypes.data, pr.ctypes.data)
    dep = None if depth is None else np.asarray(depth, np.int32)
    head = (C.byref(desc), pads, nt, vf, dm, kg, None if dep is None else dep.ctypes.data)
    info = np.zeros(8, np.int32)
    assert L.swd_graph_cache_image(*head, info.ctypes.data, *([None] * 6)) == 0, _lib.last_error()
    S, K, D, cv, cc = (int(x) for x in info[:5])
    t = dict(img_vn=np.zeros(cv * nt * 4, np.uint32), img_cn=np.zeros(cc * nt * 4, np.uint32), jptr=np.zeros(K + 1, np.uint16),
             row_deg=np.zeros(m, np.uint8), vn_edge=np.zeros(D * n, np.uint32), llr=np.zeros(n))
    info2 = np.zeros(8, np.int32)
    assert L.swd_graph_cache_image(*head, info2.ctypes.data, *[a.ctypes.data for a in t.values()]) == 0
    assert np.array_equal(info, info2)
    t.update(S=S, K=K, D=D, cv=cv, cc=cc, pads=int(info[5]), m=m, n=n)
    return t


def by_role(img, nt):
    """[chunks * nt * 4] chunk-major, role-minor -> [nt, chunks * 4]: the words of each role in order"""
    return img.reshape(-1, nt, 4).transpose(1, 0, 2).reshape(nt, -1)


def restated_node_part(t, variant, depth):
    """the former vn_cache_pack(_depth), per role: priors, then edp[][] (byte offsets of the cells, two per word), then par[][] (lane << 2)"""
    nt, vf, dm, kg = variant
    m, n, D, S = t["m"], t["n"], t["D"], t["S"]
    ve, llr = t["vn_edge"].reshape(D, n), t["llr"]
    dep = [min(d, dm) for d in (depth if depth is not None else [dm] * vf)]
    pw = sum((d + 1) // 2 for d in dep)
    out = np.zeros((nt, 2 * vf + 2 * pw), np.uint32)
    for t_ in range(nt):
        dead = (S + 1 + nt // 64 + (t_ >> 6)) << 3
        at = 2 * vf
        for i in range(vf):
            idx = t_ + i * nt
            valid = idx < n
            lo_hi = np.array([llr[idx] if valid else 0.0]).view(np.uint32)
            out[t_, 2 * i], out[t_, 2 * i + 1] = lo_hi[0], lo_hi[1]
            for k in range((dep[i] + 1) & ~1):
                ed, ph = dead, m << 2
                if valid and k < dep[i] and k < D and ve[k, idx] != PAD_EDGE:
                    e = int(ve[k, idx])
                    ed, ph = (e & 0xFFFF) << 3, ((e >> 16) & 0x3FF) << 2
                assert ed < 65536 and ph < 65536
                out[t_, at + k // 2] |= ed << (16 * (k & 1))
                out[t_, at + pw + k // 2] |= ph << (16 * (k & 1))
            at += (dep[i] + 1) // 2
    return out


def restated_check_part(t, variant):
    """the former cn_cache_load<FULL> for one thread per check: slp[] (byte offsets (jptr[k] + lane) << 3, the far slot beyond the
    degree), then lane | cnt << 16 | live << 24 (lane 0xFFFF: no check)"""
    nt, vf, dm, kg = variant
    m, S, jptr, deg = t["m"], t["S"], t["jptr"].astype(np.int64), t["row_deg"].astype(np.int64)
    out = np.zeros((nt, 2 * kg + 1), np.uint32)
    for t_ in range(nt):
        far = (S + 1 + (t_ >> 6)) << 3
        cnt = int(deg[t_]) if t_ < m else 0
        for k in range(4 * kg):
            sv = (int(jptr[k]) + t_) << 3 if k < cnt else far
            assert sv < 65536
            out[t_, k // 2] |= sv << (16 * (k & 1))
        out[t_, 2 * kg] = (t_ if t_ < m else 0xFFFF) | (cnt << 16) | (cnt << 24)
    return out


IMAGES = {
    "headline_mid_profiled": (headline_mid_window, HEADLINE, PROFILE),
    "headline_mid_uniform": (headline_mid_window, HEADLINE, None),
    "mixed_profiled": (mixed_matrix, HEADLINE, PROFILE),
    "mixed_uniform": (mixed_matrix, HEADLINE, None),
    "few_checks_profiled": (few_checks_matrix, HEADLINE, PROFILE),
    "few_checks_uniform": (few_checks_matrix, HEADLINE, None),
    "short_profiled": (short_matrix, HEADLINE, PROFILE),
    "ragged_256_2_8_16": (CASES["ragged"], (256, 2, 8, 16), None),
    "ragged_64_4_8_16": (CASES["ragged"], (64, 4, 8, 16), None),
}


@pytest.mark.parametrize("case", list(IMAGES))
def test_image_equals_the_restated_caches(case, monkeypatch):
    monkeypatch.delenv("SWD_NATURAL_LAYOUT", raising=False)
    make, variant, depth = IMAGES[case]
    nt, vf, dm, kg = variant
    H = make()
    t = cache_image(H, variant, depth)
    m, n = H.shape
    rdeg, cdeg = np.diff(sp.csr_matrix(H).indptr), np.asarray(H.sum(axis=0)).ravel()
    # the tables describe the graph: degrees by lane descending, diagonals that hold them, the columns' edges at the front
    assert np.array_equal(t["row_deg"], np.sort(rdeg)[::-1]) and t["K"] == rdeg.max() and t["D"] == cdeg.max()
    assert t["S"] == H.nnz + t["pads"] and t["jptr"][-1] == t["S"] and t["pads"] <= 8
    order = np.argsort(-cdeg, kind="stable") if depth is not None else np.arange(n)
    ve = t["vn_edge"].reshape(t["D"], n)
    assert np.array_equal((ve != PAD_EDGE).sum(axis=0), cdeg[order])
    pr = priors_for(n)
    assert t["llr"].tobytes() == np.log((1 - pr) / pr)[order].tobytes()
    # word for word
    want_vn, want_cn = restated_node_part(t, variant, depth), restated_check_part(t, variant)
    assert t["cv"] == (want_vn.shape[1] + 3) // 4 and t["cc"] == (want_cn.shape[1] + 3) // 4
    got_vn, got_cn = by_role(t["img_vn"], nt), by_role(t["img_cn"], nt)
    assert np.array_equal(got_vn[:, :want_vn.shape[1]], want_vn)
    assert np.array_equal(got_cn[:, :want_cn.shape[1]], want_cn)
    assert not got_vn[:, want_vn.shape[1]:].any() and not got_cn[:, want_cn.shape[1]:].any()  # (the tail of the last chunk)


def test_the_cases_hold_what_they_are_there_for():
    H = mixed_matrix()
    cdeg = np.sort(np.asarray(H.sum(axis=0)).ravel())[::-1]
    assert (cdeg[512:1500] <= 3).all() and (cdeg[512:1500] == 1).any() and (cdeg[450:512] < 6).all()  # weight 1 in depth 3, weight 3 in depth 6
    t = cache_image(H, HEADLINE, PROFILE)
    vn = by_role(t["img_vn"], 256)
    dead = [(t["S"] + 1 + 4 + w) << 3 for w in range(4)]
    row3 = vn[:, 14 + 8:14 + 10]  # edp words of cache row 3, depth 3 (rows 0 and 1 take three words each, row 2 two)
    p0, p2 = row3[:, 0] & 0xFFFF, row3[:, 1] & 0xFFFF
    assert any(p0[r] != dead[r >> 6] and p2[r] == dead[r >> 6] for r in range(256))  # a live node of weight 2: its third position is dead
    assert any(p2[r] != dead[r >> 6] for r in range(256))                            # ... beside nodes of weight 3 in the same row
    F = few_checks_matrix()
    t = cache_image(F, HEADLINE, PROFILE)
    cn = by_role(t["img_cn"], 256)[:, 18]
    assert (cn[:65] & 0xFFFF).tolist() == list(range(65)) and ((cn[65:] & 0xFFFF) == 0xFFFF).all() and not (cn[65:] >> 16).any()
    assert cn[0] >> 24 == 36 and {int(x) for x in cn[1:65] >> 24} == {7, 5, 1}
    assert headline_mid_window().shape[1] % 256 != 0


def test_tables_are_those_of_the_depth_entry(monkeypatch):
    """the profiled image is packed from the layout ``swd_graph_node_depth`` reports for the same graph, profile and pad cells"""
    monkeypatch.delenv("SWD_NATURAL_LAYOUT", raising=False)
    H = mixed_matrix()
    t, d = cache_image(H, HEADLINE, PROFILE), node_depth(H, pads=8)
    assert d["fits"] and t["S"] == d["S"] and np.array_equal(t["vn_edge"], d["vn_edge_d"]) and t["llr"].tobytes() == d["llr_d"].tobytes()


def test_refusals():
    L = _lib.lib() if os.path.exists(_lib.LIB_PATH) else pytest.skip("libswd_hip.so not built (run __graft_entry__.build())")
    H = sp.csr_matrix(mixed_matrix())
    rp, ci, pr = H.indptr.astype(np.int32), H.indices.astype(np.int32), priors_for(H.shape[1])
    desc = _lib.GraphDesc(H.shape[0], H.shape[1], int(H.nnz), rp.ctypes.data, ci.ctypes.data, pr.ctypes.data)
    info = np.zeros(8, np.int32)
    for variant, depth in (((64, 4, 8, 16), None), ((256, 7, 4, 9), None), ((256, 7, 6, 4), None), (HEADLINE, (6, 3, 3, 3, 3, 3, 2))):
        dep = None if depth is None else np.asarray(depth, np.int32)
        assert L.swd_graph_cache_image(C.byref(desc), 8, *variant, None if dep is None else dep.ctypes.data, info.ctypes.data, *([None] * 6)) == -1
        assert "swd_graph_cache_image" in _lib.last_error()
