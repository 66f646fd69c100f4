"""The case table of tests/window_forms.py, checked on the host alone (no GPU): every case reaches the form it is for -- the record
of ``window_forms`` (include/swd.h, swd_window_forms: the code a handle's creation runs, without a device) equals the record written
in the table, field by field -- and the oracle's own exits on the case's syndromes reach the phase the case is for.  Then the table
as a whole: every form of the selection tree the suite means to test is reached by at least one case.
tests/test_gpu_window_forms.py decodes the same cases on the device."""
import os

import numpy as np
import pytest

from slidingwindowdecoder_amd import _lib
from tests import window_forms as T

if not os.path.exists(_lib.LIB_PATH):
    pytest.skip("libswd_hip.so not built (run __graft_entry__.build())", allow_module_level=True)

PLAN_FIELDS = ("nt", "vf", "dm", "kg", "sf", "big", "depth_fit", "lds_total", "gdg_parallel", "post_depth2", "general")


def probe(c, monkeypatch):
    from slidingwindowdecoder_amd import window_forms
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    H, pr, _ = T.problem(c)
    return window_forms([(H, pr)], decoder=c["decoder"], **c["kw"])


def assert_record(got, want, tag):
    for k in PLAN_FIELDS:
        assert got[k] == want[k], f"{tag}: plan field {k}: {got[k]} != {want[k]}"
    assert len(got["windows"]) == len(want["windows"])
    for i, (g, w) in enumerate(zip(got["windows"], want["windows"])):
        for k in w:
            assert g[k] == w[k], f"{tag}: window {i} field {k}: {g[k]} != {w[k]}"
    assert (got["kind"], got["stream_serial"], got["depth_launch"]) == (-1, -1, -1)  # no launch yet


@pytest.mark.parametrize("name", T.case_names())
def test_case_reaches_its_form(name, monkeypatch):
    c = T.case(name)
    assert_record(probe(c, monkeypatch), T.expected(name), name)


@pytest.mark.parametrize("name", list(T.PIPELINES))
def test_pipeline_reaches_its_form(name):
    from slidingwindowdecoder_amd import window_forms
    p = T.PIPELINES[name]
    plan, _ = T.pipeline_problem(name)
    got = window_forms(plan, **p["kw"])
    assert_record(got, T.expected(name), name)
    alone = []
    for m in p["mats"]:
        H = T.matrix(m)
        f = window_forms([(H, T.priors_for(H.shape[1]))], **p["kw"])
        alone.append((f["nt"], f["vf"], f["dm"], f["kg"], f["big"]))
    joint = (got["nt"], got["vf"], got["dm"], got["kg"], got["big"])
    if name == "pipe_joint_maxima":
        # the largest m and K come from window 0, the largest n and D from window 1: the variant covers them jointly
        (m0, n0), (m1, n1) = (w.mat.shape for w in plan.windows)
        K = [int(np.diff(w.mat.indptr).max()) for w in plan.windows]
        D = [int(w.mat.sum(axis=0).max()) for w in plan.windows]
        assert m0 > m1 and K[0] > K[1] and n1 > n0 and D[1] > D[0]
        assert joint[0] >= m0 and joint[0] * joint[1] >= n1 and joint[2] >= D[1] and 4 * joint[3] >= K[0]
        assert alone[0] != joint  # window 0 alone takes a smaller variant
    else:
        assert alone[0][4] == 0 and alone[1][4] == 1 and joint[4] == 1  # LDS-resident alone, large-graph form in the plan


@pytest.mark.parametrize("name", [c["name"] for c in T.CASES if c["decoder"] == "osd_window"])
def test_oracle_exits_cover_what_the_case_is_for(name):
    """a condition on the inputs, checked against the oracle alone"""
    b = T.oracle_exit_counts(name)
    c = T.case(name)
    if "osd" in c["aims"]:
        assert b[2] >= 4, b
    if "post" in c["aims"]:
        assert b[1] >= 4 and b[2] >= 4, b
    if "rare" in c["aims"]:
        assert b[3] + b[4] >= 1, b


@pytest.mark.parametrize("family", ["tuned", "lds1024", "big"])
def test_rare_exits_present_in_every_kernel_family(family):
    """classes 3 ("setting vn failed") and 4 ("peeling failed") both occur in the family: within one case on the kernels of up to 256
    threads and on the LDS-resident 1024-thread kernels; on the large-graph kernels in the two cases of one matrix and one syndrome
    set (tests/window_forms.py, rare_big)"""
    counts = [T.oracle_exit_counts(c["name"]) for c in T.CASES if c["family"] == family and "rare" in c["aims"]]
    assert counts
    if family != "big":
        assert any(b[3] > 0 and b[4] > 0 for b in counts), counts
    assert sum(b[3] for b in counts) > 0 and sum(b[4] for b in counts) > 0, counts


@pytest.mark.parametrize("name", [c["name"] for c in T.CASES if c["decoder"] != "osd_window"])
def test_guessing_cases_reach_the_decimation(name):
    """at least four shots whose pre-processing BP does not converge: the tree search runs"""
    assert T.oracle_gdg(name)[2].sum() >= 4


def test_rank_deficient_cases_are_rank_deficient():
    from oracle import oracle as O
    for name in ("rd_wave", "rd_quad", "rd_cols", "rd_block", "rd_colsw"):
        H = T.matrix(name)
        assert O.osd_window(H, channel_probs=T.priors_for(H.shape[1])).rank == H.shape[0] - 4


def test_table_reaches_every_listed_form():
    E = {n: T.expected(n) for n in T.case_names()}
    osdw = {n: e for n, e in E.items() if T.case(n)["decoder"] == "osd_window"}
    gdg = {n: e for n, e in E.items() if T.case(n)["decoder"] != "osd_window"}

    def variant(e):
        return (e["nt"], e["vf"], e["dm"], e["kg"], e["sf"], e["big"])

    def fam(e):
        return "big" if e["big"] else ("tuned" if e["nt"] <= 256 else "lds1024")
    lds = [(64, 4, 4, 2, 0, 0), (64, 4, 8, 16, 0, 0), (256, 2, 8, 16, 0, 0), (256, 4, 8, 16, 0, 0), (256, 2, 10, 12, 0, 0), (256, 7, 6, 9, 0, 0),
           (256, 7, 8, 16, 0, 0), (1024, 5, 6, 6, 1, 0), (1024, 5, 6, 9, 0, 0), (1024, 3, 10, 12, 0, 0), (1024, 8, 8, 16, 0, 0)]
    big = [(1024, 9, 6, 9, 0, 1), (1024, 9, 10, 16, 0, 1)]
    # every variant, once with a column at its column-weight bound (the cases named after the variant)
    assert {variant(e) for e in osdw.values()} == set(lds + big)
    for n, e in osdw.items():
        if n.split(":")[0].startswith(("v64", "v256", "v1024", "big_9")):
            assert int(T.matrix(T.case(n)["mat"]).sum(axis=0).max()) == e["dm"], n
    # <256, 7, 6, 9> uniform and depth-profiled
    assert {e["depth_fit"] for e in osdw.values() if variant(e) == (256, 7, 6, 9, 0, 0)} == {0, 1}
    # kinds: 0 and 3 on every variant with a kind-3 kernel, 5 and 6 on both large-graph variants, 0 on the others
    for v in lds + big:
        kinds = {e["kind"] for e in osdw.values() if variant(e) == v}
        assert kinds == ({5, 6} if v[5] else ({0, 3} if v[:4] in T.K3 else {0})), (v, kinds)
    assert {e["depth_launch"] for e in osdw.values() if e["depth_fit"] and e["kind"] == 3} == {1}
    # a row at 4 x KG on a 64-thread, a 256-thread and a 1024-thread variant without the heavy-check split
    at_4kg = {e["nt"] for n, e in osdw.items() if not e["sf"] and not e["big"]
              and int(np.diff(T.matrix(T.case(n)["mat"]).indptr).max()) == 4 * e["kg"]}
    assert at_4kg == {64, 256, 1024}
    # both live-mask widths on the tuned kernels
    assert {e["windows"][0]["mask_bytes"] for e in osdw.values() if fam(e) == "tuned"} == {6, 8}
    # heavy-check split: more than one T, all three group sizes in one graph, need == nt
    sf = [e["windows"][0] for e in osdw.values() if e["sf"]]
    assert len({w["split_t"] for w in sf}) >= 2
    assert any(min(w["split_1"], w["split_2"], w["split_4"]) > 0 for w in sf)
    assert any(w["split_need"] == 1024 for w in sf)
    # elimination routines per kernel family, with the numbers of checks at the bounds
    routines = {(fam(e), e["windows"][0]["osd0"]) for e in osdw.values()}
    assert routines >= {("tuned", "osd0_wave_reg"), ("big", "osd0_wave_reg"), ("tuned", "osd0_quad"), ("lds1024", "osd0_quad"),
                        ("lds1024", "osd0_cols"), ("lds1024", "osd0_block"), ("big", "osd0_colsw"), ("big", "osd0_block")}

    def rows(routine, family, dm=None):
        return {T.matrix(T.case(n)["mat"]).shape[0] for n, e in osdw.items()
                if e["windows"][0]["osd0"] == routine and fam(e) == family and (dm is None or e["dm"] == dm)}
    assert rows("osd0_quad", "tuned") >= {255, 256} and rows("osd0_quad", "lds1024") >= {255, 256}
    assert rows("osd0_cols", "lds1024") >= {257, 576}
    assert rows("osd0_colsw", "big") >= {577, 960}
    assert max(rows("osd0_block", "big", 6)) > 960 and rows("osd0_block", "big", 10)
    assert min(rows("osd0_block", "lds1024", 8)) >= 577 or 577 in rows("osd0_block", "lds1024", 8)
    assert any(r > 256 for r in rows("osd0_block", "lds1024", 10))
    assert any(r <= 256 for r in rows("osd0_wave_reg", "big"))
    # ... each routine also on a rank-deficient matrix
    assert {E[n]["windows"][0]["osd0"] for n in E if n.startswith("rd_")} == {"osd0_wave_reg", "osd0_quad", "osd0_cols", "osd0_colsw", "osd0_block"}
    # sweep: both methods over the sort keys and with arrays of their own; fewer candidates at a time than threads
    sweep = {(T.case(n)["kw"]["osd_method"], e["windows"][0]["cs_own"]) for n, e in osdw.items() if T.case(n)["kw"]["osd_method"] != "osd_0"}
    assert sweep >= {("osd_cs", 0), ("osd_cs", 1), ("osd_e", 0), ("osd_e", 1)}
    assert any(e["windows"][0]["cs_par"] < e["nt"] for n, e in osdw.items() if T.case(n)["kw"]["osd_method"] != "osd_0")
    # post phase, among the cases whose syndromes reach it
    post = {(fam(e), e["windows"][0]["post"]) for n, e in osdw.items() if "post" in T.case(n)["aims"]}
    assert post >= {("tuned", "sorted"), ("tuned", "lists"), ("tuned", "no_lists"), ("lds1024", "sorted"), ("lds1024", "no_lists"),
                    ("big", "renumbered"), ("big", "lists")}
    # guessing decoders: every variant that has kernels for them, serial / work items / bpgd / ensemble; depth-2 cache on and off
    for v in [x for x in lds if not x[4]] + big:
        kinds = {(T.case(n)["decoder"], e["kind"]) for n, e in gdg.items() if variant(e) == v}
        want = {("bpgdg_decoder", 8), ("bpgd_decoder", 8), ("bpgdg_decoder", 9)} if v[5] else {("bpgdg_decoder", 1), ("bpgd_decoder", 1), ("bpgdg_decoder", 7)}
        if v[0] <= 256:
            want |= {("bpgdg_decoder", 2)}
        assert kinds >= want, (v, kinds)
    assert {(fam(e), e["post_depth2"]) for e in gdg.values()} >= {("tuned", 0), ("tuned", 1), ("lds1024", 0), ("lds1024", 1), ("big", 1)}
