"""Case table of the window kernels' forms (csrc/swd_osdw_kernel.h, pipeline_kernel): deterministic matrices, each built to reach
one form of the selection tree -- kernel variant, LDS layout flags, OSD-0 elimination routine, post-phase form, launch kind -- with
the form record the case must reach (``window_forms`` / ``last_form`` of the package, include/swd.h).

tests/test_window_forms_host.py checks the table on the host alone: the record of every case, and that the oracle's own exits on
the case's syndromes reach the phase the case is for.  tests/test_gpu_window_forms.py decodes every case on the device, asserts
the record and the kernel kind of the launch, and compares every output with the oracle.

The expected records are written out in full: a change of a selection rule or of a layout that moves a case onto another form
fails the host test, and the case then has to be re-aimed, not the record copied."""
import functools

import numpy as np
import scipy.sparse as sp


def graded_matrix(m, col_degs, heavy_rows=(), seed=0, dup=0):
    """(m + dup) x len(col_degs) check matrix with a prescribed column-degree multiset and row-weight profile.

    col_degs    [(degree, count), ...]
    heavy_rows  [(weight, count), ...]: these rows get exactly that weight, the other rows share the remaining edges evenly
    dup         the last `dup` rows repeat rows 0 .. dup - 1: a rank-deficient matrix (column degrees grow by one on those rows'
                columns), on which a random syndrome is inconsistent
    Columns take the rows with the largest remaining capacity (ties at random), heaviest columns first; then the columns are
    shuffled.  Asserts the degrees it promises."""
    rng = np.random.default_rng(seed)
    degs = np.concatenate([np.full(c, d, np.int64) for d, c in col_degs])
    degs = np.sort(degs)[::-1]
    total = int(degs.sum())
    heavy = [w for w, c in heavy_rows for _ in range(c)]
    rest_rows = m - len(heavy)
    rest = total - sum(heavy)
    assert rest_rows > 0 and rest >= rest_rows, (rest_rows, rest)
    cap = np.array(heavy + [rest // rest_rows + (1 if i < rest % rest_rows else 0) for i in range(rest_rows)], np.int64)
    want_rows = cap.copy()
    H = np.zeros((m, len(degs)), np.uint8)
    for v, d in enumerate(degs):
        rows = np.lexsort((rng.random(m), -cap))[:d]
        assert (cap[rows] > 0).all(), "row profile cannot hold the columns"
        H[rows, v] = 1
        cap[rows] -= 1
    assert (H.sum(axis=1) == want_rows).all() and (H.sum(axis=0) == degs).all()
    H = H[rng.permutation(m)][:, rng.permutation(len(degs))]
    if dup:
        H = np.concatenate([H, H[:dup]], axis=0)
    return sp.csr_matrix(H)


def priors_for(n, lo=0.002, span=0.03):
    """distinct priors, deterministic"""
    return lo + span * ((np.arange(n) * 37) % 101) / 101.0


def synthetic_syndromes(H, shots, seed, dense=0.5, err=0.004):
    """a third from sparse errors (of rate err + 0.0004 k for shot k), the rest random bits of density 0.02 .. `dense`
    (tests/test_gpu_node_depth.py)"""
    rng = np.random.default_rng(seed)
    m, n = H.shape
    synd = np.zeros((shots, m), np.uint8)
    for k in range(shots):
        if k % 3 == 0:
            synd[k] = (H @ (rng.random(n) < err + 0.0004 * k).astype(np.uint8)) % 2
        else:
            synd[k] = rng.random(m) < rng.uniform(0.02, dense)
    return synd


# ---- decoder parameters -------------------------------------------------------------------------------------------------------
# iteration caps that are multiples of four let an osd_window launch take the kernel that sums the history in registers (kind 3,
# large graphs: 6) where the variant has one; any other caps the plain kernel (kind 0 / 5)
M4 = dict(pre_max_iter=4, post_max_iter=8)
ODD = dict(pre_max_iter=3, post_max_iter=7)
POST_M4 = dict(pre_max_iter=4, post_max_iter=40)   # post-phase cases: enough iterations for the shortened graph to converge
POST_ODD = dict(pre_max_iter=3, post_max_iter=41)
OSD0 = dict(ms_scaling_factor=0.9, osd_method="osd_0")
OSD_CS = dict(ms_scaling_factor=0.9, osd_method="osd_cs", osd_order=3)
OSD_E = dict(ms_scaling_factor=0.9, osd_method="osd_e", osd_order=5)
GDG = dict(max_iter=6, ms_scaling_factor=0.9, max_iter_per_step=4, max_step=8, max_tree_depth=2, max_side_depth=4,
           max_tree_branch_step=4, max_side_branch_step=4)

# variants with a kind-3 kernel (csrc/swd_variants.h) and the two large-graph variants (kind 6): their cases run with both caps
K3 = {(256, 2, 10, 12), (256, 7, 6, 9), (1024, 5, 6, 6), (1024, 5, 6, 9), (1024, 9, 6, 9), (1024, 9, 10, 16)}

# ---- matrices: (rows, column degrees, heavy rows, seed[, duplicated rows]) ------------------------------------------------------
MATS = {
    # one per variant, a column at the variant's column-weight bound and (non-sf) a row at 4 x KG
    "v64_4_4_2": (40, [(4, 10), (3, 60), (2, 50)], [(8, 1)], 1),
    "v64_4_8_16": (48, [(8, 1), (3, 100), (2, 60)], [(64, 1)], 2),
    "v256_2_8_16": (100, [(8, 1), (3, 300), (2, 100)], [(64, 1)], 3),
    "v256_4_8_16": (120, [(8, 1), (3, 600), (2, 200)], [(64, 1)], 4),
    "v256_2_10_12": (100, [(10, 1), (3, 300), (2, 100)], [(48, 1)], 5),
    "v256_7_6_9_uniform": (150, [(6, 513), (3, 600)], [(36, 1)], 6),   # 513 columns above degree 3: one too many for the profile
    "v256_7_6_9_depth": (150, [(6, 100), (3, 1000)], [(36, 1)], 7),
    "v256_7_8_16": (150, [(8, 1), (3, 900), (2, 200)], [(64, 1)], 8),
    "v1024_5_6_6_sf": (257, [(6, 1), (3, 2100)], [], 19),              # m = 257: osd0_cols at its lower bound; T = 12
    "v1024_5_6_9": (520, [(6, 1), (3, 4498)], [(36, 1)], 10),          # 519 rows of weight 26: two threads each at T = 24 > 1024
    "v1024_3_10_12": (257, [(10, 1), (3, 2100)], [(48, 1)], 22),       # osd0_block: the DM = 10 kernel has no column form
    "v1024_8_8_16": (577, [(8, 1), (3, 2500)], [(64, 1)], 21),         # m = 577: beyond osd0_cols
    "big_9_6_9": (577, [(6, 1), (3, 4000), (2, 2000)], [(36, 1)], 23),  # osd0_colsw at m = 577
    "big_9_10_16": (577, [(10, 1), (3, 4000), (2, 2000)], [(36, 1)], 26),  # osd0_block: DM = 10
    # elimination routines at their bounds
    "quad256_m255": (255, [(6, 1), (3, 300), (2, 150)], [], 16),
    "quad256_m256": (256, [(6, 1), (3, 300), (2, 150)], [], 17),
    "quad1024_m255": (255, [(6, 1), (3, 1500), (2, 400)], [], 18),
    "quad1024_m256": (256, [(6, 1), (3, 1500), (2, 400)], [], 18),     # 256 checks on four threads each at T = 6: need == nt
    "cols_m576": (576, [(6, 1), (3, 2100)], [], 20),
    "colsw_m960": (960, [(3, 1500), (2, 700)], [], 24),
    "bigblock_m961": (961, [(3, 1500), (2, 700)], [], 25),
    "bigwave_m256": (256, [(2, 1000), (1, 7300)], [(64, 1)], 15),
    # rank-deficient (four repeated rows), decoded on random syndromes: inconsistent systems
    "rd_wave": (36, [(3, 70), (2, 50)], [], 50, 4),
    "rd_quad": (196, [(3, 300), (2, 100)], [], 51, 4),
    "rd_cols": (296, [(3, 2100)], [], 52, 4),
    "rd_block": (596, [(7, 1), (3, 2500)], [(60, 1)], 53, 4),
    "rd_colsw": (596, [(3, 4000), (2, 2000)], [], 54, 4),
    # heavy-check split: checks in all three group sizes (T = 8: 100 on one thread, 60 on two, 140 on four)
    "sf_three_groups": (300, [(3, 1500), (2, 500)], [(4, 100), (14, 60), (30, 30)], 42),
    # sweep arrays over the sort keys / behind the OSD-0 arrays
    "cs_over_keys": (120, [(6, 50), (3, 700), (2, 300)], [], 35),
    "cs_own_arrays": (100, [(3, 300), (2, 100)], [], 36),
    # post phase
    "post64": (60, [(3, 200)], [], 33),
    "post256": (200, [(3, 900), (2, 200)], [], 34),
    "nolists64": (64, [(2, 60), (1, 70)], [(64, 1)], 30),
    "nolists256": (250, [(2, 200), (1, 250)], [(64, 1)], 31),
    "nolists1024": (300, [(2, 200), (1, 262)], [(64, 1)], 32),
    # guessing decoders keep more state in LDS: smaller graphs for two of the 1024-thread variants
    "g1024_5_6_9": (300, [(6, 1), (3, 1500), (2, 500)], [(36, 1)], 10),
    "g1024_8_8_16": (300, [(8, 1), (3, 1500), (2, 500)], [(64, 1)], 12),
}


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "boundary":  # 200 x 1792, every cache row of the <256, 7, 6, 9> depth profile at its depth
        from tests.test_node_depth_host import boundary_matrix
        return boundary_matrix()
    return graded_matrix(*MATS[name][:3], seed=MATS[name][3], dup=MATS[name][4] if len(MATS[name]) > 4 else 0)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
# aims: what the oracle's exits on the case's syndromes must cover (tests/test_window_forms_host.py) --
#   "osd"   at least 4 shots through the OSD (exit class 2): elimination routines, sweep arrays
#   "post"  at least 4 shots in class 1 (post-phase BP converged) and 4 in class 2
#   "rare"  classes 3 ("setting vn failed") and 4 ("peeling failed") both present: one case per kernel family
# family: "tuned" (kernels of up to 256 threads), "lds1024", "big"
CASES = []


def _osdw(name, mat, method, aims, family, shots, sseed=1, dense=0.5, err=0.004, twin=False, post=False, osd0=False, prior="graded",
          caps=None, **extra):
    both = (("m4", POST_M4 if post else M4), ("odd", POST_ODD if post else ODD))
    for tag, cp in (both if twin else (("m4", caps or both[0][1]),)):
        CASES.append(dict(name=f"{name}:{tag}" if twin else name, mat=mat, decoder="osd_window", kw=dict(cp, **method, **extra),
                          aims=aims, family=family, shots=shots, sseed=sseed, dense=dense, err=err, osd0=osd0, prior=prior, env={}))


# variants (each with a column at its column-weight bound), the elimination routine each of them takes
_osdw("v64_4_4_2", "v64_4_4_2", OSD0, ("osd",), "tuned", 24, osd0=True)
_osdw("v64_4_8_16", "v64_4_8_16", OSD0, ("osd",), "tuned", 24)
_osdw("v256_2_8_16", "v256_2_8_16", OSD0, ("osd",), "tuned", 24)
_osdw("v256_4_8_16", "v256_4_8_16", OSD0, ("osd",), "tuned", 24)
_osdw("v256_2_10_12", "v256_2_10_12", OSD0, ("osd",), "tuned", 24, twin=True)
_osdw("v256_7_6_9_uniform", "v256_7_6_9_uniform", OSD0, ("osd",), "tuned", 16, twin=True)
_osdw("v256_7_6_9_depth", "v256_7_6_9_depth", OSD0, ("osd",), "tuned", 16, twin=True)
_osdw("v256_7_8_16", "v256_7_8_16", OSD0, ("osd",), "tuned", 16)
_osdw("v1024_5_6_6_sf", "v1024_5_6_6_sf", OSD0, ("osd",), "lds1024", 12, twin=True, osd0=True)
_osdw("v1024_5_6_9", "v1024_5_6_9", OSD0, ("osd",), "lds1024", 8, twin=True)
_osdw("v1024_3_10_12", "v1024_3_10_12", OSD0, ("osd",), "lds1024", 12, osd0=True)
_osdw("v1024_8_8_16", "v1024_8_8_16", OSD0, ("osd",), "lds1024", 8, osd0=True)
_osdw("big_9_6_9", "big_9_6_9", OSD0, ("osd",), "big", 8, twin=True, osd0=True)
_osdw("big_9_10_16", "big_9_10_16", OSD0, ("osd",), "big", 8, twin=True, osd0=True)
# elimination routines at their bounds
_osdw("quad256_m255", "quad256_m255", OSD0, ("osd",), "tuned", 16, osd0=True)
_osdw("quad256_m256", "quad256_m256", OSD0, ("osd",), "tuned", 16, osd0=True)
_osdw("quad1024_m255", "quad1024_m255", OSD0, ("osd",), "lds1024", 12, twin=True, osd0=True)
_osdw("quad1024_m256", "quad1024_m256", OSD0, ("osd",), "lds1024", 12, twin=True, osd0=True)
_osdw("cols_m576", "cols_m576", OSD0, ("osd",), "lds1024", 8, twin=True, osd0=True)
_osdw("colsw_m960", "colsw_m960", OSD0, ("osd",), "big", 8, twin=True, osd0=True)
_osdw("bigblock_m961", "bigblock_m961", OSD0, ("osd",), "big", 8, twin=True, osd0=True)
_osdw("bigwave_m256", "bigwave_m256", OSD0, ("osd",), "big", 8, twin=True, osd0=True)
# ... and on rank-deficient matrices with inconsistent syndromes
_osdw("rd_wave", "rd_wave", OSD0, ("osd",), "tuned", 24, osd0=True)
_osdw("rd_quad", "rd_quad", OSD0, ("osd",), "tuned", 16, osd0=True)
_osdw("rd_cols", "rd_cols", OSD0, ("osd",), "lds1024", 8, twin=True, osd0=True)
_osdw("rd_block", "rd_block", OSD0, ("osd",), "lds1024", 8, osd0=True)
_osdw("rd_colsw", "rd_colsw", OSD0, ("osd",), "big", 8, twin=True, osd0=True)
# heavy-check split
_osdw("sf_three_groups", "sf_three_groups", OSD0, ("osd",), "lds1024", 12, twin=True)
# higher-order sweep: arrays over the dead sort keys / behind the OSD-0 arrays; fewer candidates at a time than threads
_osdw("cs_over_keys", "cs_over_keys", OSD_CS, ("osd",), "tuned", 16, twin=True)
_osdw("e_over_keys", "cs_over_keys", OSD_E, ("osd",), "tuned", 16, twin=True)
_osdw("cs_own_arrays", "cs_own_arrays", OSD_CS, ("osd",), "tuned", 24)
_osdw("e_own_arrays", "cs_own_arrays", OSD_E, ("osd",), "tuned", 24)
_osdw("cs_par_below_nt", "v1024_5_6_9", OSD_CS, ("osd",), "lds1024", 8, twin=True)
# post phase: sorted / lists without sorting (new_n at 2 NT and 2 NT + 1) / no lists; large graphs: renumbered or not
_osdw("post64_new_n_128", "post64", OSD0, ("post",), "tuned", 48, sseed=3, post=True, new_n=128)
_osdw("post64_new_n_129", "post64", OSD0, ("post",), "tuned", 48, sseed=3, post=True, new_n=129)
_osdw("post256_new_n_512", "post256", OSD0, ("post",), "tuned", 48, twin=True, post=True, new_n=512)
_osdw("post256_new_n_513", "post256", OSD0, ("post",), "tuned", 48, twin=True, post=True, new_n=513)
# (columns of weight one and two: one iteration in front, so that the post phase has work left)
SHORT_PRE = dict(pre_max_iter=1, post_max_iter=40)
_osdw("nolists64", "nolists64", OSD0, ("post",), "tuned", 48, caps=SHORT_PRE)
_osdw("nolists256", "nolists256", OSD0, ("post",), "tuned", 48, caps=SHORT_PRE)
_osdw("nolists1024", "nolists1024", OSD0, ("post",), "lds1024", 16, caps=SHORT_PRE)
_osdw("post1024_sorted", "v1024_5_6_6_sf", OSD0, ("post",), "lds1024", 16, sseed=3, twin=True, post=True)
_osdw("big_new_n_2048", "colsw_m960", OSD0, ("post",), "big", 16, sseed=3, err=0.02, twin=True, post=True, new_n=2048)
_osdw("big_new_n_2049", "colsw_m960", OSD0, ("post",), "big", 16, sseed=3, err=0.02, twin=True, post=True, new_n=2049)
# the rare exits, one case per family: random syndromes on a short new_n
# (uniform priors of 0.01; the tuned case is (b) of tests/test_gpu_node_depth.py, here also through the kind-0 kernel)
RARE_M4, RARE_ODD = dict(pre_max_iter=4, post_max_iter=12), dict(pre_max_iter=3, post_max_iter=11)
for _tag, _caps in (("m4", RARE_M4), ("odd", RARE_ODD)):
    _osdw(f"rare_tuned:{_tag}", "boundary", dict(ms_scaling_factor=0.9, osd_method="osd_cs", osd_order=2), ("rare",), "tuned", 48, sseed=10,
          prior="uniform", caps=_caps, new_n=210)
    _osdw(f"rare_lds1024:{_tag}", "v1024_5_6_6_sf", OSD0, ("rare",), "lds1024", 16, sseed=2, prior="uniform", caps=_caps, new_n=260)
# (large graphs: no single set of 16 syndromes was found on which the oracle leaves through both rare exits -- 120 sets on three
# graphs were searched; on this one the same shot leaves through "peeling failed" after four iterations in front and through
# "setting vn failed" after three, so the two cases together cover both exits)
_osdw("rare_big", "big_9_6_9", OSD0, ("rare",), "big", 16, twin=True, new_n=600)


# guessing decoders: every variant with kernels for them and both large-graph variants, on the variants' matrices --
#   serial tree walk (kind 1, large graphs 8; SWD_GDG_SERIAL=1 when the decoder is built), work items (kind 2, the variants of up to
#   256 threads), bpgd_decoder (kind 1 / 8), the threaded ensemble (kind 7 / 9)
def _gdg(name, mat, decoder, family, shots, env=None, **extra):
    CASES.append(dict(name=name, mat=mat, decoder=decoder, kw=dict(GDG, **extra), aims=("gdg",), family=family, shots=shots, sseed=1,
                      dense=0.5, err=0.004, osd0=False, prior="graded", env=env or {}))


GDG_MATS = [("v64_4_4_2", "tuned", 16, True), ("v64_4_8_16", "tuned", 16, True), ("v256_2_8_16", "tuned", 16, True),
            ("v256_4_8_16", "tuned", 16, True), ("v256_2_10_12", "tuned", 16, True), ("v256_7_6_9_depth", "tuned", 16, True),
            ("v256_7_8_16", "tuned", 16, True), ("g1024_5_6_9", "lds1024", 8, False), ("v1024_3_10_12", "lds1024", 8, False),
            ("g1024_8_8_16", "lds1024", 8, False), ("big_9_6_9", "big", 8, False), ("bigwave_m256", "big", 8, False)]
for _m, _fam, _shots, _k2 in GDG_MATS:
    _gdg(f"gdg_serial_{_m}", _m, "bpgdg_decoder", _fam, _shots, env={"SWD_GDG_SERIAL": "1"})
    if _k2:
        _gdg(f"gdg_items_{_m}", _m, "bpgdg_decoder", _fam, _shots)
    _gdg(f"gd_{_m}", _m, "bpgd_decoder", _fam, _shots)
    _gdg(f"ens_{_m}", _m, "bpgdg_decoder", _fam, _shots, multi_thread=True)
# the depth-2 cache of the shortened graph is off when a window keeps more than 2 NT columns (the large-graph kernels refuse those)
_gdg("gdg_depth2_off_tuned", "v64_4_8_16", "bpgdg_decoder", "tuned", 16, env={"SWD_GDG_SERIAL": "1"}, new_n=161)
_gdg("gdg_depth2_off_lds1024", "v1024_3_10_12", "bpgdg_decoder", "lds1024", 8, env={"SWD_GDG_SERIAL": "1"}, new_n=2101)


def case_names():
    return [c["name"] for c in CASES]


def case(name):
    return next(c for c in CASES if c["name"] == name)


def problem(c):
    """(H, priors, syndromes) of a single-window case"""
    H = matrix(c["mat"])
    pr = priors_for(H.shape[1]) if c["prior"] == "graded" else np.full(H.shape[1], 0.01)
    return H, pr, synthetic_syndromes(H, c["shots"], c["sseed"], c["dense"], c["err"])


# ---- pipelines: two windows on a block-diagonal global matrix, every column committed -------------------------------------------
MATS.update({
    "pipe_tall": (200, [(3, 300), (2, 100)], [(40, 1)], 60),   # the plan's largest m and K
    "pipe_wide": (100, [(8, 1), (3, 800), (2, 100)], [], 61),  # ... and its largest n and D: jointly <256, 4, 8, 16>
    "pipe_small": (100, [(3, 300), (2, 100)], [], 62),         # alone: <256, 2, 8, 16>; beside a large graph the whole plan is large
})
PIPELINES = {
    # (at least four iterations in front: the oracle's host loop re-uses one decoder object per window, whose history slot of a
    # fourth iteration that never ran would carry the previous shot's value; the device gives every shot a new object's history)
    "pipe_joint_maxima": dict(mats=("pipe_tall", "pipe_wide"), kw=dict(pre_max_iter=5, post_max_iter=7, **OSD_CS), shots=24, sseed=1,
                              family="tuned"),
    "pipe_one_window_big": dict(mats=("pipe_small", "big_9_6_9"), kw=dict(M4, **OSD0), shots=8, sseed=2, family="big"),
}


@functools.lru_cache(maxsize=None)
def pipeline_problem(name):
    """(WindowPlan, detector bits [shots, rows]) of a pipeline case"""
    from slidingwindowdecoder_amd.windows import Window, WindowPlan
    p = PIPELINES[name]
    Hs = [matrix(m) for m in p["mats"]]
    chk = sp.block_diag(Hs, format="csr")
    pri = np.concatenate([priors_for(H.shape[1]) for H in Hs])
    wins, r0, c0 = [], 0, 0
    for i, H in enumerate(Hs):
        m, n = H.shape
        wins.append(Window(r0, r0 + m, c0, n, n, H, pri[c0:c0 + n], i == len(Hs) - 1))
        r0, c0 = r0 + m, c0 + n
    plan = WindowPlan(chk, None, pri, np.arange(c0), [], wins, None, 0)
    det = np.concatenate([synthetic_syndromes(H, p["shots"], p["sseed"] + i) for i, H in enumerate(Hs)], axis=1)
    det.setflags(write=False)
    return plan, det


# ---- the oracle's answers, computed once per case and left unchanged ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_osdw(name):
    """(decoded vectors, result records, OSD-0 vectors or None) of an osd_window case"""
    from oracle import oracle as O
    c = case(name)
    H, pr, synd = problem(c)
    ora = O.osd_window(H, channel_probs=pr, **c["kw"])
    want, res = ora.decode_batch(synd)
    osd0 = None
    if c["osd0"]:  # (the batch call keeps no OSD-0 vector: one decode per shot, each with a new object's history)
        osd0 = np.zeros_like(want)
        for k in range(len(synd)):
            ora.clear_history()
            ora.decode(synd[k])
            osd0[k] = ora.osd0_decoding
        osd0.setflags(write=False)
    for a in (want, res):
        a.setflags(write=False)
    return want, res, osd0


def oracle_exit_counts(name):
    return np.bincount(oracle_osdw(name)[1]["exit_class"], minlength=5)


@functools.lru_cache(maxsize=None)
def oracle_gdg(name):
    """(vectors, converge flags, shots that went past the pre-processing BP, min_pm, per-shot (winner, ties, BP blocks) of the
    threaded ensemble or None) of a guessing-decoder case"""
    from oracle import oracle as O
    c = case(name)
    H, pr, synd = problem(c)
    ora = getattr(O, c["decoder"])(H, channel_probs=pr, **c["kw"])
    ens = bool(c["kw"].get("multi_thread"))
    B = len(synd)
    want, conv, post, pm = np.zeros((B, H.shape[1]), np.uint8), np.zeros(B, bool), np.zeros(B, bool), np.zeros(B)
    info = np.zeros((B, 3), np.int64) if ens else None
    for k in range(B):
        ora.clear_history()
        want[k] = ora.decode(synd[k])
        conv[k], post[k], pm[k] = bool(ora.converge), ora._res.exit_class != 0, ora.min_pm
        if ens and post[k]:
            _, winner, ties = ora.ensemble_info()
            info[k] = (winner, ties, ora.ensemble_blocks()[0])
    for a in (want, conv, post, pm):
        a.setflags(write=False)
    return want, conv, post, pm, info


def expected(name):
    """the form record a case must reach, in the shape of ``window_forms`` / ``last_form`` (kind and depth_launch: of its launch)"""
    plan, kind, depth_launch, wins = EXPECT[name]
    out = dict(zip(("nt", "vf", "dm", "kg", "sf", "big", "depth_fit", "lds_total", "gdg_parallel", "post_depth2"), plan))
    out.update(general=0, kind=kind, stream_serial=0, depth_launch=depth_launch)
    out["windows"] = [dict(zip(WINDOW_FIELDS, w)) for w in wins]
    return out


WINDOW_FIELDS = ("lslot", "post_lds", "osd_lds", "owide_ring", "cs_own", "cs_par", "mask_bytes", "osd0", "post", "split_t", "split_1",
                 "split_2", "split_4", "split_need", "wm", "pads")
# name: ((nt, vf, dm, kg, sf, big, depth_fit, lds_total, gdg_parallel, post_depth2), kernel kind of the launch, depth-profiled launcher,
#        [one tuple of WINDOW_FIELDS per window])
EXPECT = {
    "v64_4_4_2": ((64, 4, 4, 2, 0, 0, 0, 7056, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 1, 64, 6, 'osd0_wave_reg', 'sorted', 0, 0, 0, 0, 0, 1, 7)]),
    "v64_4_8_16": ((64, 4, 8, 16, 0, 0, 0, 9200, 0, 0), 0, 0,
        [('none', 0, 0, 0, 0, 64, 8, 'osd0_wave_reg', 'no_lists', 0, 0, 0, 0, 0, 1, 63)]),
    "v256_2_8_16": ((256, 2, 8, 16, 0, 0, 0, 20304, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 1, 256, 8, 'osd0_quad', 'lists', 0, 0, 0, 0, 0, 2, 63)]),
    "v256_4_8_16": ((256, 4, 8, 16, 0, 0, 0, 26864, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 256, 8, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 2, 63)]),
    "v256_2_10_12:m4": ((256, 2, 10, 12, 0, 0, 0, 17888, 0, 0), 3, 0,
        [('staged', 0, 0, 0, 1, 256, 6, 'osd0_quad', 'lists', 0, 0, 0, 0, 0, 2, 47)]),
    "v256_2_10_12:odd": ((256, 2, 10, 12, 0, 0, 0, 17888, 0, 0), 0, 0,
        [('staged', 0, 0, 0, 1, 256, 6, 'osd0_quad', 'lists', 0, 0, 0, 0, 0, 2, 47)]),
    "v256_7_6_9_uniform:m4": ((256, 7, 6, 9, 0, 0, 0, 43488, 0, 0), 3, 0,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 3, 35)]),
    "v256_7_6_9_uniform:odd": ((256, 7, 6, 9, 0, 0, 0, 43488, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 3, 35)]),
    "v256_7_6_9_depth:m4": ((256, 7, 6, 9, 0, 0, 1, 38640, 0, 0), 3, 1,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 3, 35)]),
    "v256_7_6_9_depth:odd": ((256, 7, 6, 9, 0, 0, 1, 38640, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 3, 35)]),
    "v256_7_8_16": ((256, 7, 8, 16, 0, 0, 0, 38064, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 256, 8, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 3, 63)]),
    "v1024_5_6_6_sf:m4": ((1024, 5, 6, 6, 1, 0, 0, 73568, 0, 0), 3, 0,
        [('staged', 1, 0, 0, 0, 576, 8, 'osd0_cols', 'sorted', 12, 0, 119, 138, 790, 5, 24)]),
    "v1024_5_6_6_sf:odd": ((1024, 5, 6, 6, 1, 0, 0, 73568, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 576, 8, 'osd0_cols', 'sorted', 12, 0, 119, 138, 790, 5, 24)]),
    "v1024_5_6_9:m4": ((1024, 5, 6, 9, 0, 0, 0, 150672, 0, 0), 3, 0,
        [('staged', 1, 0, 0, 0, 640, 8, 'osd0_cols', 'sorted', 0, 0, 0, 0, 0, 9, 35)]),
    "v1024_5_6_9:odd": ((1024, 5, 6, 9, 0, 0, 0, 150672, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 640, 8, 'osd0_cols', 'sorted', 0, 0, 0, 0, 0, 9, 35)]),
    "v1024_3_10_12": ((1024, 3, 10, 12, 0, 0, 0, 73664, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 576, 8, 'osd0_block', 'sorted', 0, 0, 0, 0, 0, 5, 47)]),
    "v1024_8_8_16": ((1024, 8, 8, 16, 0, 0, 0, 145520, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 1, 256, 8, 'osd0_block', 'sorted', 0, 0, 0, 0, 0, 10, 63)]),
    "big_9_6_9:m4": ((1024, 9, 6, 9, 0, 1, 0, 92720, 0, 0), 6, 0,
        [('staged', 1, 1, 64, 0, 512, 8, 'osd0_colsw', 'renumbered', 0, 0, 0, 0, 0, 10, 0)]),
    "big_9_6_9:odd": ((1024, 9, 6, 9, 0, 1, 0, 92720, 0, 0), 5, 0,
        [('staged', 1, 1, 64, 0, 512, 8, 'osd0_colsw', 'renumbered', 0, 0, 0, 0, 0, 10, 0)]),
    "big_9_10_16:m4": ((1024, 9, 10, 16, 0, 1, 0, 125280, 0, 0), 6, 0,
        [('staged', 1, 1, 64, 0, 512, 8, 'osd0_block', 'renumbered', 0, 0, 0, 0, 0, 10, 0)]),
    "big_9_10_16:odd": ((1024, 9, 10, 16, 0, 1, 0, 125280, 0, 0), 5, 0,
        [('staged', 1, 1, 64, 0, 512, 8, 'osd0_block', 'renumbered', 0, 0, 0, 0, 0, 10, 0)]),
    "quad256_m255": ((256, 2, 8, 16, 0, 0, 0, 33424, 0, 0), 0, 0,
        [('staged', 0, 0, 0, 1, 256, 6, 'osd0_quad', 'lists', 0, 0, 0, 0, 0, 4, 4)]),
    "quad256_m256": ((256, 2, 8, 16, 0, 0, 0, 33488, 0, 0), 0, 0,
        [('staged', 0, 0, 0, 1, 256, 6, 'osd0_quad', 'lists', 0, 0, 0, 0, 0, 4, 4)]),
    "quad1024_m255:m4": ((1024, 5, 6, 6, 1, 0, 0, 52480, 0, 0), 3, 0,
        [('staged', 0, 0, 0, 0, 256, 8, 'osd0_quad', 'lists', 6, 0, 0, 255, 1020, 4, 19)]),
    "quad1024_m255:odd": ((1024, 5, 6, 6, 1, 0, 0, 52480, 0, 0), 0, 0,
        [('staged', 0, 0, 0, 0, 256, 8, 'osd0_quad', 'lists', 6, 0, 0, 255, 1020, 4, 19)]),
    "quad1024_m256:m4": ((1024, 5, 6, 6, 1, 0, 0, 52480, 0, 0), 3, 0,
        [('staged', 0, 0, 0, 0, 256, 8, 'osd0_quad', 'lists', 6, 0, 0, 256, 1024, 4, 17)]),
    "quad1024_m256:odd": ((1024, 5, 6, 6, 1, 0, 0, 52480, 0, 0), 0, 0,
        [('staged', 0, 0, 0, 0, 256, 8, 'osd0_quad', 'lists', 6, 0, 0, 256, 1024, 4, 17)]),
    "cols_m576:m4": ((1024, 5, 6, 6, 1, 0, 0, 105456, 0, 0), 3, 0,
        [('staged', 0, 0, 0, 0, 256, 8, 'osd0_cols', 'lists', 12, 576, 0, 0, 576, 9, 10)]),
    "cols_m576:odd": ((1024, 5, 6, 6, 1, 0, 0, 105456, 0, 0), 0, 0,
        [('staged', 0, 0, 0, 0, 256, 8, 'osd0_cols', 'lists', 12, 576, 0, 0, 576, 9, 10)]),
    "colsw_m960:m4": ((1024, 9, 6, 9, 0, 1, 0, 151856, 0, 0), 6, 0,
        [('staged', 1, 1, 64, 1, 256, 8, 'osd0_colsw', 'renumbered', 0, 0, 0, 0, 0, 15, 0)]),
    "colsw_m960:odd": ((1024, 9, 6, 9, 0, 1, 0, 151856, 0, 0), 5, 0,
        [('staged', 1, 1, 64, 1, 256, 8, 'osd0_colsw', 'renumbered', 0, 0, 0, 0, 0, 15, 0)]),
    "bigblock_m961:m4": ((1024, 9, 6, 9, 0, 1, 0, 151328, 0, 0), 6, 0,
        [('staged', 1, 1, 0, 1, 256, 8, 'osd0_block', 'renumbered', 0, 0, 0, 0, 0, 16, 0)]),
    "bigblock_m961:odd": ((1024, 9, 6, 9, 0, 1, 0, 151328, 0, 0), 5, 0,
        [('staged', 1, 1, 0, 1, 256, 8, 'osd0_block', 'renumbered', 0, 0, 0, 0, 0, 16, 0)]),
    "bigwave_m256:m4": ((1024, 9, 10, 16, 0, 1, 0, 105536, 0, 0), 6, 0,
        [('staged', 1, 1, 0, 0, 1024, 8, 'osd0_wave_reg', 'renumbered', 0, 0, 0, 0, 0, 4, 0)]),
    "bigwave_m256:odd": ((1024, 9, 10, 16, 0, 1, 0, 105536, 0, 0), 5, 0,
        [('staged', 1, 1, 0, 0, 1024, 8, 'osd0_wave_reg', 'renumbered', 0, 0, 0, 0, 0, 4, 0)]),
    "rd_wave": ((64, 4, 8, 16, 0, 0, 0, 7104, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 1, 64, 6, 'osd0_wave_reg', 'sorted', 0, 0, 0, 0, 0, 1, 8)]),
    "rd_quad": ((256, 2, 8, 16, 0, 0, 0, 29824, 0, 0), 0, 0,
        [('staged', 0, 0, 0, 1, 256, 6, 'osd0_quad', 'lists', 0, 0, 0, 0, 0, 4, 5)]),
    "rd_cols:m4": ((1024, 5, 6, 6, 1, 0, 0, 74992, 0, 0), 3, 0,
        [('staged', 1, 0, 0, 0, 576, 8, 'osd0_cols', 'sorted', 12, 0, 300, 0, 600, 5, 21)]),
    "rd_cols:odd": ((1024, 5, 6, 6, 1, 0, 0, 74992, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 576, 8, 'osd0_cols', 'sorted', 12, 0, 300, 0, 600, 5, 21)]),
    "rd_block": ((1024, 8, 8, 16, 0, 0, 0, 148176, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 1, 256, 8, 'osd0_block', 'sorted', 0, 0, 0, 0, 0, 10, 59)]),
    "rd_colsw:m4": ((1024, 9, 6, 9, 0, 1, 0, 93120, 0, 0), 6, 0,
        [('staged', 1, 1, 64, 0, 512, 8, 'osd0_colsw', 'renumbered', 0, 0, 0, 0, 0, 10, 0)]),
    "rd_colsw:odd": ((1024, 9, 6, 9, 0, 1, 0, 93120, 0, 0), 5, 0,
        [('staged', 1, 1, 64, 0, 512, 8, 'osd0_colsw', 'renumbered', 0, 0, 0, 0, 0, 10, 0)]),
    "sf_three_groups:m4": ((1024, 5, 6, 6, 1, 0, 0, 66992, 0, 0), 3, 0,
        [('staged', 1, 0, 0, 1, 256, 8, 'osd0_block', 'sorted', 8, 100, 60, 140, 780, 5, 30)]),
    "sf_three_groups:odd": ((1024, 5, 6, 6, 1, 0, 0, 66992, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 1, 256, 8, 'osd0_block', 'sorted', 8, 100, 60, 140, 780, 5, 30)]),
    "cs_over_keys:m4": ((256, 7, 6, 9, 0, 0, 1, 36496, 0, 0), 3, 1,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 2, 24)]),
    "cs_over_keys:odd": ((256, 7, 6, 9, 0, 0, 1, 36496, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 2, 24)]),
    "e_over_keys:m4": ((256, 7, 6, 9, 0, 0, 1, 36496, 0, 0), 3, 1,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 2, 24)]),
    "e_over_keys:odd": ((256, 7, 6, 9, 0, 0, 1, 36496, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 2, 24)]),
    "cs_own_arrays": ((256, 2, 8, 16, 0, 0, 0, 17776, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 1, 256, 6, 'osd0_quad', 'lists', 0, 0, 0, 0, 0, 2, 10)]),
    "e_own_arrays": ((256, 2, 8, 16, 0, 0, 0, 17776, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 1, 256, 6, 'osd0_quad', 'lists', 0, 0, 0, 0, 0, 2, 10)]),
    "cs_par_below_nt:m4": ((1024, 5, 6, 9, 0, 0, 0, 150672, 0, 0), 3, 0,
        [('staged', 1, 0, 0, 0, 640, 8, 'osd0_cols', 'sorted', 0, 0, 0, 0, 0, 9, 35)]),
    "cs_par_below_nt:odd": ((1024, 5, 6, 9, 0, 0, 0, 150672, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 640, 8, 'osd0_cols', 'sorted', 0, 0, 0, 0, 0, 9, 35)]),
    "post64_new_n_128": ((64, 4, 8, 16, 0, 0, 0, 9648, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 64, 6, 'osd0_wave_reg', 'sorted', 0, 0, 0, 0, 0, 1, 9)]),
    "post64_new_n_129": ((64, 4, 8, 16, 0, 0, 0, 9664, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 64, 6, 'osd0_wave_reg', 'lists', 0, 0, 0, 0, 0, 1, 9)]),
    "post256_new_n_512:m4": ((256, 7, 6, 9, 0, 0, 1, 38976, 0, 0), 3, 1,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 4, 15)]),
    "post256_new_n_512:odd": ((256, 7, 6, 9, 0, 0, 1, 38976, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 4, 15)]),
    "post256_new_n_513:m4": ((256, 7, 6, 9, 0, 0, 1, 38976, 0, 0), 3, 1,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'lists', 0, 0, 0, 0, 0, 4, 15)]),
    "post256_new_n_513:odd": ((256, 7, 6, 9, 0, 0, 1, 38976, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'lists', 0, 0, 0, 0, 0, 4, 15)]),
    "nolists64": ((64, 4, 8, 16, 0, 0, 0, 8960, 0, 0), 0, 0,
        [('none', 0, 0, 0, 0, 64, 8, 'osd0_wave_reg', 'no_lists', 0, 0, 0, 0, 0, 1, 34)]),
    "nolists256": ((256, 2, 8, 16, 0, 0, 0, 33760, 0, 0), 0, 0,
        [('none', 0, 0, 0, 1, 256, 8, 'osd0_quad', 'no_lists', 0, 0, 0, 0, 0, 4, 63)]),
    "nolists1024": ((1024, 8, 8, 16, 0, 0, 0, 41936, 0, 0), 0, 0,
        [('none', 0, 0, 0, 1, 256, 8, 'osd0_block', 'no_lists', 0, 0, 0, 0, 0, 5, 63)]),
    "post1024_sorted:m4": ((1024, 5, 6, 6, 1, 0, 0, 73568, 0, 0), 3, 0,
        [('staged', 1, 0, 0, 0, 576, 8, 'osd0_cols', 'sorted', 12, 0, 119, 138, 790, 5, 24)]),
    "post1024_sorted:odd": ((1024, 5, 6, 6, 1, 0, 0, 73568, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 576, 8, 'osd0_cols', 'sorted', 12, 0, 119, 138, 790, 5, 24)]),
    "big_new_n_2048:m4": ((1024, 9, 6, 9, 0, 1, 0, 152112, 0, 0), 6, 0,
        [('staged', 1, 1, 64, 1, 256, 8, 'osd0_colsw', 'renumbered', 0, 0, 0, 0, 0, 15, 0)]),
    "big_new_n_2048:odd": ((1024, 9, 6, 9, 0, 1, 0, 152112, 0, 0), 5, 0,
        [('staged', 1, 1, 64, 1, 256, 8, 'osd0_colsw', 'renumbered', 0, 0, 0, 0, 0, 15, 0)]),
    "big_new_n_2049:m4": ((1024, 9, 6, 9, 0, 1, 0, 152112, 0, 0), 6, 0,
        [('staged', 0, 1, 64, 1, 256, 8, 'osd0_colsw', 'lists', 0, 0, 0, 0, 0, 15, 0)]),
    "big_new_n_2049:odd": ((1024, 9, 6, 9, 0, 1, 0, 152112, 0, 0), 5, 0,
        [('staged', 0, 1, 64, 1, 256, 8, 'osd0_colsw', 'lists', 0, 0, 0, 0, 0, 15, 0)]),
    "rare_tuned:m4": ((256, 7, 6, 9, 0, 0, 1, 52480, 0, 0), 3, 1,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 4, 15)]),
    "rare_lds1024:m4": ((1024, 5, 6, 6, 1, 0, 0, 73056, 0, 0), 3, 0,
        [('staged', 1, 0, 0, 0, 576, 8, 'osd0_cols', 'sorted', 12, 0, 119, 138, 790, 5, 24)]),
    "rare_tuned:odd": ((256, 7, 6, 9, 0, 0, 1, 52480, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 4, 15)]),
    "rare_lds1024:odd": ((1024, 5, 6, 6, 1, 0, 0, 73056, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 0, 576, 8, 'osd0_cols', 'sorted', 12, 0, 119, 138, 790, 5, 24)]),
    "rare_big:m4": ((1024, 9, 6, 9, 0, 1, 0, 91616, 0, 0), 6, 0,
        [('staged', 1, 1, 64, 0, 576, 8, 'osd0_colsw', 'renumbered', 0, 0, 0, 0, 0, 10, 0)]),
    "rare_big:odd": ((1024, 9, 6, 9, 0, 1, 0, 91616, 0, 0), 5, 0,
        [('staged', 1, 1, 64, 0, 576, 8, 'osd0_colsw', 'renumbered', 0, 0, 0, 0, 0, 10, 0)]),
    "gdg_serial_v64_4_4_2": ((64, 4, 4, 2, 0, 0, 0, 9424, 0, 1), 1, 0,
        [('own', 0, 0, 0, 1, 64, 8, None, None, 0, 0, 0, 0, 0, 1, 0)]),
    "gdg_items_v64_4_4_2": ((64, 4, 4, 2, 0, 0, 0, 9424, 1, 1), 2, 0,
        [('own', 0, 0, 0, 1, 64, 8, None, None, 0, 0, 0, 0, 0, 1, 0)]),
    "gd_v64_4_4_2": ((64, 4, 4, 2, 0, 0, 0, 9424, 0, 1), 1, 0,
        [('own', 0, 0, 0, 1, 64, 8, None, None, 0, 0, 0, 0, 0, 1, 0)]),
    "ens_v64_4_4_2": ((64, 4, 4, 2, 0, 0, 0, 9424, 0, 1), 7, 0,
        [('own', 0, 0, 0, 1, 64, 8, None, None, 0, 0, 0, 0, 0, 1, 0)]),
    "gdg_serial_v64_4_8_16": ((64, 4, 8, 16, 0, 0, 0, 17088, 0, 1), 1, 0,
        [('own', 0, 0, 0, 0, 64, 8, None, None, 0, 0, 0, 0, 0, 1, 0)]),
    "gdg_items_v64_4_8_16": ((64, 4, 8, 16, 0, 0, 0, 17088, 1, 1), 2, 0,
        [('own', 0, 0, 0, 0, 64, 8, None, None, 0, 0, 0, 0, 0, 1, 0)]),
    "gd_v64_4_8_16": ((64, 4, 8, 16, 0, 0, 0, 17088, 0, 1), 1, 0,
        [('own', 0, 0, 0, 0, 64, 8, None, None, 0, 0, 0, 0, 0, 1, 0)]),
    "ens_v64_4_8_16": ((64, 4, 8, 16, 0, 0, 0, 17088, 0, 1), 7, 0,
        [('own', 0, 0, 0, 0, 64, 8, None, None, 0, 0, 0, 0, 0, 1, 0)]),
    "gdg_serial_v256_2_8_16": ((256, 2, 8, 16, 0, 0, 0, 36128, 0, 1), 1, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "gdg_items_v256_2_8_16": ((256, 2, 8, 16, 0, 0, 0, 36128, 1, 1), 2, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "gd_v256_2_8_16": ((256, 2, 8, 16, 0, 0, 0, 36128, 0, 1), 1, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "ens_v256_2_8_16": ((256, 2, 8, 16, 0, 0, 0, 36128, 0, 1), 7, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "gdg_serial_v256_4_8_16": ((256, 4, 8, 16, 0, 0, 0, 46320, 0, 1), 1, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "gdg_items_v256_4_8_16": ((256, 4, 8, 16, 0, 0, 0, 46320, 1, 1), 2, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "gd_v256_4_8_16": ((256, 4, 8, 16, 0, 0, 0, 46320, 0, 1), 1, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "ens_v256_4_8_16": ((256, 4, 8, 16, 0, 0, 0, 46320, 0, 1), 7, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "gdg_serial_v256_2_10_12": ((256, 2, 10, 12, 0, 0, 0, 30832, 0, 1), 1, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "gdg_items_v256_2_10_12": ((256, 2, 10, 12, 0, 0, 0, 30832, 1, 1), 2, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "gd_v256_2_10_12": ((256, 2, 10, 12, 0, 0, 0, 30832, 0, 1), 1, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "ens_v256_2_10_12": ((256, 2, 10, 12, 0, 0, 0, 30832, 0, 1), 7, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 2, 0)]),
    "gdg_serial_v256_7_6_9_depth": ((256, 7, 6, 9, 0, 0, 0, 54928, 0, 1), 1, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 3, 0)]),
    "gdg_items_v256_7_6_9_depth": ((256, 7, 6, 9, 0, 0, 0, 54928, 1, 1), 2, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 3, 0)]),
    "gd_v256_7_6_9_depth": ((256, 7, 6, 9, 0, 0, 0, 54928, 0, 1), 1, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 3, 0)]),
    "ens_v256_7_6_9_depth": ((256, 7, 6, 9, 0, 0, 0, 54928, 0, 1), 7, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 3, 0)]),
    "gdg_serial_v256_7_8_16": ((256, 7, 8, 16, 0, 0, 0, 62400, 0, 1), 1, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 3, 0)]),
    "gdg_items_v256_7_8_16": ((256, 7, 8, 16, 0, 0, 0, 62400, 1, 1), 2, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 3, 0)]),
    "gd_v256_7_8_16": ((256, 7, 8, 16, 0, 0, 0, 62400, 0, 1), 1, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 3, 0)]),
    "ens_v256_7_8_16": ((256, 7, 8, 16, 0, 0, 0, 62400, 0, 1), 7, 0,
        [('own', 0, 0, 0, 0, 256, 8, None, None, 0, 0, 0, 0, 0, 3, 0)]),
    "gdg_serial_g1024_5_6_9": ((1024, 5, 6, 9, 0, 0, 0, 95024, 0, 1), 1, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 5, 0)]),
    "gd_g1024_5_6_9": ((1024, 5, 6, 9, 0, 0, 0, 95024, 0, 1), 1, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 5, 0)]),
    "ens_g1024_5_6_9": ((1024, 5, 6, 9, 0, 0, 0, 95024, 0, 1), 7, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 5, 0)]),
    "gdg_serial_v1024_3_10_12": ((1024, 3, 10, 12, 0, 0, 0, 104224, 0, 1), 1, 0,
        [('own', 0, 0, 0, 0, 576, 8, None, None, 0, 0, 0, 0, 0, 5, 0)]),
    "gd_v1024_3_10_12": ((1024, 3, 10, 12, 0, 0, 0, 104224, 0, 1), 1, 0,
        [('own', 0, 0, 0, 0, 576, 8, None, None, 0, 0, 0, 0, 0, 5, 0)]),
    "ens_v1024_3_10_12": ((1024, 3, 10, 12, 0, 0, 0, 104224, 0, 1), 7, 0,
        [('own', 0, 0, 0, 0, 576, 8, None, None, 0, 0, 0, 0, 0, 5, 0)]),
    "gdg_serial_g1024_8_8_16": ((1024, 8, 8, 16, 0, 0, 0, 112928, 0, 1), 1, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 5, 0)]),
    "gd_g1024_8_8_16": ((1024, 8, 8, 16, 0, 0, 0, 112928, 0, 1), 1, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 5, 0)]),
    "ens_g1024_8_8_16": ((1024, 8, 8, 16, 0, 0, 0, 112928, 0, 1), 7, 0,
        [('own', 0, 0, 0, 1, 256, 8, None, None, 0, 0, 0, 0, 0, 5, 0)]),
    "gdg_serial_big_9_6_9": ((1024, 9, 6, 9, 0, 1, 0, 79568, 0, 1), 8, 0,
        [('own', 0, 0, 0, 0, 512, 8, None, None, 0, 0, 0, 0, 0, 10, 0)]),
    "gd_big_9_6_9": ((1024, 9, 6, 9, 0, 1, 0, 79568, 0, 1), 8, 0,
        [('own', 0, 0, 0, 0, 512, 8, None, None, 0, 0, 0, 0, 0, 10, 0)]),
    "ens_big_9_6_9": ((1024, 9, 6, 9, 0, 1, 0, 79568, 0, 1), 9, 0,
        [('own', 0, 0, 0, 0, 512, 8, None, None, 0, 0, 0, 0, 0, 10, 0)]),
    "gdg_serial_bigwave_m256": ((1024, 9, 10, 16, 0, 1, 0, 67472, 0, 1), 8, 0,
        [('own', 0, 0, 0, 0, 1024, 8, None, None, 0, 0, 0, 0, 0, 4, 0)]),
    "gd_bigwave_m256": ((1024, 9, 10, 16, 0, 1, 0, 67472, 0, 1), 8, 0,
        [('own', 0, 0, 0, 0, 1024, 8, None, None, 0, 0, 0, 0, 0, 4, 0)]),
    "ens_bigwave_m256": ((1024, 9, 10, 16, 0, 1, 0, 67472, 0, 1), 9, 0,
        [('own', 0, 0, 0, 0, 1024, 8, None, None, 0, 0, 0, 0, 0, 4, 0)]),
    "gdg_depth2_off_tuned": ((64, 4, 8, 16, 0, 0, 0, 17600, 0, 0), 1, 0,
        [('own', 0, 0, 0, 0, 64, 8, None, None, 0, 0, 0, 0, 0, 1, 0)]),
    "gdg_depth2_off_lds1024": ((1024, 3, 10, 12, 0, 0, 0, 116928, 0, 0), 1, 0,
        [('own', 0, 0, 0, 0, 512, 8, None, None, 0, 0, 0, 0, 0, 5, 0)]),
    "pipe_joint_maxima": ((256, 4, 8, 16, 0, 0, 0, 29952, 0, 0), 0, 0,
        [('staged', 1, 0, 0, 1, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 4, 39),
         ('staged', 1, 0, 0, 0, 256, 6, 'osd0_quad', 'sorted', 0, 0, 0, 0, 0, 2, 26)]),
    "pipe_one_window_big": ((1024, 9, 6, 9, 0, 1, 0, 92816, 0, 0), 6, 0,
        [('staged', 1, 1, 0, 1, 256, 8, 'osd0_wave_reg', 'renumbered', 0, 0, 0, 0, 0, 2, 0),
         ('staged', 1, 1, 64, 0, 512, 8, 'osd0_colsw', 'renumbered', 0, 0, 0, 0, 0, 10, 0)]),
}
