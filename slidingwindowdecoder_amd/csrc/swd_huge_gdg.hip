// The guessing decoders on graphs beyond every kernel variant (more than 1024 checks, 9216 columns, row weight 64, column weight
// 10 or new_n > 2048): bpgdg_decoder (single-thread gdg() and the threaded ensemble), bpgd_decoder and bp_history_decoder of
// /root/reference/src/bp_guessing_decoder.pyx with the BPGD engine of src/include/bpgd.cpp -- the reference has no size limit
// (src/include/mod2sparse.c:52-80).  The form of swd_huge.hip: one 1024-thread workgroup per shot slot, a grid of at most one
// workgroup per CU that loops over the batch, every array in the slot's slice of an HBM buffer, LDS only for scans and reductions.
// A shot lives and dies in one workgroup.  Phases, each bit-exact with the test oracle (its routines in parentheses):
//   pre-processing BP with the 4-slot history        bp_guessing_decoder.pyx:48-139        (swo_gdg_decode, gdg_bp)
//   stable argsort of ((h0 + h1) + h2) + h3           pyx:259-271                           (index_sort)
//   BPGD::reset on the first new_n sorted columns     bpgd.cpp:199-239                      (bpgd_reset)
//   gdg() / gd() / the threaded ensemble               pyx:254-338, 517-560, bpgd.cpp:419-688 (gdg_run, gd_run, gdg_multi_run)
// The columns keep their full-graph ids: pos[x] is a column's place in the sorted order, the columns past new_n carry vn = -2
// (never live, decision 0), and the sub-matrix of BPGD::reset is a per-shot CSR of its edges over those ids (srp / sci; messages
// per sub edge).  Scans the reference runs "for vn in range(new_n)" run over positions.  Every step of one hypothesis depends on the previous one, so the hypotheses run one after another in the
// oracle's order; the work inside a step (check / node passes, the selection scan, peeling rounds) is spread over the block.
#include <math.h>
#include <string.h>

#include <memory>

#include "swd_huge_common.h"

namespace swd {

struct SwdHugeGdgArgs {
    HugeGraphDev g;
    const int32_t *r2c;                    // CSR edge -> CSC position
    int32_t E, new_n, npad, B;
    int32_t mode, ens;                     // mode 0 bpgdg, 1 bpgd, 2 bp_history; ens: the threaded ensemble (multi_thread=True)
    int32_t pre_iter, mips, max_step, D, S, tree_step, side_step, low_error, max_guess, NS;
    double alpha, factor;
    HugeIo io;
    int64_t rec;                           // bytes of one snapshot: vn by position (new_n), check values (m), check degrees (4 m)
    // offsets inside a slot's scratch slice
    int64_t o_b2c, o_c2b, o_hist, o_post, o_key, o_idx, o_pos, o_vn, o_hard, o_bph, o_dec, o_cnval, o_cndeg, o_tsyn, o_tmp, o_lc,
        o_lv, o_bvn, o_bh, o_bcv, o_bcd, o_best, o_merr, o_meta, o_snap, o_srp, o_sci, o_sc2r;
};

struct HgView {
    double *b2c, *c2b, *hist, *post;
    uint64_t *key;
    int32_t *idx, *pos, *vn, *cnval, *cndeg, *tmp, *lc, *lv, *bvn, *bcv, *bcd, *meta;
    int32_t *srp, *sci, *sc2r; // the sub-matrix of BPGD::reset: CSR over its columns (full ids), CSC position -> sub edge
    uint8_t *hard, *bph, *tsyn, *bh, *best, *merr, *snap;
    int8_t *dec;
};

// snapshot metadata: decision value, decision column, alternative depth, status per slot
struct HgMeta {
    int32_t *val, *col, *depth, *status;
};

static constexpr int HG_NONE = 0x7FFFFFFF;

// lexicographic block minimum of (key, j); j = -1: no candidate
__device__ __forceinline__ void hg_argmin(uint64_t &key, int &j, HugeLds &s) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t ok = (uint64_t)__shfl_xor((long long)key, o, 64);
        const int oj = __shfl_xor(j, o, 64);
        if (oj >= 0 && (j < 0 || ok < key || (ok == key && oj < j))) { key = ok; j = oj; }
    }
    __syncthreads();
    if (lane == 0) { s.red[w] = key; s.redi[w] = j; }
    __syncthreads();
    key = ~0ull; j = -1;
    for (int q = 0; q < HNT / 64; ++q) {
        const uint64_t ok = s.red[q];
        const int oj = s.redi[q];
        if (oj >= 0 && (j < 0 || ok < key || (ok == key && oj < j))) { key = ok; j = oj; }
    }
    __syncthreads();
}

__device__ __forceinline__ double hg_key2f(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// BPGD::vn_set_value (bpgd.cpp:51-80) by ONE thread
// (not huge_set_value of swd_huge.hip: osd_window.pyx:340-368 skips a check that is already met, this one fails on it or on degree 0)
__device__ int hg_set_value(const SwdHugeGdgArgs &a, const HgView &v, int x, int value) {
    if (v.vn[x] != -1) return (v.vn[x] == value) ? 0 : -1;
    v.vn[x] = value;
    v.hard[x] = (uint8_t)value;
    for (int k = a.g.col_ptr[x]; k < a.g.col_ptr[x + 1]; ++k) {
        const int c = a.g.row_idx[k];
        if (v.cnval[c] == -1 || v.cndeg[c] == 0) return -1;
        const int deg = v.cndeg[c] - 1;
        if (value) v.cnval[c] = 1 - v.cnval[c];
        v.cndeg[c] = deg;
        if (deg == 0) {
            if (v.cnval[c] != 0) return -1;
            v.cnval[c] = -1;
        }
    }
    return 0;
}

// vn_set_value of one column by the whole block (thread 0 works); returns 0 / -1
__device__ int hg_set1(const SwdHugeGdgArgs &a, const HgView &v, int x, int value, HugeLds &s) {
    __syncthreads();
    if (threadIdx.x == 0) s.flag[2] = hg_set_value(a, v, x, value);
    __syncthreads();
    const int rc = s.flag[2];
    __syncthreads();
    return rc;
}

// BPGD::peel (bpgd.cpp:13-49).  Parallel rounds: the closure does not depend on the order unless a contradiction appears.  Only the
// main branch of a shot uses the decisions a failed peel leaves behind (its vector is the answer when nothing converges); there
// (`exact`) the state before the peel is restored and thread 0 replays the reference's sweep to the point where it stops.  Returns
// 0 / -1.  (Not the peel of swd_huge.hip: this one walks the per-shot sub-matrix, with BPGD's failure rules and the event-driven replay.)
__device__ int hg_peel(const SwdHugeGdgArgs &a, const HgView &v, HugeLds &s, bool exact) {
    const int tid = threadIdx.x, m = a.g.m;
    bool any = false;
    for (int c = tid; c < m; c += HNT) if (v.cnval[c] != -1 && v.cndeg[c] < 2) any = true;
    if (!huge_any(any, s)) return 0;
    if (exact) {
        for (int j = tid; j < a.new_n; j += HNT) { const int x = v.idx[j]; v.bvn[x] = v.vn[x]; v.bh[x] = v.hard[x]; }
        for (int c = tid; c < m; c += HNT) { v.bcv[c] = v.cnval[c]; v.bcd[c] = v.cndeg[c]; }
        __syncthreads();
    }
    bool contra = false;
    for (;;) {
        bool work = false, bad = false;
        for (int c = tid; c < m; c += HNT) {
            v.tmp[c] = -1;
            if (v.cnval[c] == -1 || v.cndeg[c] >= 2) continue;
            work = true;
            if (v.cndeg[c] <= 0) { bad = true; continue; } // (not in a consistent state: the sweep below decides)
            int x = -1;
            for (int e = v.srp[c]; e < v.srp[c + 1]; ++e) if (v.vn[v.sci[e]] == -1) { x = v.sci[e]; break; }
            if (x < 0) { bad = true; continue; }
            v.tmp[c] = x; // proposal: node x takes the check's residual value
        }
        __syncthreads();
        // a node proposed by several checks takes the value of the lowest check (the first in the reference's sweep); the others
        // see their degree reach 0 in the update below and are met or contradicted like in the serial order
        for (int c = tid; c < m; c += HNT) {
            const int x = v.tmp[c];
            if (x < 0) continue;
            bool first = true;
            for (int k = a.g.col_ptr[x]; k < a.g.col_ptr[x + 1]; ++k) { const int c2 = a.g.row_idx[k]; if (c2 < c && v.tmp[c2] == x) { first = false; break; } }
            if (first) { v.vn[x] = v.cnval[c]; v.hard[x] = (uint8_t)v.cnval[c]; v.dec[x] = (int8_t)v.cnval[c]; }
        }
        __syncthreads();
        for (int c = tid; c < m; c += HNT) {
            if (v.cnval[c] == -1) continue;
            int cnt = 0, flip = 0;
            for (int e = v.srp[c]; e < v.srp[c + 1]; ++e) { const int d = v.dec[v.sci[e]]; if (d >= 0) { ++cnt; flip ^= d; } }
            if (!cnt) continue;
            const int d = v.cndeg[c] - cnt, val = v.cnval[c] ^ flip;
            v.cndeg[c] = d;
            if (d == 0) { if (val != 0) bad = true; v.cnval[c] = -1; } else v.cnval[c] = val;
        }
        __syncthreads();
        for (int c = tid; c < m; c += HNT) { const int x = v.tmp[c]; if (x >= 0) v.dec[x] = -1; }
        contra = huge_any(bad, s);
        if (contra) break;
        if (!huge_any(work, s)) break;
    }
    if (!contra) return 0;
    if (!exact) return -1; // (the branch ends here; its state is overwritten before anything reads it)
    for (int j = tid; j < a.new_n; j += HNT) { const int x = v.idx[j]; v.vn[x] = v.bvn[x]; v.hard[x] = v.bh[x]; }
    for (int c = tid; c < m; c += HNT) { v.cnval[c] = v.bcv[c]; v.cndeg[c] = v.bcd[c]; }
    // the reference's sweep, event driven: a pass visits the checks in ascending order that are live with degree < 2 when it gets
    // there -- those of the bit set `cur` (degree 1 at the start of the pass, or reached by a decision at a lower check of the same
    // pass); a check a decision brings to degree 1 behind the sweep's position waits in `nxt` for the next pass
    unsigned long long *cur = s.y, *nxt = s.y + 64;
    for (int w = tid; w < 128; w += HNT) s.y[w] = 0ull;
    __syncthreads();
    for (int c = tid; c < m; c += HNT) if (v.cnval[c] != -1 && v.cndeg[c] < 2) atomicOr(&cur[c >> 6], 1ull << (c & 63));
    __syncthreads();
    if (tid == 0) {
        const int wm = (m + 63) >> 6;
        int rc = 0;
        for (;;) {
            bool work = false;
            for (int w = 0; w < wm && rc == 0;) {
                if (!cur[w]) { ++w; continue; }
                const int c = (w << 6) + __ffsll((long long)cur[w]) - 1;
                cur[w] &= cur[w] - 1;
                if (v.cnval[c] == -1 || v.cndeg[c] >= 2) continue;
                if (v.cndeg[c] <= 0) { v.cnval[c] = -1; continue; }
                work = true;
                int x = -1;
                for (int e = v.srp[c]; e < v.srp[c + 1]; ++e) if (v.vn[v.sci[e]] == -1) { x = v.sci[e]; break; }
                if (x < 0) { rc = -1; break; }
                const int value = v.cnval[c];
                v.vn[x] = value; v.hard[x] = (uint8_t)value; // vn_set_value (bpgd.cpp:51-80) on a live node
                for (int k = a.g.col_ptr[x]; k < a.g.col_ptr[x + 1]; ++k) {
                    const int c2 = a.g.row_idx[k];
                    if (v.cnval[c2] == -1 || v.cndeg[c2] == 0) { rc = -1; break; }
                    const int deg = v.cndeg[c2] - 1;
                    if (value) v.cnval[c2] = 1 - v.cnval[c2];
                    v.cndeg[c2] = deg;
                    if (deg == 0) {
                        if (v.cnval[c2] != 0) { rc = -1; break; }
                        v.cnval[c2] = -1;
                    } else if (deg == 1) (c2 > c ? cur : nxt)[c2 >> 6] |= 1ull << (c2 & 63);
                }
            }
            if (rc || !work) break;
            for (int w = 0; w < wm; ++w) { cur[w] = nxt[w]; nxt[w] = 0ull; }
        }
        s.flag[2] = rc;
    }
    __syncthreads();
    const int rc = s.flag[2];
    __syncthreads();
    return rc;
}

// bp_init (bpgd.cpp:82-95): the messages of every live node's edges = its prior
__device__ void hg_bp_init(const SwdHugeGdgArgs &a, const HgView &v) {
    for (int j = threadIdx.x; j < a.new_n; j += HNT) {
        const int x = v.idx[j];
        if (v.vn[x] != -1) continue;
        for (int k = a.g.col_ptr[x]; k < a.g.col_ptr[x + 1]; ++k) v.b2c[v.sc2r[k]] = a.g.llr[x];
    }
    __syncthreads();
}

// BPGD::min_sum_log (bpgd.cpp:97-197) on the sub-graph; returns converged, *it = iterations run
__device__ int hg_block(const SwdHugeGdgArgs &a, const HgView &v, const uint8_t *synd, HugeLds &s, int *it) {
    *it = 0;
    if (a.mips <= 0) return 0;
    const int nlc = huge_compact(a.g.m, v.lc, s, [&](int c) { return v.cnval[c] != -1; });
    const int nlv = huge_compact(a.g.n, v.lv, s, [&](int x) { return v.vn[x] == -1; });
    const HugeGraphDev sg{a.g.m, a.g.n, v.srp, v.sci, a.g.col_ptr, a.g.row_idx, v.sc2r, a.g.llr};
    return huge_minsum(sg, a.factor, v.b2c, v.c2b, v.post, v.hard, v.tsyn, v.vn, v.cnval, synd, a.mips, v.lc, nlc, v.lv, nlv, s, it);
}

// BPGD::get_pm (bpgd.cpp:250-256): prior LLRs of the set positions, added in position order
__device__ double hg_pm(const SwdHugeGdgArgs &a, const HgView &v, HugeLds &s) {
    const int cnt = huge_compact(a.new_n, v.lv, s, [&](int j) { return v.hard[v.idx[j]] != 0; });
    if (threadIdx.x == 0) {
        double pm = 0.0;
        for (int i = 0; i < cnt; ++i) pm += a.g.llr[v.idx[v.lv[i]]];
        s.red[0] = (unsigned long long)__double_as_longlong(pm);
    }
    __syncthreads();
    const double pm = __longlong_as_double((long long)s.red[0]);
    __syncthreads();
    return pm;
}

// error vector by position -> dst[new_n]
__device__ void hg_take_err(const SwdHugeGdgArgs &a, const HgView &v, uint8_t *dst) {
    for (int j = threadIdx.x; j < a.new_n; j += HNT) dst[j] = v.hard[v.idx[j]];
    __syncthreads();
}

// snapshot of the masks and degrees (vn_stack / cn_stack / cn_degree_stack, bp_guessing_decoder.pyx:431-435)
__device__ void hg_save(const SwdHugeGdgArgs &a, const HgView &v, int slot) {
    uint8_t *r = v.snap + (int64_t)slot * a.rec;
    int8_t *sv = (int8_t *)r, *sc = (int8_t *)(r + ((a.new_n + 15) & ~15));
    int32_t *sd = (int32_t *)(r + ((a.new_n + 15) & ~15) + ((a.g.m + 15) & ~15));
    for (int j = threadIdx.x; j < a.new_n; j += HNT) sv[j] = (int8_t)v.vn[v.idx[j]];
    for (int c = threadIdx.x; c < a.g.m; c += HNT) { sc[c] = (int8_t)v.cnval[c]; sd[c] = v.cndeg[c]; }
    __syncthreads();
}

// back to a snapshot: BPGD::set_masks (bpgd.cpp:241-248, error = vn_mask, then init()) when set_masks, the state BPGD::reset left
// (error 0 on the live nodes) otherwise
__device__ void hg_load(const SwdHugeGdgArgs &a, const HgView &v, int slot, bool set_masks) {
    const uint8_t *r = v.snap + (int64_t)slot * a.rec;
    const int8_t *sv = (const int8_t *)r, *sc = (const int8_t *)(r + ((a.new_n + 15) & ~15));
    const int32_t *sd = (const int32_t *)(r + ((a.new_n + 15) & ~15) + ((a.g.m + 15) & ~15));
    for (int j = threadIdx.x; j < a.new_n; j += HNT) {
        const int x = v.idx[j], q = sv[j];
        v.vn[x] = q;
        v.hard[x] = (uint8_t)(set_masks ? q : (q == -1 ? 0 : q));
    }
    for (int c = threadIdx.x; c < a.g.m; c += HNT) { v.cnval[c] = sc[c]; v.cndeg[c] = sd[c]; }
    __syncthreads();
    hg_bp_init(a, v);
}

// The selection step of a decimation: bpgdg_decoder.select_vn (bp_guessing_decoder.pyx:340-442) and BPGD::select_vn
// (bpgd.cpp:288-355) share it.  Every live position of column weight > 2 is classified from its own history and the check values
// alone (aggressive 0 / aggressive 1 / candidate), so the classification runs in parallel; the aggressive decimations are then
// applied as the sequential loop would apply them: the first one that fails is the one at the last position of a check all of whose
// live nodes are decimated here with a residual parity of 1, and the decisions before it (and its own) stay.  Then peel.  Returns
// -1 when a decimation or the peel fails, else 0 with *gcol (column or -1) and *favor of the smallest history sum (all-negative
// histories first).
__device__ int hg_select(const SwdHugeGdgArgs &a, const HgView &v, const uint8_t *synd, double A, double A_sum, int depth,
                         HugeLds &s, int *gcol, int *favor, bool exact) {
    const int tid = threadIdx.x, m = a.g.m, n = a.g.n;
    const double C = 30.0, D = 3.0;
    uint64_t k_all = ~0ull, k_neg = ~0ull;
    int j_all = -1, j_neg = -1;
    bool anydec = false;
    for (int j = tid; j < a.new_n; j += HNT) {
        const int x = v.idx[j];
        v.dec[x] = -1;
        if (v.vn[x] != -1) continue;
        const int k0 = a.g.col_ptr[x], k1 = a.g.col_ptr[x + 1];
        if (k1 - k0 <= 2) continue;
        int num_flip = 0;
        for (int k = k0; k < k1; ++k) {
            const int c = a.g.row_idx[k];
            if (v.cnval[c] == -1) continue;
            if ((synd[c] ? 1 : 0) != v.tsyn[c]) num_flip++;
        }
        bool all_smaller_than_A = true, all_negative = true, all_larger_than_C = true, all_larger_than_D = true;
        double history_sum = 0.0;
        for (int i = 0; i < 4; ++i) {
            const double llr = v.post[(size_t)i * n + x];
            history_sum += llr;
            if (llr < C) all_larger_than_C = false;
            if (llr < D) all_larger_than_D = false;
            if (llr > A) all_smaller_than_A = false;
            if (llr > 0.0) all_negative = false;
        }
        if (!a.low_error && all_larger_than_C && depth < 4) { v.dec[x] = 0; anydec = true; }
        else if (!a.low_error && num_flip >= 3 && all_larger_than_D) { v.dec[x] = 0; anydec = true; }
        else if (!a.low_error && all_smaller_than_A && history_sum < A_sum) { v.dec[x] = 1; anydec = true; }
        else if (history_sum < 10000.0) {
            const uint64_t key = huge_f2key(history_sum);
            if (j_all < 0 || key < k_all) { k_all = key; j_all = j; } // (ascending j per thread: strict < keeps the earliest)
            if (all_negative && (j_neg < 0 || key < k_neg)) { k_neg = key; j_neg = j; }
        }
    }
    if (huge_any(anydec, s)) {
        if (tid == 0) s.flag[1] = HG_NONE;
        __syncthreads();
        for (int c = tid; c < m; c += HNT) {
            if (v.cnval[c] == -1) continue;
            int cnt = 0, flip = 0, last = -1;
            for (int e = v.srp[c]; e < v.srp[c + 1]; ++e) {
                const int x = v.sci[e], d = v.dec[x];
                if (d >= 0) { ++cnt; flip ^= d; last = max(last, v.pos[x]); }
            }
            if (cnt > 0 && cnt == v.cndeg[c] && (v.cnval[c] ^ flip) != 0) atomicMin(&s.flag[1], last);
        }
        __syncthreads();
        const int fail_at = s.flag[1];
        __syncthreads();
        if (fail_at != HG_NONE) {
            for (int j = tid; j < a.new_n; j += HNT) {
                const int x = v.idx[j];
                if (j <= fail_at && v.dec[x] >= 0) { v.vn[x] = v.dec[x]; v.hard[x] = (uint8_t)v.dec[x]; }
                v.dec[x] = -1;
            }
            __syncthreads();
            return -1;
        }
        for (int c = tid; c < m; c += HNT) {
            if (v.cnval[c] == -1) continue;
            int cnt = 0, flip = 0;
            for (int e = v.srp[c]; e < v.srp[c + 1]; ++e) { const int d = v.dec[v.sci[e]]; if (d >= 0) { ++cnt; flip ^= d; } }
            if (!cnt) continue;
            const int d = v.cndeg[c] - cnt;
            v.cndeg[c] = d;
            v.cnval[c] = (d == 0) ? -1 : (v.cnval[c] ^ flip); // (no failure: a check that reaches degree 0 is met)
        }
        __syncthreads();
        for (int j = tid; j < a.new_n; j += HNT) { const int x = v.idx[j]; if (v.dec[x] >= 0) { v.vn[x] = v.dec[x]; v.hard[x] = (uint8_t)v.dec[x]; v.dec[x] = -1; } }
        __syncthreads();
    }
    hg_argmin(k_all, j_all, s);
    hg_argmin(k_neg, j_neg, s);
    if (hg_peel(a, v, s, exact) == -1) return -1;
    if (j_neg >= 0) { *gcol = v.idx[j_neg]; *favor = 1; }
    else { *gcol = j_all >= 0 ? v.idx[j_all] : -1; *favor = (j_all >= 0 && !(hg_key2f(k_all) > 0)) ? 1 : 0; }
    return 0;
}

// BPGD::decimate_vn_reliable (bpgd.cpp:258-286): the live position of largest |history slot 3| (strict >, the earliest wins)
__device__ int hg_reliable(const SwdHugeGdgArgs &a, const HgView &v, HugeLds &s) {
    uint64_t key = ~0ull;
    int jb = -1;
    for (int j = threadIdx.x; j < a.new_n; j += HNT) {
        const int x = v.idx[j];
        if (v.vn[x] != -1) continue;
        const double h = fabs(v.post[3 * (size_t)a.g.n + x]);
        if (!(h > 0.0)) continue;
        const uint64_t k = ~huge_f2key(h); // largest first
        if (jb < 0 || k < key) { key = k; jb = j; }
    }
    hg_argmin(key, jb, s);
    if (jb < 0) return -1;
    const int x = v.idx[jb];
    const int val = (v.post[3 * (size_t)a.g.n + x] > 0) ? 0 : 1;
    if (hg_set1(a, v, x, val, s) == -1) return -1;
    return hg_peel(a, v, s, true);
}

// the oracle's ens_offer: strict < against the best so far, ties with a different vector counted
__device__ void hg_offer(const SwdHugeGdgArgs &a, const HgView &v, HugeLds &s, int who, double pm, double &best, int &winner, int &ties) {
    if (pm < best) {
        best = pm; winner = who; ties = 0;
        hg_take_err(a, v, v.best);
    } else if (pm == best) {
        bool diff = false;
        for (int j = threadIdx.x; j < a.new_n; j += HNT) if (v.best[j] != v.hard[v.idx[j]]) diff = true;
        if (huge_any(diff, s)) ++ties;
    }
}

__global__ void __launch_bounds__(HNT) huge_gdg_kernel(const SwdHugeGdgArgs a) {
    __shared__ HugeLds s;
    const int tid = threadIdx.x, m = a.g.m, n = a.g.n, new_n = a.new_n;
    uint8_t *base = a.io.scratch + (int64_t)blockIdx.x * a.io.scratch_stride;
    HgView v;
    v.b2c = (double *)(base + a.o_b2c); v.c2b = (double *)(base + a.o_c2b); v.hist = (double *)(base + a.o_hist);
    v.post = (double *)(base + a.o_post); v.key = (uint64_t *)(base + a.o_key); v.idx = (int32_t *)(base + a.o_idx);
    v.pos = (int32_t *)(base + a.o_pos); v.vn = (int32_t *)(base + a.o_vn); v.hard = base + a.o_hard; v.bph = base + a.o_bph;
    v.dec = (int8_t *)(base + a.o_dec); v.cnval = (int32_t *)(base + a.o_cnval); v.cndeg = (int32_t *)(base + a.o_cndeg);
    v.tsyn = base + a.o_tsyn; v.tmp = (int32_t *)(base + a.o_tmp); v.lc = (int32_t *)(base + a.o_lc); v.lv = (int32_t *)(base + a.o_lv);
    v.bvn = (int32_t *)(base + a.o_bvn); v.bh = base + a.o_bh; v.bcv = (int32_t *)(base + a.o_bcv); v.bcd = (int32_t *)(base + a.o_bcd);
    v.best = base + a.o_best; v.merr = base + a.o_merr; v.meta = (int32_t *)(base + a.o_meta); v.snap = base + a.o_snap;
    v.srp = (int32_t *)(base + a.o_srp); v.sci = (int32_t *)(base + a.o_sci); v.sc2r = (int32_t *)(base + a.o_sc2r);
    const int nslots = a.ens ? a.NS + 2 : a.max_guess;
    const HgMeta M{v.meta, v.meta + nslots, v.meta + 2 * nslots, v.meta + 3 * nslots};
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const uint8_t *synd = a.io.synd + (int64_t)b * a.io.synd_stride;
        uint8_t *out = a.io.out + (int64_t)b * a.io.out_stride;
        double *hio = a.io.hist ? a.io.hist + (int64_t)b * 4 * n : nullptr;
        __syncthreads();
        // ---- bp_history_decoder.bp_decode_llr (bp_guessing_decoder.pyx:48-139): every node and check live, sign seed = syndrome
        huge_shot_reset(a.g, a.E, synd, a.io.hist_is_state ? hio : nullptr, v.cnval, nullptr, v.lc, v.vn, v.hard, v.lv, v.hist, v.b2c);
        for (int c = tid; c < m; c += HNT) v.tsyn[c] = 0;
        for (int x = tid; x < n; x += HNT) v.dec[x] = -1;
        for (int i = tid; i < 4 * n; i += HNT) v.post[i] = 0.0;
        __syncthreads();
        int it_pre = 0, it_post = 0, exit_class = -1, conv = 0;
        int w4 = n, w5 = m, w6 = a.E, w7 = 0; // statistics words 4-7 of the exits without a decimation tree
        double min_pm = 0.0;
        conv = huge_minsum(a.g, a.alpha, v.b2c, v.c2b, v.hist, v.hard, nullptr, v.vn, v.cnval, synd, a.pre_iter, v.lc, m, v.lv, n, s, &it_pre);
        if (conv) exit_class = SWD_EXIT_PRE;
        else if (a.mode == 2) exit_class = SWD_EXIT_NO_OSD;
        const uint8_t *ret = v.hard; // over columns
        if (exit_class < 0) {
            // ---- order by the summed history (pyx:259-271), BPGD::reset on the first new_n sorted columns (bpgd.cpp:199-239)
            for (int x = tid; x < n; x += HNT) v.bph[x] = v.hard[x];
            huge_history_order(v.hist, n, a.npad, nullptr, v.key, v.idx);
            for (int i = tid; i < n; i += HNT) {
                const int x = v.idx[i];
                v.pos[x] = i;
                v.vn[x] = (i < new_n) ? -1 : -2;
                v.hard[x] = 0;
                if (i >= new_n) v.bph[x] = 0; // bp_decoding[cols[new_n:]] = 0 (pyx:271)
            }
            __syncthreads();
            {   // the sub-matrix (mod2sparse_copycols, bpgd.cpp:200-202) as a CSR of its edges; every row stays, so a column's CSC is
                // the full graph's with its positions mapped to sub edges
                const int ch = (m + HNT - 1) / HNT, c0 = min(m, tid * ch), c1 = min(m, c0 + ch);
                int cnt = 0;
                for (int c = c0; c < c1; ++c) {
                    int d = 0;
                    for (int e = a.g.row_ptr[c]; e < a.g.row_ptr[c + 1]; ++e) d += (v.pos[a.g.col_idx[e]] < new_n) ? 1 : 0;
                    v.cnval[c] = (d == 0) ? -1 : (synd[c] ? 1 : 0);
                    v.cndeg[c] = d;
                    cnt += d;
                }
                int tot;
                int o = huge_scan(cnt, s, &tot);
                for (int c = c0; c < c1; ++c) {
                    v.srp[c] = o;
                    for (int e = a.g.row_ptr[c]; e < a.g.row_ptr[c + 1]; ++e) {
                        const int x = a.g.col_idx[e];
                        if (v.pos[x] < new_n) { v.sci[o] = x; v.sc2r[a.r2c[e]] = o; ++o; }
                    }
                }
                if (tid == 0) v.srp[m] = tot;
                __syncthreads();
            }
            if (hg_peel(a, v, s, false) == -1) {
                // BPGD::reset failed: gdg() / gd() return the BP vector with cols[new_n:] zeroed, the ensemble its zero-initialised
                // min_pm_error (bpgd.cpp:583, 619-625)
                exit_class = SWD_EXIT_FAIL_PEEL;
                for (int x = tid; x < n; x += HNT) v.hard[x] = a.ens ? 0 : v.bph[x];
                __syncthreads();
            }
        }
        if (exit_class < 0 && !a.ens) {
            hg_bp_init(a, v);
            // ---- gdg() phase 1 / gd(): the main branch (pyx:276-299, 525-544)
            int used_guess = 0, mcd = a.max_step, blocks = 0, it;
            double best = 10000.0;
            conv = 0;
            for (int depth = 0; depth < a.max_step; ++depth) {
                const int cv = hg_block(a, v, synd, s, &it);
                ++blocks; it_post += it;
                if (cv) {
                    conv = 1; mcd = depth;
                    best = hg_pm(a, v, s);
                    hg_take_err(a, v, v.best);
                    break;
                }
                int rc;
                if (a.mode == 0) {
                    int gcol = -1, fav = 0;
                    rc = hg_select(a, v, synd, -3.0, depth == 0 ? -16.0 : -12.0, depth, s, &gcol, &fav, true);
                    if (rc == 0) {
                        const bool guess = !(depth > mcd) && !(depth >= a.S);
                        if (guess && used_guess < a.max_guess) { // the snapshot (pyx:426-436)
                            if (tid == 0) { M.val[used_guess] = 1 - fav; M.col[used_guess] = gcol; M.depth[used_guess] = depth + 1; }
                            hg_save(a, v, used_guess);
                            ++used_guess;
                        }
                        rc = (gcol < 0) ? -1 : hg_set1(a, v, gcol, fav, s);
                        if (rc == 0) rc = hg_peel(a, v, s, true);
                    }
                } else rc = hg_reliable(a, v, s);
                if (rc == -1) break;
            }
            if (!conv) hg_take_err(a, v, v.best);
            // ---- gdg() phase 2: the snapshots in stack order (pyx:301-335)
            for (int i = 0; a.mode == 0 && i < used_guess; ++i) {
                __syncthreads();
                const int d0 = M.depth[i], gcol0 = M.col[i], val0 = M.val[i];
                if (d0 > mcd) continue;
                hg_load(a, v, i, true);
                if (gcol0 < 0 || hg_set1(a, v, gcol0, val0, s) == -1) continue;
                if (hg_peel(a, v, s, false) == -1) continue;
                for (int j = 0; j < a.side_step; ++j) {
                    const int depth = d0 + j;
                    const int cv = hg_block(a, v, synd, s, &it);
                    ++blocks; it_post += it;
                    if (cv) {
                        conv = 1;
                        const double pm = hg_pm(a, v, s);
                        if (pm < best) {
                            if (depth < mcd) mcd = depth;
                            hg_take_err(a, v, v.best);
                            best = pm;
                        }
                        break;
                    }
                    if (depth > mcd + 2) break;
                    int gcol = -1, fav = 0;
                    int rc = hg_select(a, v, synd, 0.0, -10.0, depth, s, &gcol, &fav, false);
                    if (rc == -1) break;
                    const bool guess = !(depth > mcd) && !(depth > a.D);
                    if (guess && used_guess < a.max_guess) {
                        if (tid == 0) { M.val[used_guess] = 1 - fav; M.col[used_guess] = gcol; M.depth[used_guess] = depth + 1; }
                        hg_save(a, v, used_guess);
                        ++used_guess;
                    }
                    if (gcol < 0 || hg_set1(a, v, gcol, fav, s) == -1 || hg_peel(a, v, s, false) == -1) break;
                }
            }
            __syncthreads();
            exit_class = SWD_EXIT_POST;
            min_pm = best;
            w4 = used_guess; w5 = blocks; w6 = mcd; w7 = 0;
        } else if (exit_class < 0) {
            // ---- the threaded ensemble (bpgd.cpp:419-688) in the oracle's order: main thread, tree threads by id, side threads
            const int Dp = a.D, S = a.S, T = (1 << Dp) - 1, NS = a.NS;
            const int R0 = NS, BK = NS + 1; // snapshot slots: side threads 0 .. NS-1, the state after reset, the tree thread's backup
            hg_save(a, v, R0);
            double best = 10000.0;
            int winner = -1, ties = 0, blocks = 0, it, sides = 0;
            bool main_converge = false;
            for (int j = tid; j < NS; j += HNT) M.status[j] = 0;
            __syncthreads();
            auto kill_sides = [&](int from) { // side_status[from:] = -1
                __syncthreads();
                for (int j = max(from, 0) + tid; j < NS; j += HNT) M.status[j] = -1;
                __syncthreads();
            };
            hg_bp_init(a, v);
            for (int depth = 0; depth < a.max_step; ++depth) { // main thread (:591-688)
                const int cv = hg_block(a, v, synd, s, &it);
                ++blocks; it_post += it;
                int gcol = -1, fav = 0;
                const int rc = hg_select(a, v, synd, -3.0, depth == 0 ? -16.0 : -12.0, depth, s, &gcol, &fav, true); // BEFORE the test (:630-633)
                if (cv || rc == -1 || gcol < 0) {
                    kill_sides(depth - Dp);
                    if (!cv) break;
                    main_converge = true;
                    hg_offer(a, v, s, 0, hg_pm(a, v, s), best, winner, ties);
                    break;
                }
                if (depth >= Dp && depth < S) {
                    const int j = depth - Dp;
                    hg_save(a, v, j);
                    if (tid == 0) { M.col[j] = gcol; M.val[j] = 1 - fav; M.depth[j] = depth + 1; M.status[j] = 1; }
                }
                if (hg_set1(a, v, gcol, fav, s) != -1 && hg_peel(a, v, s, true) != -1) continue;
                kill_sides(depth + 1 - Dp);
                break;
            }
            hg_take_err(a, v, v.merr);
            for (int id = 1; id <= T; ++id) { // tree threads (:435-525)
                hg_load(a, v, R0, false);
                bool on_side = false, saved = false, done = false;
                double A = -3.0, A_sum = -16.0, own_pm = 10000.0;
                int bk_col = -1, bk_val = 0;
                for (int depth = 0; depth < a.tree_step + Dp + 1; ++depth) {
                    if (depth > 0 && !on_side) A_sum = -12.0;
                    const int cv = hg_block(a, v, synd, s, &it);
                    ++blocks; it_post += it;
                    if (cv) { own_pm = hg_pm(a, v, s); hg_offer(a, v, s, id, own_pm, best, winner, ties); done = true; break; }
                    int gcol = -1, fav = 0;
                    if (hg_select(a, v, synd, A, A_sum, depth, s, &gcol, &fav, false) == -1 || gcol < 0) break;
                    if (depth < Dp) {
                        if ((id >> (Dp - 1 - depth)) & 1) { on_side = true; A = 0.0; A_sum = -10.0; fav = 1 - fav; }
                    } else if (depth == Dp) {
                        hg_save(a, v, BK);
                        bk_col = gcol; bk_val = 1 - fav; saved = true;
                    }
                    if (hg_set1(a, v, gcol, fav, s) == -1 || hg_peel(a, v, s, false) == -1) break;
                }
                if (done || !saved) continue;
                hg_load(a, v, BK, true);
                if (hg_set1(a, v, bk_col, bk_val, s) == -1 || hg_peel(a, v, s, false) == -1) continue;
                int depth = Dp + 1;
                for (int i = 0; i < a.tree_step; ++i) {
                    const int cv = hg_block(a, v, synd, s, &it);
                    ++blocks; it_post += it;
                    if (cv) {
                        const double pm = hg_pm(a, v, s);
                        if (!(pm > own_pm)) hg_offer(a, v, s, id, pm, best, winner, ties);
                        break;
                    }
                    int gcol = -1, fav = 0;
                    if (hg_select(a, v, synd, A, A_sum, depth, s, &gcol, &fav, false) == -1 || gcol < 0) break;
                    if (hg_set1(a, v, gcol, fav, s) == -1 || hg_peel(a, v, s, false) == -1) break;
                    ++depth;
                }
            }
            for (int j = 0; j < NS; ++j) { // side threads (:527-570): the handed-over masks, messages = priors
                __syncthreads();
                if (M.status[j] != 1) continue;
                ++sides;
                const int scol = M.col[j], sval = M.val[j];
                int depth = M.depth[j];
                hg_load(a, v, j, true);
                if (hg_set1(a, v, scol, sval, s) == -1 || hg_peel(a, v, s, false) == -1) continue;
                for (int i = 0; i < a.side_step; ++i) {
                    const int cv = hg_block(a, v, synd, s, &it);
                    ++blocks; it_post += it;
                    if (cv) { hg_offer(a, v, s, 1 + T + j, hg_pm(a, v, s), best, winner, ties); break; }
                    int gcol = -1, fav = 0;
                    if (hg_select(a, v, synd, 0.0, -10.0, depth, s, &gcol, &fav, false) == -1 || gcol < 0) break;
                    if (hg_set1(a, v, gcol, fav, s) == -1 || hg_peel(a, v, s, false) == -1) break;
                    ++depth;
                }
            }
            if (!main_converge && best > 10000.0 - 1.0) { // :677-682
                for (int j = tid; j < new_n; j += HNT) v.best[j] = v.merr[j];
                __syncthreads();
            }
            exit_class = SWD_EXIT_POST;
            conv = best < 9999.0;
            min_pm = best;
            w4 = 1 + T + sides; w5 = blocks; w6 = winner; w7 = ties;
        }
        if (exit_class == SWD_EXIT_POST) { // bp_decoding[cols[j]] = error[j] for j < new_n, 0 past new_n
            for (int j = tid; j < n; j += HNT) v.hard[v.idx[j]] = (j < new_n) ? v.best[j] : 0;
            __syncthreads();
        }
        for (int x = tid; x < n; x += HNT) out[x] = ret[x];
        if (hio) for (int i = tid; i < 4 * n; i += HNT) hio[i] = v.hist[i];
        if (tid == 0) {
            if (a.io.stats) {
                int32_t *st = a.io.stats + (int64_t)b * SWD_STAT_WORDS;
                st[0] = exit_class | (conv ? SWD_STATUS_CONVERGE : 0);
                st[1] = it_pre + it_post; st[2] = it_pre; st[3] = it_post; st[4] = w4; st[5] = w5; st[6] = w6; st[7] = w7;
            }
            if (a.io.min_pm) a.io.min_pm[b] = min_pm;
        }
    }
}

struct HugeGdg : HugeHost {
    SwdHugeGdgArgs tmpl{};
    void launch(int32_t B, const HugeIo &io, uint8_t *, uint8_t *, int grid, hipStream_t st) override {
        SwdHugeGdgArgs a = tmpl;
        a.io = io; a.B = B;
        hipLaunchKernelGGL(huge_gdg_kernel, dim3(grid), dim3(HNT), 0, st, a);
    }
};

// builds the general form of the guessing decoders; NULL (with a message naming the bound) when it cannot take the graph
HugeIface *huge_gdg_create(const swd_graph_desc *g, const swd_gdg_params *p, int device) {
    if (HugeHost::check_desc(g)) return nullptr;
    const int m = g->m, n = g->n, E = g->nnz;
    if (m > 4096) { set_error(SWD_ERR_CAPACITY, "m=%d exceeds the guessing decoders' general form limit of 4096 checks", m); return nullptr; }
    if ((long long)n > (1 << 22)) { set_error(SWD_ERR_CAPACITY, "n=%d exceeds the guessing decoders' general form limit of 4194304 columns", n); return nullptr; }
    if (p->multi_thread == 2) {
        set_error(SWD_ERR_CAPACITY, "hypotheses= / multi_thread=2 needs a kernel variant, and none takes this graph (m=%d, n=%d) with these parameters: the "
                  "general form runs the reference's modes only", m, n);
        return nullptr;
    }
    const int D = p->max_tree_depth, S = p->max_side_depth;
    int max_guess = ((1 << D) - 1) * 2 + S - D; // bp_guessing_decoder.pyx:181
    if (max_guess < 1) max_guess = 1;
    const int NS = std::max(S - D, 0);
    const bool ens = p->mode == 0 && p->multi_thread == 1;
    const int nslots = p->mode == 0 ? (ens ? NS + 2 : max_guess) : 1;
    if (nslots > 4096) { set_error(SWD_ERR_CAPACITY, "%d snapshots per shot exceed the guessing decoders' general form limit of 4096", nslots); return nullptr; }
    std::unique_ptr<HugeGdg> h(new HugeGdg());
    SwdHugeGdgArgs &a = h->tmpl;
    CsrHost c;
    if (h->ingest(g, device, c, &a.g, &a.r2c)) return nullptr;
    // the reference keeps check degrees in char (bpgd.hpp:23, bpgd.cpp:204-223): from 128 on they wrap, no answer is pinned
    for (int r = 0; r < m && p->mode != 2; ++r)
        if (c.row_ptr[r + 1] - c.row_ptr[r] >= 128) {
            set_error(SWD_ERR_CAPACITY, "check %d has weight %d: the guessing decoders' general form takes check weights below 128 (the reference's "
                      "char check degrees wrap there)", r, c.row_ptr[r + 1] - c.row_ptr[r]);
            return nullptr;
        }
    h->new_n = (p->new_n <= 0) ? std::min(n, 2 * m) : std::min(p->new_n, n); // bp_guessing_decoder.pyx:186-189
    const int npad = h->npad;
    a.E = E; a.new_n = h->new_n; a.npad = npad;
    a.mode = p->mode; a.ens = ens ? 1 : 0;
    a.pre_iter = p->max_iter; a.mips = p->max_iter_per_step; a.max_step = p->max_step; a.D = D; a.S = S;
    a.tree_step = p->max_tree_branch_step; a.side_step = p->max_side_branch_step; a.low_error = p->low_error_mode ? 1 : 0;
    a.max_guess = max_guess; a.NS = NS;
    a.alpha = p->ms_scaling_factor; a.factor = p->gdg_factor;
    a.rec = (int64_t)HugeHost::al((size_t)((h->new_n + 15) & ~15) + (size_t)((m + 15) & ~15) + (size_t)m * 4);
    a.o_b2c = h->take((size_t)E * 8); a.o_c2b = h->take((size_t)E * 8); a.o_hist = h->take((size_t)4 * n * 8); a.o_post = h->take((size_t)4 * n * 8);
    a.o_key = h->take((size_t)npad * 8); a.o_idx = h->take((size_t)npad * 4); a.o_pos = h->take((size_t)n * 4); a.o_vn = h->take((size_t)n * 4);
    a.o_hard = h->take((size_t)n); a.o_bph = h->take((size_t)n); a.o_dec = h->take((size_t)n);
    a.o_cnval = h->take((size_t)m * 4); a.o_cndeg = h->take((size_t)m * 4); a.o_tsyn = h->take((size_t)m); a.o_tmp = h->take((size_t)m * 4);
    a.o_lc = h->take((size_t)m * 4); a.o_lv = h->take((size_t)n * 4);
    a.o_bvn = h->take((size_t)n * 4); a.o_bh = h->take((size_t)n); a.o_bcv = h->take((size_t)m * 4); a.o_bcd = h->take((size_t)m * 4);
    a.o_best = h->take((size_t)h->new_n); a.o_merr = h->take((size_t)h->new_n); a.o_meta = h->take((size_t)4 * nslots * 4);
    a.o_snap = h->take((size_t)nslots * (size_t)a.rec);
    a.o_srp = h->take((size_t)(m + 1) * 4); a.o_sci = h->take((size_t)E * 4); a.o_sc2r = h->take((size_t)E * 4);
    return h.release();
}

} // namespace swd
