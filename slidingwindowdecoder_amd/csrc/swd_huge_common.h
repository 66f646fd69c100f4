// What the general forms share (swd_huge.hip: osd_window, swd_huge_gdg.hip: the guessing decoders).  Device helpers: one 1024-thread
// workgroup per decode, every array in HBM, LDS only for block-wide scans and reductions.  Host side (at the end): the handle both
// forms derive from -- CSR ingest and upload, the scratch layout, the launch path.
#pragma once
#include <stdint.h>

#include <mutex>

#include <hip/hip_runtime.h>

#include "swd_plan.h"

namespace swd {

static constexpr int HNT = 1024;

__device__ __forceinline__ uint64_t huge_f2key(double x) {
    x = x + 0.0; // -0.0 -> +0.0: equal doubles get equal keys (the reference's stable sort compares with <)
    uint64_t u = (uint64_t)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

struct HugeLds {
    int scan[HNT / 64 + 1];
    int flag[4];
    unsigned long long red[HNT / 64];
    int redi[HNT / 64];
    unsigned long long y[64 * 16]; // reduced columns of a batch (wm <= 64 words each)
    int piv[16];
};

// exclusive prefix sum of one int per thread over the block; *total = sum.  Two barriers.
__device__ __forceinline__ int huge_scan(int x, HugeLds &s, int *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int v = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
    __syncthreads();
    if (lane == 63) s.scan[w] = v;
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < HNT / 64; ++i) { const int c = s.scan[i]; if (i < w) base += c; tot += c; }
    *total = tot;
    return base + v - x;
}

__device__ __forceinline__ bool huge_any(bool p, HugeLds &s) {
    __syncthreads();
    if (threadIdx.x == 0) s.flag[0] = 0;
    __syncthreads();
    if (p) s.flag[0] = 1;
    __syncthreads();
    return s.flag[0] != 0;
}

// indices i in [0, count) with pred(i), ascending, into list[]; returns how many (every thread a contiguous chunk)
template <class F>
__device__ __forceinline__ int huge_compact(int count, int32_t *list, HugeLds &s, F pred) {
    const int ch = (count + HNT - 1) / HNT, i0 = min(count, (int)threadIdx.x * ch), i1 = min(count, i0 + ch);
    int c = 0;
    for (int i = i0; i < i1; ++i) c += pred(i) ? 1 : 0;
    int tot;
    int o = huge_scan(c, s, &tot);
    for (int i = i0; i < i1; ++i) if (pred(i)) list[o++] = i;
    __syncthreads();
    return tot;
}

// sum of llr[v] over the listed nodes IN LIST ORDER (ascending v: "pm" sums of osd_window.pyx run over v ascending), by one thread
__device__ __forceinline__ double huge_ordered_sum(const int32_t *list, int cnt, const double *llr) {
    double pm = 0.0;
    for (int i = 0; i < cnt; ++i) pm += llr[list[i]];
    return pm;
}

// ascending bitonic sort of (key, idx) pairs, lexicographic = the reference's stable ascending argsort (bpgd.cpp:384-389)
__device__ inline void huge_sort(uint64_t *key, int32_t *idx, int npad) {
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < npad; i += HNT) {
                const int l = i ^ j;
                if (l > i) {
                    const uint64_t ki = key[i], kl = key[l];
                    const int32_t ii = idx[i], il = idx[l];
                    const bool up = (i & k) == 0;
                    const bool gt = ki > kl || (ki == kl && ii > il);
                    if (gt == up) { key[i] = kl; key[l] = ki; idx[i] = il; idx[l] = ii; }
                }
            }
            __syncthreads();
        }
}

// the check matrix in HBM: CSR (columns ascending inside a row), CSC (rows ascending inside a column), CSC position -> CSR edge
struct HugeGraphDev {
    int32_t m, n;
    const int32_t *row_ptr, *col_idx, *col_ptr, *row_idx, *c2r;
    const double *llr;
};

// what a launch adds to an argument template, next to B (which stays where each form had it: spill counts follow the layout)
struct HugeIo {
    const uint8_t *synd; int64_t synd_stride;
    uint8_t *out; int64_t out_stride;
    int32_t *stats; double *min_pm;
    double *hist; int32_t hist_is_state;     // nullable [B][4][n]
    uint8_t *scratch; int64_t scratch_stride; // a workgroup's slice: scratch + blockIdx.x * scratch_stride
};

// start of a shot in both forms: every check and node live (check value = syndrome bit, degree = row weight where cndeg is given),
// decisions 0, the 4-slot history from hist_in (a stateful caller's; null: zeros, a new reference object), messages = priors
// (bp_init).  No barrier.
__device__ __forceinline__ void huge_shot_reset(const HugeGraphDev &g, int E, const uint8_t *synd, const double *hist_in, int32_t *cnval,
                                                int32_t *cndeg, int32_t *lc, int32_t *vn, uint8_t *hard, int32_t *lv, double *hist, double *b2c) {
    const int tid = threadIdx.x;
    for (int c = tid; c < g.m; c += HNT) { cnval[c] = synd[c] ? 1 : 0; if (cndeg) cndeg[c] = g.row_ptr[c + 1] - g.row_ptr[c]; lc[c] = c; }
    for (int x = tid; x < g.n; x += HNT) { vn[x] = -1; hard[x] = 0; lv[x] = x; }
    for (int i = tid; i < 4 * g.n; i += HNT) hist[i] = hist_in ? hist_in[i] : 0.0;
    for (int e = tid; e < E; e += HNT) b2c[e] = g.llr[g.col_idx[e]];
}

// idx[] = the stable ascending argsort of the summed history ((h0 + h1) + h2) + h3 (osd_window.pyx:172, bp_guessing_decoder.pyx:
// 259-271), padded to npad.  With vn (the OSD's order, osd_window.pyx:205-215) a node decided 1 sorts as -1000, one decided 0 as +1000.
__device__ inline void huge_history_order(const double *hist, int n, int npad, const int32_t *vn, uint64_t *key, int32_t *idx) {
    const uint64_t kp = huge_f2key(1000.0), km = huge_f2key(-1000.0);
    for (int i = threadIdx.x; i < npad; i += HNT) {
        if (i < n) {
            const int st = vn ? vn[i] : -1;
            key[i] = st == 1 ? km : (st == 0 ? kp : huge_f2key(((hist[i] + hist[n + i]) + hist[2 * (size_t)n + i]) + hist[3 * (size_t)n + i]));
            idx[i] = i;
        } else { key[i] = ~0ull; idx[i] = 0x7FFFFFFF; }
    }
    __syncthreads();
    huge_sort(key, idx, npad);
}

// masked min-sum (osd_window.pyx:381-485 == bp_guessing_decoder.pyx:64-126 == bpgd.cpp:103-182): `iters` flooding iterations at
// most over the listed live checks / live nodes (nlc / nlv entries).  A node is live when vn[x] == -1, a check when cnval[c] != -1
// (its value seeds the sign).  Posterior of iteration `it` into hist[(it % 4) * n + x], decisions into hard[], the parity of every
// check of the FULL matrix into tsyn[] (nullable; the reference's temp_syndrome).  Returns 1 when H * hard == synd after an
// iteration; *done = iterations executed.
__device__ inline int huge_minsum(const HugeGraphDev &g, double alpha, double *b2c, double *c2b, double *hist, uint8_t *hard,
                                  uint8_t *tsyn, const int32_t *vn, const int32_t *cnval, const uint8_t *synd, int iters,
                                  const int32_t *lc, int nlc, const int32_t *lv, int nlv, HugeLds &s, int *done) {
    const int tid = threadIdx.x;
    *done = 0;
    for (int it = 0; it < iters; ++it) {
        // check pass: first and second minimum of the clipped magnitudes over the live edges, parity of the non-positive ones
        for (int q = tid; q < nlc; q += HNT) {
            const int c = lc[q];
            const int e0 = g.row_ptr[c], e1 = g.row_ptr[c + 1];
            double min1 = 1e308, min2 = 1e308;
            int arg = -1, neg = (cnval[c] == 1) ? 1 : 0;
            for (int e = e0; e < e1; ++e) {
                if (vn[g.col_idx[e]] != -1) continue;
                double x = b2c[e];
                x = (x > 50.0) ? 50.0 : ((x < -50.0) ? -50.0 : x);
                const double ax = fabs(x);
                if (ax < min1) { min2 = min1; min1 = ax; arg = e; }
                else if (ax < min2) min2 = ax;
                neg += (x <= 0) ? 1 : 0;
            }
            for (int e = e0; e < e1; ++e) {
                if (vn[g.col_idx[e]] != -1) continue;
                double x = b2c[e];
                const int sg = (neg - ((x <= 0) ? 1 : 0)) & 1; // (clipping keeps the sign)
                const double mag = (e == arg) ? min2 : min1;   // minimum over the OTHER live edges (none: the 1e308 sentinel)
                c2b[e] = mag * (sg ? -alpha : alpha);
            }
        }
        __syncthreads();
        // variable-node pass: prefix / suffix sums in row order, posterior into history slot it % 4
        double *hs = hist + (size_t)(it & 3) * g.n;
        for (int q = tid; q < nlv; q += HNT) {
            const int x = lv[q];
            const int k0 = g.col_ptr[x], k1 = g.col_ptr[x + 1];
            double temp = g.llr[x];
            for (int k = k0; k < k1; ++k) {
                if (cnval[g.row_idx[k]] == -1) continue;
                const int e = g.c2r[k];
                b2c[e] = temp;
                temp += c2b[e];
            }
            hs[x] = temp;
            hard[x] = (temp <= 0) ? 1 : 0;
            temp = 0.0;
            for (int k = k1 - 1; k >= k0; --k) {
                if (cnval[g.row_idx[k]] == -1) continue;
                const int e = g.c2r[k];
                b2c[e] += temp;
                temp += c2b[e];
            }
        }
        __syncthreads();
        // H * decision == syndrome over the FULL matrix (decided nodes included)
        bool bad = false;
        for (int c = tid; c < g.m; c += HNT) {
            int p = 0;
            for (int e = g.row_ptr[c]; e < g.row_ptr[c + 1]; ++e) p ^= hard[g.col_idx[e]];
            if (tsyn) tsyn[c] = (uint8_t)p;
            if (p != (synd[c] ? 1 : 0)) bad = true;
        }
        *done = it + 1;
        if (!huge_any(bad, s)) return 1;
    }
    return 0;
}

// the member columns (indices into the candidate columns) of candidate l in the reference's order: osd_cs -- k of weight one, then the
// pairs i < j < order (osd_window.pyx:134-155); osd_e -- every pattern of the first `order` columns, pattern l = the binary digits
// of l (:128-132).  Returns how many.
__device__ inline int huge_cand_members(int osd_method, int w, int k, long long l, int *mem) {
    int nm = 0;
    if (osd_method == 2) {
        if (l < k) mem[nm++] = (int)l;
        else { long long q = l - k; int i = 0; while (q >= w - 1 - i) { q -= w - 1 - i; ++i; } mem[nm++] = i; mem[nm++] = i + 1 + (int)q; }
    } else {
        for (int bit = 0; bit < w; ++bit) if ((l >> bit) & 1) mem[nm++] = bit;
    }
    return nm;
}

// The arrays of the elimination and the sweep (huge_osd) in a workgroup's scratch slice, for a matrix of m checks (wm = words per
// column of T), n columns, rank pivots, k = new_n - rank candidate columns:
//   T [wm * m] words, ycand [max(reduced candidate columns, 1) * wm] words, pm [2 * wm + 4] doubles, pc / pr [rank + 1], rowof [n],
//   plist [max(n, m)], ht [k + 1], lv [n], lc [max(m, new_n)], best 64 bytes, bak [n] (the OSD-0 solution), hard [n] (the sweep's winner)
struct HugeOsdView {
    uint64_t *T, *ycand;
    double *pm;
    int32_t *pc, *pr, *rowof, *plist, *ht, *lv, *lc, *best;
    uint8_t *bak, *hard;
};

// OSD on one matrix (osd_window.pyx:201-284 == bp4_osd.pyx:299-368; mod2sparse_decomp_osd / LU_forward_backward_solve,
// src/include/mod2sparse_extra.cpp:78-376) with every array in HBM: the elimination over all n columns in the order idx[] lists them,
// the OSD-0 solution (also into osd0 when given), and with osd_order > 0 the osd_e / osd_cs sweep over the first new_n - rank
// non-pivot columns among the first new_n sorted ones, path metrics from g.llr.  One body for osd_window's general form
// (huge_kernel) and bp4_osd's (huge_bp4_osd_kernel).  Returns the solution (v.bak or v.hard; behind a barrier only: the caller
// synchronises before reading it), its path metric in min_pm; adds the row additions to rowadds.
__device__ __forceinline__ const uint8_t *huge_osd(const HugeGraphDev &g, int wm, int rank, int new_n, int osd_method, int osd_order,
                                                  const int32_t *idx, const uint8_t *synd, uint8_t *osd0, const HugeOsdView &v,
                                                  HugeLds &s, int &rowadds, double &min_pm) {
    const int tid = threadIdx.x, m = g.m, n = g.n;
    const uint8_t *ret;
    // transform matrix T (word-major: T[w * m + j] = word w of column j), identity
    for (int i = tid; i < wm * m; i += HNT) { const int w = i / m, j = i - w * m; v.T[i] = (j >> 6) == w ? (1ull << (j & 63)) : 0ull; }
    for (int x = tid; x < n; x += HNT) v.rowof[x] = -1;
    uint64_t *pivmask = (uint64_t *)v.pm; // [wm] (the path metrics are not needed before the sweep)
    for (int w = tid; w < wm; w += HNT) pivmask[w] = 0ull;
    __syncthreads();
    // greedy first-independent columns in sorted order; pivot row = lowest unpivoted row with a 1 (mod2sparse_extra.cpp:113-376).
    // Sixteen columns are reduced against T at a time (one wave each); the first of them with a pivot is applied, the scan
    // resumes behind it (the reduced forms of the later ones are stale then).
    int np = 0, kcol = 0;
    const int wv = tid >> 6, lane = tid & 63;
    while (np < rank && kcol < n) {
        {
            const int kk = kcol + wv;
            uint64_t y = 0ull;
            if (kk < n && lane < wm) {
                const int col = idx[kk];
                for (int k = g.col_ptr[col]; k < g.col_ptr[col + 1]; ++k) y ^= v.T[(size_t)lane * m + g.row_idx[k]];
            }
            s.y[wv * 64 + lane] = y;
            const uint64_t cand = (lane < wm) ? (y & ~pivmask[lane]) : 0ull;
            const unsigned long long bal = __ballot(cand != 0ull);
            if (lane == 0) s.piv[wv] = -1;
            if (bal) {
                const int w0 = __ffsll((long long)bal) - 1;
                const uint64_t cw = __shfl(cand, w0, 64);
                if (lane == 0) s.piv[wv] = w0 * 64 + (__ffsll((long long)cw) - 1);
            }
        }
        __syncthreads();
        int first = -1;
        for (int q = 0; q < 16; ++q) if (s.piv[q] >= 0) { first = q; break; }
        if (first < 0) { kcol += 16; __syncthreads(); continue; }
        const int r = s.piv[first], col = idx[kcol + first];
        // Gauss-Jordan step in transform form: every column j of T with bit r set takes S = y with bit r cleared
        const unsigned long long *yv = &s.y[first * 64];
        for (int j = tid; j < m; j += HNT) {
            if ((v.T[(size_t)(r >> 6) * m + j] >> (r & 63)) & 1ull) {
                for (int w = 0; w < wm; ++w) {
                    uint64_t sv = (uint64_t)yv[w];
                    if (w == (r >> 6)) sv &= ~(1ull << (r & 63));
                    if (sv) v.T[(size_t)w * m + j] ^= sv;
                }
            }
        }
        if (tid == 0) {
            v.pc[np] = col; v.pr[np] = r; v.rowof[col] = r;
            pivmask[r >> 6] |= 1ull << (r & 63);
            int ra = 0;
            for (int w = 0; w < wm; ++w) ra += __popcll((unsigned long long)yv[w]);
            s.flag[3] = ra - 1;
        }
        __syncthreads();
        rowadds += s.flag[3];
        ++np;
        kcol += first + 1;
        __syncthreads();
    }
    // base = T * syndrome; the OSD-0 solution: pivot column i takes bit pr[i] of it, every other column 0
    uint64_t *basev = (uint64_t *)(v.pm) + wm; // [wm]
    {
        const int cnt = huge_compact(m, v.plist, s, [&](int c) { return synd[c] != 0; });
        for (int w = tid; w < wm; w += HNT) {
            uint64_t y = 0ull;
            for (int i = 0; i < cnt; ++i) y ^= v.T[(size_t)w * m + v.plist[i]];
            basev[w] = y;
        }
        __syncthreads();
    }
    uint8_t *o0 = v.bak; // [n] osd0_decoding
    for (int x = tid; x < n; x += HNT) { const int r = v.rowof[x]; o0[x] = (r >= 0 && ((basev[r >> 6] >> (r & 63)) & 1ull)) ? 1 : 0; }
    __syncthreads();
    const int npiv = huge_compact(n, v.plist, s, [&](int x) { return v.rowof[x] >= 0; }); // pivot columns, ascending
    {
        const int cnt = huge_compact(n, v.lv, s, [&](int x) { return o0[x] != 0; });
        if (tid == 0) v.best[2] = cnt, ((double *)v.best)[2] = huge_ordered_sum(v.lv, cnt, g.llr);
        __syncthreads();
    }
    min_pm = ((double *)v.best)[2];
    if (osd0) for (int x = tid; x < n; x += HNT) osd0[x] = o0[x];
    ret = o0;
    if (osd_order > 0) {
        // candidate columns: the first k = new_n - rank non-pivot columns among the first new_n of the sorted order (:243-256)
        const int k = new_n - rank;
        int nht = huge_compact(new_n, v.lc, s, [&](int i) { return v.rowof[idx[i]] < 0; }); // positions in sorted order
        nht = min(nht, k);
        for (int j = tid; j < nht; j += HNT) v.ht[j] = idx[v.lc[j]];
        __syncthreads();
        const int nyc = (osd_method == 2) ? nht : min(nht, osd_order); // columns whose reduced form the sweep needs
        for (int j = wv; j < nyc; j += 16) {
            uint64_t y = 0ull;
            if (lane < wm) { const int col = v.ht[j]; for (int q = g.col_ptr[col]; q < g.col_ptr[col + 1]; ++q) y ^= v.T[(size_t)lane * m + g.row_idx[q]]; }
            if (lane < wm) v.ycand[(size_t)j * wm + lane] = y;
        }
        __syncthreads();
        const int w = osd_order;
        const long long ncand = (osd_method == 2) ? (long long)k + (long long)w * (w - 1) / 2 : (1ll << w);
        double bpm = min_pm;
        long long bidx = -1;
        for (long long l = tid; l < ncand; l += HNT) {
            int mem[16];
            const int nm = huge_cand_members(osd_method, w, k, l, mem);
            // members beyond the candidate columns that exist contribute nothing (enc rows are k long: they cannot occur)
            int nmv = 0;
            int memc[16];
            for (int q = 0; q < nm; ++q) if (mem[q] < nht) { mem[nmv] = mem[q]; memc[nmv] = v.ht[mem[q]]; ++nmv; }
            // candidate columns in ascending column order for the ordered sum
            for (int p = 1; p < nmv; ++p) { const int cc = memc[p], mm2 = mem[p]; int q = p - 1; while (q >= 0 && memc[q] > cc) { memc[q + 1] = memc[q]; mem[q + 1] = mem[q]; --q; } memc[q + 1] = cc; mem[q + 1] = mm2; }
            double pm = 0.0;
            int nx = 0;
            for (int i = 0; i < npiv; ++i) {
                const int col = v.plist[i], r = v.rowof[col];
                while (nx < nmv && memc[nx] < col) pm += g.llr[memc[nx++]];
                uint64_t bit = (basev[r >> 6] >> (r & 63)) & 1ull;
                for (int q = 0; q < nmv; ++q) bit ^= (v.ycand[(size_t)mem[q] * wm + (r >> 6)] >> (r & 63)) & 1ull;
                if (bit) pm += g.llr[col];
            }
            while (nx < nmv) pm += g.llr[memc[nx++]];
            if (pm < bpm) { bpm = pm; bidx = l; } // (ascending l per thread: strict < keeps the earliest)
        }
        // block minimum of (pm, index): the reference keeps the first candidate that is strictly better than everything before
        for (int o = 32; o > 0; o >>= 1) {
            const double op = __shfl_xor(bpm, o, 64);
            const long long oi = __shfl_xor(bidx, o, 64);
            if (oi >= 0 && (bidx < 0 || op < bpm || (op == bpm && oi < bidx))) { bpm = op; bidx = oi; }
        }
        __syncthreads();
        if (lane == 0) { s.red[wv] = (unsigned long long)__double_as_longlong(bpm); ((long long *)s.y)[wv] = bidx; }
        __syncthreads();
        bpm = min_pm; bidx = -1;
        for (int q = 0; q < HNT / 64; ++q) {
            const double op = __longlong_as_double((long long)s.red[q]);
            const long long oi = ((long long *)s.y)[q];
            if (oi >= 0 && (bidx < 0 || op < bpm || (op == bpm && oi < bidx))) { bpm = op; bidx = oi; }
        }
        __syncthreads();
        if (bidx >= 0 && bpm < min_pm) {
            min_pm = bpm;
            int mem[16];
            const int nm = huge_cand_members(osd_method, w, k, bidx, mem);
            uint8_t *ow = v.hard; // (the BP decisions went out before)
            for (int x = tid; x < n; x += HNT) {
                const int r = v.rowof[x];
                uint64_t bit = 0;
                if (r >= 0) {
                    bit = (basev[r >> 6] >> (r & 63)) & 1ull;
                    for (int q = 0; q < nm; ++q) if (mem[q] < nht) bit ^= (v.ycand[(size_t)mem[q] * wm + (r >> 6)] >> (r & 63)) & 1ull;
                }
                ow[x] = (uint8_t)bit;
            }
            __syncthreads();
            if (tid == 0) for (int q = 0; q < nm; ++q) if (mem[q] < nht) ow[v.ht[mem[q]]] = 1;
            __syncthreads();
            ret = ow;
        }
    }
    return ret;
}

// ---- host side ----

// What both general forms own and do alike; each derives its handle from this and adds its argument template and kernel launch.
struct HugeHost : HugeIface {
    int device = 0, npad = 0; // npad: n rounded up to a power of two, the length of the bitonic sort
    DevBuf graph, scratch;
    int64_t stride = 0;       // scratch bytes of one workgroup: the sum of what take() handed out
    int grid_max = 0;         // one workgroup per CU, each looping over the batch
    std::mutex mu;
    hipStream_t last_stream = nullptr;
    bool last_stream_set = false;

    static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

    // the header check of a description (the size limits follow in the create functions, each in its decoder's wording)
    static int check_desc(const swd_graph_desc *g) {
        if (!g || !g->row_ptr || !g->col_idx || !g->channel_probs) { set_error("null graph description"); return -1; }
        if (g->m <= 0 || g->n <= 0 || g->nnz <= 0 || g->row_ptr[0] != 0 || g->row_ptr[g->m] != g->nnz) { set_error("empty or inconsistent check matrix"); return -1; }
        return 0;
    }

    // Copies, checks and sorts the CSR (c keeps the host arrays for the caller), builds the CSC, c2r, llr and on request r2c, and
    // uploads all of it as one buffer of 256-byte aligned arrays: *gd, *r2c point into it.
    int ingest(const swd_graph_desc *g, int dev, CsrHost &c, HugeGraphDev *gd, const int32_t **r2c = nullptr) {
        m = g->m; n = g->n; device = dev;
        const size_t E = (size_t)g->nnz;
        c.row_ptr.assign(g->row_ptr, g->row_ptr + m + 1);
        c.col_idx.assign(g->col_idx, g->col_idx + E);
        if (csr_check_rows(m, n, c.row_ptr, c.col_idx)) return -1;
        csr_transpose(m, n, g->channel_probs, r2c != nullptr, c);
        npad = 2; while (npad < n) npad <<= 1;
        if (hipSetDevice(device) != hipSuccess) { set_error(SWD_ERR_DEVICE, "hipSetDevice(%d) failed", device); return -1; }
        const struct { const void *src; size_t bytes; } seg[7] = {
            {c.row_ptr.data(), (size_t)(m + 1) * 4}, {c.col_idx.data(), E * 4}, {c.col_ptr.data(), (size_t)(n + 1) * 4}, {c.row_idx.data(), E * 4},
            {c.c2r.data(), E * 4}, {c.llr.data(), (size_t)n * 8}, {c.r2c.data(), r2c ? E * 4 : 0}};
        size_t off[8] = {0};
        for (int i = 0; i < 7; ++i) off[i + 1] = off[i] + al(seg[i].bytes);
        if (graph.reserve(off[7])) return -1;
        char *d = (char *)graph.p;
        for (int i = 0; i < 7; ++i)
            if (seg[i].bytes && hipMemcpy(d + off[i], seg[i].src, seg[i].bytes, hipMemcpyHostToDevice) != hipSuccess) { set_error(SWD_ERR_DEVICE, "hipMemcpy of the graph failed"); return -1; }
        *gd = HugeGraphDev{m, n, (const int32_t *)(d + off[0]), (const int32_t *)(d + off[1]), (const int32_t *)(d + off[2]),
                           (const int32_t *)(d + off[3]), (const int32_t *)(d + off[4]), (const double *)(d + off[5])};
        if (r2c) *r2c = (const int32_t *)(d + off[6]);
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 64;
        grid_max = std::max(1, cus);
        return 0;
    }

    // the next array of a workgroup's scratch slice: 256-byte aligned offsets in call order
    int64_t take(size_t bytes) { const int64_t at = stride; stride += (int64_t)al(bytes); return at; }

    int decode_dev(int32_t B, const uint8_t *synd, int64_t synd_stride, uint8_t *out, int64_t out_stride, int32_t *stats,
                   double *min_pm, double *hist, int32_t hist_is_state, uint8_t *osd0, uint8_t *bp_dec, void *stream) final {
        std::lock_guard<std::mutex> lk(mu); // one scratch area: launches of one handle run one after the other
        SWD_HIP(hipSetDevice(device));
        const int grid = std::max(1, std::min(B, grid_max));
        if (scratch.reserve((size_t)grid * (size_t)stride)) return -1;
        const HugeIo io{synd, synd_stride ? synd_stride : m, out, out_stride ? out_stride : n, stats, min_pm, hist, hist_is_state,
                        scratch.as<uint8_t>(), stride};
        hipStream_t st = (hipStream_t)stream;
        // (the scratch area is shared by consecutive launches of this handle: order them on the device too)
        if (last_stream_set && last_stream != st) SWD_HIP(hipStreamSynchronize(last_stream));
        launch(B, io, osd0, bp_dec, grid, st);
        SWD_HIP(hipGetLastError());
        last_stream = st; last_stream_set = true;
        return 0;
    }
    // the form's kernel on `grid` workgroups of HNT threads: its argument template with io (and what else a launch sets) filled in
    virtual void launch(int32_t B, const HugeIo &io, uint8_t *osd0, uint8_t *bp_dec, int grid, hipStream_t st) = 0;
};

} // namespace swd
