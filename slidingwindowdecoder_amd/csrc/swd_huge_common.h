// Device helpers of the general forms (swd_huge.hip: osd_window, swd_huge_gdg.hip: the guessing decoders): one 1024-thread
// workgroup per decode, every array in HBM, LDS only for block-wide scans and reductions.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

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

} // namespace swd
