// bp4_osd on graphs beyond the tuned BP kernels (swd_bp4_kernel.h: more than 8 columns above weight 10, more than 1024 checks, rows
// past the graph tables, or messages past 160 KB of LDS): the Euclidean-geometry codes [[273,111,17]] and [[1057,571,33]] of
// Misc.ipynb cell 8, large light codes.  The reference has no size limit (src/include/mod2sparse.c:52-80).  The form of swd_huge.hip
// and swd_huge_gdg.hip: one 1024-thread workgroup per unit -- a shot of decode, one of the four runs of a shot of camel_decode -- a
// grid of at most one workgroup per CU that loops over the units, both graphs in HBM as CSR + CSC, every per-unit array in the
// workgroup's slice of an HBM buffer, LDS only for block-wide flags (and the scan behind cal_pm).  huge_bp4_kernel runs BP; with
// osd_order >= 0 (a handle created with SWD_BP4_GENERAL_OSD) the decodes it leaves unconverged are queued for huge_bp4_osd_kernel
// below, the elimination in HBM that also finishes the queue of the tuned BP kernels on graphs with heavy columns.
// Restated from /root/reference/src/bp4_osd.pyx, bit for bit (exp / log1p of swd_libm.h through bp4_log1pexp / bp4_logaddexp):
//   reset 371-386, vn_set_value 389-423, bp_init 425-442, bp4_decode_llr 444-481, cn_update_all 483-529, vn_update 533-589,
//   cal_pm 250-259.
// The reference keeps two messages per edge; so does this form: bit_to_check in CSR order (the check pass walks rows), check_to_bit
// in CSC order (the node sums walk columns).  Per iteration:
//   check pass   one thread per check of Hx and of Hz, any row weight: first / second minimum of the clipped magnitudes and the
//                parity of the signs, seeded by the check's value -- what the reference's two sweeps leave per edge
//   node totals  one thread per live node adds the check messages of its Hz list, then of its Hx list, rows ascending, as ONE chain
//                of fp64 adds (the order is part of the result: bp4_heavy_sum, swd_bp4_kernel.h), then posteriors, decision and the
//                two numerators log1pexp(-llrx_hx), log1pexp(-llrz_hz)
//   convergence  parity of Hx * z-string and Hz * x-string against the syndromes, one block-wide any
//   edge pass    one thread per CSC position of both graphs: the new bit_to_check from its node's totals.  A column of weight 1024
//                costs two serial chains per iteration, its 2048 logaddexp evaluations spread over the block.
#include <math.h>
#include <string.h>

#include <memory>

#include "swd_huge_common.h"
#include "swd_bp4_kernel.h"

namespace swd {

struct SwdHugeBp4Args {
    HugeGraphDev gx, gz;                   // (llr unused: the channel LLRs are the three arrays below)
    const int32_t *r2cx, *r2cz;            // CSR edge -> CSC position
    const int32_t *nodex, *nodez;          // CSC position -> column
    const double *llr_x, *llr_y, *llr_z;   // [n] channel LLRs (bp4_osd.pyx:131-133)
    int32_t Ex, Ez;
    HugeBp4Io io;
    uint8_t *scratch; int64_t stride;      // a workgroup's slice: scratch + blockIdx.x * stride
    // offsets inside a slice
    int64_t o_b2cx, o_c2bx, o_b2cz, o_c2bz, o_inix, o_iniz, o_tx, o_ty, o_tz, o_numx, o_numz, o_decx, o_decz, o_cnx, o_cnz, o_list;
};

// (calls, not inlined copies: a 1024-thread workgroup has 128 registers per lane, and exp / log1p inlined at every site is what
// spilled in huge_gdg_kernel's neighbours; the callee is the one body of swd_bp4_kernel.h)
__device__ __attribute__((noinline)) double hb_log1pexp(double x) { return bp4_log1pexp(x); }
__device__ __attribute__((noinline)) double hb_logaddexp(double x, double y) { return bp4_logaddexp(x, y); }

// sum of msg[k0 .. k1) in index order by ONE lane (bp4_heavy_sum's rule); eight loads are issued ahead of their dependent adds
__device__ __forceinline__ double hb_chain(const double *msg, int k0, int k1) {
    double s = 0.0;
#pragma unroll 1
    for (; k0 + 8 <= k1; k0 += 8) {
        double c[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = msg[k0 + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += c[j];
    }
    for (; k0 < k1; ++k0) s += msg[k0];
    return s;
}

// cn_update_all (bp4_osd.pyx:483-529) for one check: the clip is stored back, check_to_bit goes to the edge's CSC position
__device__ __forceinline__ void hb_check(const HugeGraphDev &g, const int32_t *r2c, int c, int cv, double *b2c, double *c2b, double alpha) {
    const int e0 = g.row_ptr[c], e1 = g.row_ptr[c + 1];
    double min1 = 1e308, min2 = 1e308;
    int arg = -1, neg = cv;
    for (int e = e0; e < e1; ++e) {
        double x = b2c[e];
        // plain < and > like the reference (:506-511): a NaN passes the clip, never lowers the minimum and counts as positive
        x = (x > 50.0) ? 50.0 : ((x < -50.0) ? -50.0 : x);
        b2c[e] = x;
        const double ax = (x != x) ? 1e308 : fabs(x);
        arg = (ax < min1) ? e : arg;
        min2 = fmin(min2, fmax(min1, ax));
        min1 = fmin(min1, ax);
        neg += (x <= 0) ? 1 : 0;
    }
    for (int e = e0; e < e1; ++e) {
        const double x = b2c[e];
        const int sg = (neg - ((x <= 0) ? 1 : 0)) & 1;
        const double mag = (e == arg) ? min2 : min1; // minimum over the OTHER edges (none: the 1e308 sentinel)
        c2b[r2c[e]] = mag * (sg ? -alpha : alpha);
    }
}

__global__ void __launch_bounds__(HNT) huge_bp4_kernel(const SwdHugeBp4Args a) {
    __shared__ HugeLds s;
    const int tid = threadIdx.x, n = a.gx.n, mx = a.gx.m, mz = a.gz.m, Ex = a.Ex, Ez = a.Ez;
    uint8_t *base = a.scratch + (int64_t)blockIdx.x * a.stride;
    double *b2cx = (double *)(base + a.o_b2cx), *c2bx = (double *)(base + a.o_c2bx);
    double *b2cz = (double *)(base + a.o_b2cz), *c2bz = (double *)(base + a.o_c2bz);
    double *inix = (double *)(base + a.o_inix), *iniz = (double *)(base + a.o_iniz);
    double *tx = (double *)(base + a.o_tx), *ty = (double *)(base + a.o_ty), *tz = (double *)(base + a.o_tz);
    double *numx = (double *)(base + a.o_numx), *numz = (double *)(base + a.o_numz);
    uint8_t *decx = base + a.o_decx, *decz = base + a.o_decz, *cnx = base + a.o_cnx, *cnz = base + a.o_cnz;
    int32_t *list = (int32_t *)(base + a.o_list);
    const int camel = a.io.camel, max_iter = a.io.max_iter;
    const int nunits = camel ? 4 * a.io.B : a.io.B;
    const int fixed = camel ? n - 1 : -1; // the decided qubit of a camel run
    const double alpha = a.io.alpha;
    // the messages of bp_init depend on the channel only: once per workgroup
    for (int v = tid; v < n; v += HNT) {
        const double llrx = a.llr_x[v], llry = a.llr_y[v], llrz = a.llr_z[v];
        const double den = hb_logaddexp(-1. * llry, -1. * llrz);
        inix[v] = hb_log1pexp(-1. * llrx) - den;
        iniz[v] = hb_log1pexp(-1. * llrz) - den; // sic (bp4_osd.pyx:438)
    }
    for (int unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const int b = camel ? unit >> 2 : unit;
        const uint8_t *sx_b = a.io.sx + (int64_t)b * mx, *sz_b = a.io.sz + (int64_t)b * mz;
        __syncthreads(); // the previous unit is done with the slice (first unit: the bp_init messages are written)
        // reset + bp_init (bp4_osd.pyx:371-386, 425-442)
        for (int c = tid; c < mx; c += HNT) cnx[c] = sx_b[c] ? 1 : 0;
        for (int c = tid; c < mz; c += HNT) cnz[c] = sz_b[c] ? 1 : 0;
        for (int v = tid; v < n; v += HNT) { decx[v] = 0; decz[v] = 0; }
        for (int e = tid; e < Ex; e += HNT) b2cx[e] = inix[a.gx.col_idx[e]];
        for (int e = tid; e < Ez; e += HNT) b2cz[e] = iniz[a.gz.col_idx[e]];
        __syncthreads();
        if (camel) { // vn_set_value(n - 1, value) after bp_init (:234, 389-423): the qubit keeps its bp_init messages for good
            const int value = unit & 3, x = value & 1, z = value >> 1;
            if (tid == 0) { decx[fixed] = (uint8_t)x; decz[fixed] = (uint8_t)z; }
            if (z) for (int k = a.gx.col_ptr[fixed] + tid; k < a.gx.col_ptr[fixed + 1]; k += HNT) cnx[a.gx.row_idx[k]] ^= 1;
            if (x) for (int k = a.gz.col_ptr[fixed] + tid; k < a.gz.col_ptr[fixed + 1]; k += HNT) cnz[a.gz.row_idx[k]] ^= 1;
            __syncthreads();
        }
        // bp4_decode_llr (:444-481)
        int conv = 0, iters = 0;
        for (int it = 0; it < max_iter; ++it) {
            // check pass over every check of both graphs: nothing is skipped, a decided node's edge takes part with its bp_init message
            for (int q = tid; q < mx + mz; q += HNT) {
                if (q < mx) hb_check(a.gx, a.r2cx, q, cnx[q], b2cx, c2bx, alpha);
                else hb_check(a.gz, a.r2cz, q - mx, cnz[q - mx], b2cz, c2bz, alpha);
            }
            __syncthreads();
            // node totals (:533-569)
            for (int v = tid; v < n; v += HNT) {
                if (v == fixed) continue; // (decided, :459-460)
                double llrx_hx = hb_chain(c2bz, a.gz.col_ptr[v], a.gz.col_ptr[v + 1]);
                double llrz_hz = hb_chain(c2bx, a.gx.col_ptr[v], a.gx.col_ptr[v + 1]);
                const double llry_all = llrx_hx + llrz_hz + a.llr_y[v];
                llrx_hx = llrx_hx + a.llr_x[v];
                llrz_hz = llrz_hz + a.llr_z[v];
                tx[v] = llrx_hx; ty[v] = llry_all; tz[v] = llrz_hz;
                int idx;
                if (0 < llrx_hx && 0 < llry_all && 0 < llrz_hz) idx = 0;
                else if (llrx_hx < llry_all && llrx_hx < llrz_hz) idx = 1;
                else if (llry_all > llrz_hz) idx = 2;
                else idx = 3;
                decx[v] = (uint8_t)(idx & 1); decz[v] = (uint8_t)(idx >> 1);
                numx[v] = hb_log1pexp(-1. * llrx_hx);
                numz[v] = hb_log1pexp(-1. * llrz_hz);
            }
            __syncthreads();
            // Hx * z-string == synd_x and Hz * x-string == synd_z (:464-479), the decided qubit included
            bool bad = false;
            for (int q = tid; q < mx + mz; q += HNT) {
                const bool hz = q >= mx;
                const int c = hz ? q - mx : q;
                const HugeGraphDev &g = hz ? a.gz : a.gx;
                const uint8_t *dec = hz ? decx : decz;
                int p = 0;
                for (int e = g.row_ptr[c]; e < g.row_ptr[c + 1]; ++e) p ^= dec[g.col_idx[e]];
                if (p != ((hz ? sz_b : sx_b)[c] ? 1 : 0)) bad = true;
            }
            iters = it + 1;
            if (!huge_any(bad, s)) { conv = 1; break; }
            if (it + 1 >= max_iter) break; // (the messages of the last update feed no check pass)
            // edge pass (:571-589): position k of Hx, then of Hz
            for (int k = tid; k < Ex + Ez; k += HNT) {
                const bool hz = k >= Ex;
                const int kk = hz ? k - Ex : k;
                const int v = (hz ? a.nodez : a.nodex)[kk];
                if (v == fixed) continue;
                const double c = (hz ? c2bz : c2bx)[kk];
                const double aa = (hz ? tx[v] : tz[v]) - c, bb = ty[v] - c;
                const double num = (hz ? numz : numx)[v];
                (hz ? b2cz : b2cx)[(hz ? a.gz.c2r : a.gx.c2r)[kk]] = num - hb_logaddexp(-1. * aa, -1. * bb);
            }
            __syncthreads();
        }
        __syncthreads();
        if (camel) {
            uint8_t *dst = a.io.camel_dec + (int64_t)unit * 2 * n;
            for (int v = tid; v < n; v += HNT) { dst[v] = decx[v]; dst[n + v] = decz[v]; }
            // cal_pm (:250-259): the channel LLRs of the non-identity decisions, added in qubit order by one thread
            const int cnt = conv ? huge_compact(n, list, s, [&](int v) { return (decx[v] | decz[v]) != 0; }) : 0;
            if (tid == 0) {
                double pm = 0.0;
                for (int i = 0; i < cnt; ++i) {
                    const int v = list[i];
                    pm += (decx[v] && decz[v]) ? a.llr_y[v] : (decx[v] ? a.llr_x[v] : a.llr_z[v]);
                }
                a.io.camel_pm[unit] = pm;
                a.io.camel_st[2 * unit] = conv; a.io.camel_st[2 * unit + 1] = iters;
            }
            continue;
        }
        uint8_t *out_b = a.io.out + (int64_t)b * 2 * n;
        const bool to_osd = !conv && a.io.osd_order >= 0; // finished by huge_bp4_osd_kernel from the posteriors stored below
        for (int v = tid; v < n; v += HNT) { out_b[v] = decx[v]; out_b[n + v] = decz[v]; }
        if (a.io.bp_dec)
            for (int v = tid; v < n; v += HNT) { a.io.bp_dec[(int64_t)b * 2 * n + v] = decx[v]; a.io.bp_dec[(int64_t)b * 2 * n + n + v] = decz[v]; }
        if (a.io.osd0 && conv)
            for (int v = tid; v < n; v += HNT) { a.io.osd0[(int64_t)b * 2 * n + v] = decx[v]; a.io.osd0[(int64_t)b * 2 * n + n + v] = decz[v]; }
        if (a.io.lpr && iters > 0) {
            double *lpr_b = a.io.lpr + (int64_t)b * 3 * n;
            for (int v = tid; v < n; v += HNT) { lpr_b[v] = tx[v]; lpr_b[n + v] = ty[v]; lpr_b[2 * (int64_t)n + v] = tz[v]; }
        }
        if (tid == 0) {
            int32_t *st = a.io.stats + (int64_t)b * SWD_STAT_WORDS;
            st[0] = (conv ? SWD_EXIT_PRE : (to_osd ? SWD_EXIT_OSD : SWD_EXIT_NO_OSD)) | (conv ? SWD_STATUS_CONVERGE : 0);
            st[1] = iters; st[2] = iters; st[3] = 0; st[4] = n; st[5] = mx + mz; st[6] = Ex + Ez; st[7] = 0;
            if (to_osd) a.io.osd_list[atomicAdd(a.io.osd_count, 1u)] = b;
        }
    }
}

// ---- the elimination (bp4_osd.pyx:261-368) ----

// The decodes a BP kernel queued -- huge_bp4_kernel above, or a tuned bp4_kernel (swd_bp4_kernel.h) of a handle created with
// SWD_BP4_GENERAL_OSD -- one per workgroup at a time: osd('x') on Hx, synd_x gives the Z string, osd('z') on Hz, synd_z the X string
// (bp4_osd.decode :212-219).  Per basis: ordering keys from the stored posteriors (:280 / :297), the stable ascending order
// (huge_f2key + huge_sort), then huge_osd (swd_huge_common.h) -- the elimination over all n sorted columns, the OSD-0 solution, the
// osd_e / osd_cs sweep with path metrics from prior_llr_x / prior_llr_z (gx.llr / gz.llr).  No bound on a column's weight, up to 4096
// checks per matrix; T and the candidate columns are sized for the larger basis and used by the two in turn.
struct SwdHugeBp4OsdArgs {
    HugeGraphDev gx, gz;                 // llr: prior_llr_x (px + py), prior_llr_z (pz + py)  (bp4_osd.pyx:134-137)
    int32_t rank_x, rank_z, new_n_x, new_n_z; // new_n_z: n, or n - rank_x + rank_z -- the z sweep walks kx candidates (swd_bp4.hip)
    int32_t npad, osd_method, osd_order;
    HugeBp4OsdIo io;
    uint8_t *scratch; int64_t stride;    // a workgroup's slice: scratch + blockIdx.x * stride
    int64_t o_key, o_idx, o_T, o_ycand, o_pm, o_pc, o_pr, o_rowof, o_plist, o_ht, o_lv, o_lc, o_best, o_bak, o_hard;
};

__global__ void __launch_bounds__(HNT) huge_bp4_osd_kernel(const SwdHugeBp4OsdArgs a) {
    __shared__ HugeLds s;
    const int tid = threadIdx.x, n = a.gx.n;
    uint8_t *base = a.scratch + (int64_t)blockIdx.x * a.stride;
    uint64_t *key = (uint64_t *)(base + a.o_key);
    int32_t *idx = (int32_t *)(base + a.o_idx);
    HugeOsdView v;
    v.T = (uint64_t *)(base + a.o_T); v.ycand = (uint64_t *)(base + a.o_ycand); v.pm = (double *)(base + a.o_pm);
    v.pc = (int32_t *)(base + a.o_pc); v.pr = (int32_t *)(base + a.o_pr); v.rowof = (int32_t *)(base + a.o_rowof);
    v.plist = (int32_t *)(base + a.o_plist); v.ht = (int32_t *)(base + a.o_ht); v.lv = (int32_t *)(base + a.o_lv);
    v.lc = (int32_t *)(base + a.o_lc); v.best = (int32_t *)(base + a.o_best); v.bak = base + a.o_bak; v.hard = base + a.o_hard;
    const int count = min((int)*a.io.osd_count, a.io.B);
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
        const int b = a.io.osd_list[q];
        const double *lpr_b = a.io.lpr + (int64_t)b * 3 * n;
        uint8_t *out_b = a.io.out + (int64_t)b * 2 * n;
        int rowadds = 0;
        for (int basis = 0; basis < 2; ++basis) {
            const HugeGraphDev g = basis == 0 ? a.gx : a.gz;
            const uint8_t *synd = basis == 0 ? a.io.sx + (int64_t)b * g.m : a.io.sz + (int64_t)b * g.m;
            __syncthreads(); // the previous basis (or decode) is done with the slice
            for (int i = tid; i < a.npad; i += HNT) {
                if (i < n) {
                    const double lx = lpr_b[i], ly = lpr_b[n + i], lz = lpr_b[2 * (int64_t)n + i];
                    const double post = basis == 0 ? hb_log1pexp(-1. * lx) - hb_logaddexp(-1. * ly, -1. * lz)
                                                   : hb_log1pexp(-1. * lz) - hb_logaddexp(-1. * ly, -1. * lx);
                    key[i] = huge_f2key(post);
                    idx[i] = i;
                } else { key[i] = ~0ull; idx[i] = 0x7FFFFFFF; }
            }
            __syncthreads();
            huge_sort(key, idx, a.npad);
            uint8_t *o0 = a.io.osd0 ? a.io.osd0 + (int64_t)b * 2 * n + (basis == 0 ? n : 0) : nullptr;
            double min_pm;
            const uint8_t *ret = huge_osd(g, (g.m + 63) >> 6, basis == 0 ? a.rank_x : a.rank_z, basis == 0 ? a.new_n_x : a.new_n_z,
                                          a.osd_method, a.osd_order, idx, synd, o0, v, s, rowadds, min_pm);
            __syncthreads();
            uint8_t *dst = out_b + (basis == 0 ? n : 0);
            for (int x = tid; x < n; x += HNT) dst[x] = ret[x];
        }
        if (tid == 0) a.io.stats[(int64_t)b * SWD_STAT_WORDS + 7] = rowadds; // (word 0 is the BP kernel's: SWD_EXIT_OSD, no converge bit)
    }
}

// ---- host side ----

struct HugeBp4 : HugeBp4Iface {
    static constexpr int kSlots = 4;             // Bp4::kSlots (swd_bp4.hip)
    static constexpr int64_t kSlotBytes = 8ll << 30; // a launch slot's scratch area never exceeds this: the grid shrinks to fit
    int device = 0, grid_max = 1, osd_grid_max = 1;
    bool has_bp = false, has_osd = false;
    // one device copy of the graphs for BP and the elimination; per launch slot one area for each of the two kernels, so that four
    // launches of a handle run side by side
    DevBuf graph, scratch[kSlots], osd_scratch[kSlots];
    int64_t stride = 0;
    SwdHugeBp4Args tmpl{};
    SwdHugeBp4OsdArgs otmpl{};

    static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
    int64_t take(size_t bytes) { const int64_t at = stride; stride += (int64_t)al(bytes); return at; }

    int launch(const HugeBp4Io &io, int slot, void *stream) override {
        if (slot < 0 || slot >= kSlots) { set_error("launch slot %d out of range", slot); return -1; }
        if (!has_bp) { set_error("this handle runs the elimination only"); return -1; }
        if (!io.camel && io.osd_order >= 0 && (!has_osd || !io.lpr || !io.osd_list || !io.osd_count)) { set_error("OSD launch without its queue"); return -1; }
        SWD_HIP(hipSetDevice(device));
        const int64_t units = io.camel ? 4 * (int64_t)io.B : io.B;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(units, grid_max));
        // (a slot's area grows at its first launch of a size and is only touched by launches ordered on the slot's event)
        if (scratch[slot].reserve((size_t)grid * (size_t)stride)) return -1;
        SwdHugeBp4Args a = tmpl;
        a.io = io;
        if (io.camel) a.io.osd_order = -1;
        a.scratch = scratch[slot].as<uint8_t>();
        if (a.io.osd_order >= 0) SWD_HIP(hipMemsetAsync(io.osd_count, 0, sizeof(uint32_t), (hipStream_t)stream));
        hipLaunchKernelGGL(huge_bp4_kernel, dim3(grid), dim3(HNT), 0, (hipStream_t)stream, a);
        SWD_HIP(hipGetLastError());
        return 0;
    }

    int launch_osd(const HugeBp4OsdIo &io, int slot, void *stream) override {
        if (slot < 0 || slot >= kSlots) { set_error("launch slot %d out of range", slot); return -1; }
        if (!has_osd) { set_error("this handle was created without the elimination"); return -1; }
        if (!io.sx || !io.sz || !io.out || !io.stats || !io.lpr || !io.osd_list || !io.osd_count) { set_error("null pointer in the OSD launch"); return -1; }
        SWD_HIP(hipSetDevice(device));
        // the queue length is only known on the device: as many workgroups as the batch could queue, at most one per CU -- those
        // beyond the queue read the count and leave
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(io.B, osd_grid_max));
        if (osd_scratch[slot].reserve((size_t)grid * (size_t)otmpl.stride)) return -1;
        SwdHugeBp4OsdArgs a = otmpl;
        a.io = io;
        a.scratch = osd_scratch[slot].as<uint8_t>();
        hipLaunchKernelGGL(huge_bp4_osd_kernel, dim3(grid), dim3(HNT), 0, (hipStream_t)stream, a);
        SWD_HIP(hipGetLastError());
        return 0;
    }
};

HugeBp4Iface *huge_bp4_create(const swd_graph_desc *hx, const swd_graph_desc *hz, const double *llr, int device, bool bp,
                              const swd_bp4_params *osd) {
    if (HugeHost::check_desc(hx) || HugeHost::check_desc(hz)) return nullptr;
    if (hx->n != hz->n) { set_error(SWD_ERR_VALUE, "Hx, Hz blocklength does not match!"); return nullptr; }
    const int n = hx->n;
    // the bounds of the form: int32 ids with room for the strided loops' increments, and one scratch allocation per launch slot
    if ((long long)n > (1 << 20)) { set_error(SWD_ERR_CAPACITY, "n=%d exceeds bp4_osd's general form limit of 1048576 qubits", n); return nullptr; }
    for (const swd_graph_desc *g : {hx, hz})
        if ((long long)g->m > (1 << 20)) { set_error(SWD_ERR_CAPACITY, "m=%d exceeds bp4_osd's general form limit of 1048576 checks per matrix", g->m); return nullptr; }
    if ((long long)hx->nnz + hz->nnz > (1ll << 26)) {
        set_error(SWD_ERR_CAPACITY, "%lld edges exceed bp4_osd's general form limit of 67108864 edges in Hx and Hz together", (long long)hx->nnz + hz->nnz);
        return nullptr;
    }
    if (osd)
        for (const swd_graph_desc *g : {hx, hz})
            if (g->m > 4096) {
                set_error(SWD_ERR_CAPACITY, "m=%d exceeds the general OSD's limit of 4096 checks per matrix (64 words per column of the elimination's transform matrix)", g->m);
                return nullptr;
            }
    std::unique_ptr<HugeBp4> h(new HugeBp4());
    h->device = device; h->mx = hx->m; h->mz = hz->m; h->n = n; h->has_bp = bp; h->has_osd = osd != nullptr;
    if (hipSetDevice(device) != hipSuccess) { set_error(SWD_ERR_DEVICE, "hipSetDevice(%d) failed", device); return nullptr; }
    CsrHost c[2];
    std::vector<int32_t> node[2];
    const swd_graph_desc *gs[2] = {hx, hz};
    for (int i = 0; i < 2; ++i) {
        const swd_graph_desc *g = gs[i];
        c[i].row_ptr.assign(g->row_ptr, g->row_ptr + g->m + 1);
        c[i].col_idx.assign(g->col_idx, g->col_idx + g->nnz);
        if (csr_check_rows(g->m, n, c[i].row_ptr, c[i].col_idx)) return nullptr;
        csr_transpose(g->m, n, g->channel_probs, true, c[i]);
        node[i].resize((size_t)g->nnz);
        for (int v = 0; v < n; ++v) for (int k = c[i].col_ptr[v]; k < c[i].col_ptr[v + 1]; ++k) node[i][k] = v;
    }
    // the reference's rules that need the ranks (bp4_osd.pyx:92-104), with the tuned path's messages (swd_bp4.hip)
    // (gf2_rank works on dense rows: without the elimination, a graph whose rows would pass 1 GiB keeps -1, "not computed")
    if (osd || (size_t)std::max(hx->m, hz->m) * (size_t)((n + 63) / 64) * 8 <= ((size_t)1 << 30)) {
        h->rank_x = gf2_rank(hx->m, n, c[0].row_ptr, c[0].col_idx);
        h->rank_z = gf2_rank(hz->m, n, c[1].row_ptr, c[1].col_idx);
    }
    if (osd) {
        const int kmin = std::min(n - h->rank_x, n - h->rank_z);
        if (osd->osd_order > kmin) { set_error(SWD_ERR_VALUE, "For this code, the OSD order should be set in the range 0<=osd_oder<=%d.", kmin); return nullptr; }
        if (osd->osd_order > 0 && h->rank_x < h->rank_z) {
            set_error("higher-order OSD with rank(Hx) < rank(Hz) is undefined in the reference (kz = n - rank_x: it reads past its column array) and not supported");
            return nullptr;
        }
        if (osd->osd_method == 1 && osd->osd_order > 15) { set_error("osd_e supports osd_order <= 15 on the device"); return nullptr; }
    }
    // one buffer of 256-byte aligned arrays: per graph row_ptr, col_idx, col_ptr, row_idx, c2r, r2c, node; then the channel LLRs and
    // the two prior LLR arrays of the OSD's path metrics
    struct Seg { const void *src; size_t bytes; };
    std::vector<Seg> seg;
    for (int i = 0; i < 2; ++i) {
        const size_t E = (size_t)gs[i]->nnz;
        seg.push_back({c[i].row_ptr.data(), (size_t)(gs[i]->m + 1) * 4}); seg.push_back({c[i].col_idx.data(), E * 4});
        seg.push_back({c[i].col_ptr.data(), (size_t)(n + 1) * 4}); seg.push_back({c[i].row_idx.data(), E * 4});
        seg.push_back({c[i].c2r.data(), E * 4}); seg.push_back({c[i].r2c.data(), E * 4}); seg.push_back({node[i].data(), E * 4});
    }
    seg.push_back({llr, (size_t)3 * n * 8});
    seg.push_back({c[0].llr.data(), (size_t)n * 8}); seg.push_back({c[1].llr.data(), (size_t)n * 8});
    std::vector<size_t> off(seg.size() + 1, 0);
    for (size_t i = 0; i < seg.size(); ++i) off[i + 1] = off[i] + HugeBp4::al(seg[i].bytes);
    if (h->graph.reserve(off.back())) return nullptr;
    char *d = (char *)h->graph.p;
    for (size_t i = 0; i < seg.size(); ++i)
        if (hipMemcpy(d + off[i], seg[i].src, seg[i].bytes, hipMemcpyHostToDevice) != hipSuccess) { set_error(SWD_ERR_DEVICE, "hipMemcpy of the graph failed"); return nullptr; }
    SwdHugeBp4Args &a = h->tmpl;
    auto ip = [&](int i) { return (const int32_t *)(d + off[i]); };
    a.gx = HugeGraphDev{hx->m, n, ip(0), ip(1), ip(2), ip(3), ip(4), (const double *)(d + off[15])}; a.r2cx = ip(5); a.nodex = ip(6);
    a.gz = HugeGraphDev{hz->m, n, ip(7), ip(8), ip(9), ip(10), ip(11), (const double *)(d + off[16])}; a.r2cz = ip(12); a.nodez = ip(13);
    a.llr_x = (const double *)(d + off[14]); a.llr_y = a.llr_x + n; a.llr_z = a.llr_y + n;
    a.Ex = hx->nnz; a.Ez = hz->nnz;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 64;
    if (bp) {
        const size_t Ex = (size_t)hx->nnz, Ez = (size_t)hz->nnz;
        a.o_b2cx = h->take(Ex * 8); a.o_c2bx = h->take(Ex * 8); a.o_b2cz = h->take(Ez * 8); a.o_c2bz = h->take(Ez * 8);
        a.o_inix = h->take((size_t)n * 8); a.o_iniz = h->take((size_t)n * 8);
        a.o_tx = h->take((size_t)n * 8); a.o_ty = h->take((size_t)n * 8); a.o_tz = h->take((size_t)n * 8);
        a.o_numx = h->take((size_t)n * 8); a.o_numz = h->take((size_t)n * 8);
        a.o_decx = h->take((size_t)n); a.o_decz = h->take((size_t)n); a.o_cnx = h->take((size_t)hx->m); a.o_cnz = h->take((size_t)hz->m);
        a.o_list = h->take((size_t)n * 4);
        a.stride = h->stride;
        // one workgroup per CU, fewer when their slices would pass the slot's bound (the largest graph: 1.1 GB per slice)
        h->grid_max = (int)std::max<int64_t>(1, std::min<int64_t>(std::max(1, cus), HugeBp4::kSlotBytes / h->stride));
    }
    if (osd) {
        SwdHugeBp4OsdArgs &o = h->otmpl;
        o.gx = a.gx; o.gz = a.gz;
        o.rank_x = h->rank_x; o.rank_z = h->rank_z;
        o.osd_method = osd->osd_method; o.osd_order = osd->osd_order;
        // rank(Hx) > rank(Hz): the z-basis sweep walks the first kx = n - rank_x non-pivot columns like the reference's (swd_bp4.hip)
        o.new_n_x = n; o.new_n_z = (osd->osd_order > 0 && h->rank_x > h->rank_z) ? n - h->rank_x + h->rank_z : n;
        int npad = 2; while (npad < n) npad <<= 1;
        o.npad = npad;
        // a slice of the elimination: every array sized for the larger of the two bases
        const int mm = std::max(hx->m, hz->m), wm = (mm + 63) / 64;
        const int kx = std::max(o.new_n_x - h->rank_x, 0), kz = std::max(o.new_n_z - h->rank_z, 0), k = std::max(kx, kz);
        const int nyc = osd->osd_order <= 0 ? 0 : (osd->osd_method == 2 ? k : std::min(k, osd->osd_order));
        const int rk = std::max(h->rank_x, h->rank_z);
        int64_t st = 0;
        auto tk = [&](size_t bytes) { const int64_t at = st; st += (int64_t)HugeBp4::al(bytes); return at; };
        o.o_key = tk((size_t)npad * 8); o.o_idx = tk((size_t)npad * 4);
        o.o_T = tk((size_t)wm * mm * 8); o.o_ycand = tk((size_t)std::max(nyc, 1) * wm * 8); o.o_pm = tk((size_t)(2 * wm + 4) * 8);
        o.o_pc = tk((size_t)(rk + 1) * 4); o.o_pr = tk((size_t)(rk + 1) * 4); o.o_rowof = tk((size_t)n * 4);
        o.o_plist = tk((size_t)std::max(n, mm) * 4); o.o_ht = tk((size_t)(k + 1) * 4); o.o_lv = tk((size_t)n * 4);
        o.o_lc = tk((size_t)std::max(mm, n) * 4); o.o_best = tk(64); o.o_bak = tk((size_t)n); o.o_hard = tk((size_t)n);
        o.stride = st;
        if (st > HugeBp4::kSlotBytes) {
            set_error(SWD_ERR_CAPACITY, "the elimination needs %lld bytes per workgroup, which exceeds the general OSD's limit of %lld bytes (8 GiB) per launch slot",
                      (long long)st, (long long)HugeBp4::kSlotBytes);
            return nullptr;
        }
        h->osd_grid_max = (int)std::max<int64_t>(1, std::min<int64_t>(std::max(1, cus), HugeBp4::kSlotBytes / st));
    }
    return h.release();
}

// ---- diagnostics (include/swd.h: swd_diag_libm, ops 5 / 6): the noinline copies above, one argument (pair) per element ----
__global__ void __launch_bounds__(256) huge_bp4_diag_libm_kernel(int op, int64_t n, const double *x, const double *y, double *out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (op == 5) ? hb_log1pexp(x[i]) : hb_logaddexp(x[i], y[i]);
}

int huge_bp4_diag_libm(int op, int64_t n, const double *x, const double *y, double *out, void *stream) {
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(huge_bp4_diag_libm_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, op, n, x, y, out);
    SWD_HIP(hipGetLastError());
    return 0;
}

} // namespace swd
