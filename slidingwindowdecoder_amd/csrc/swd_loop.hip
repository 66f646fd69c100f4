// Device window loop (include/swd.h: swd_window_loop_*): the loop of the reference harness (/root/reference/osd.py:130-179) for plans
// whose windows no one-launch pipeline kernel takes.  The handle owns one single-window decoder per DISTINCT window (swd_osdw_create /
// swd_gdg_create: a tuned kernel, a large-graph kernel or the general form, whichever the window gets there) and runs, on the caller's
// stream and without a host synchronisation of its own:
//   resid = det, total = 0, observable accumulators = 0                                            (loop_begin_kernel)
//   for every window t:  decode resid[:, row0 : row0 + m] with the window's decoder                (*_decode_batch_dev, strided syndromes)
//                        commit the first `commit` columns, fold their columns of the global check matrix into resid, their
//                        observable masks into the accumulator, scatter the window's record         (loop_commit_kernel)
//   the commit of the last window also reduces "resid != 0" and writes shot_result.
// The residual syndrome is one byte per bit inside 32-bit words (byte r & 3 of word r >> 2), rows padded to a multiple of 4 with zeros.
#include <string.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>

#include "swd_host.h"

namespace swd {

// one workgroup per shot: the residual syndrome takes the detector bits (0 / 1, padding zero), total_e_hat and the accumulator are zeroed
__global__ void __launch_bounds__(256) loop_begin_kernel(const uint8_t *det, int64_t det_stride, int num_det, uint8_t *resid, int64_t res_stride,
                                                         uint8_t *total, int64_t total_stride, int num_col, uint32_t *acc) {
    const int tid = threadIdx.x, b = blockIdx.x;
    const uint8_t *src = det + (int64_t)b * det_stride;
    uint32_t *row32 = (uint32_t *)(resid + (int64_t)b * res_stride);
    for (int q = tid; q < (int)(res_stride >> 2); q += 256) {
        uint32_t x = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * q + j < num_det && src[4 * q + j]) x |= 1u << (8 * j);
        row32[q] = x;
    }
    uint8_t *tot = total + (int64_t)b * total_stride;
    for (int c = tid; c < num_col; c += 256) tot[c] = 0;
    if (tid == 0) acc[b] = 0;
}

struct LoopCommitArgs {
    uint8_t *resid; int64_t res_stride;          // [B][res_stride], res_stride = num_det rounded up to 4
    const uint8_t *est; int64_t est_stride;      // the window's full estimate
    uint8_t *total; int64_t total_stride;        // the caller's total_e_hat
    uint32_t *acc;                               // [B] observable accumulators
    const int32_t *chk_colptr, *chk_rows;        // CSC of the global check matrix
    const uint32_t *obs_mask;                    // [num_col], nullable
    const int32_t *stats_w; const double *pm_w;  // the window decode's records [B][SWD_STAT_WORDS], [B] (pm_w nullable)
    int32_t *stats; double *min_pm; int32_t *shot_result; // the caller's [B][W][SWD_STAT_WORDS], [B][W], [B][2]; all nullable
    int32_t W, t, col0, commit;
    int32_t lo, hi;                              // rows the committed columns reach, whole words: lo, hi multiples of 4
    int32_t num_det, last;
};

// one workgroup per shot.  Only the rows [lo, hi) that the committed columns reach are staged in LDS (one byte per bit inside 32-bit
// words); the committed faults go into total_e_hat, their columns of the check matrix into the staged rows with LDS atomics (as
// window_commit_kernel of the sessions does; osd.py:170-178), their observable masks into the accumulator; the window's record goes
// to [shot][window].  The last window's launch also says whether any row of the residual syndrome is left (osd.py:184-187).
__global__ void __launch_bounds__(256) loop_commit_kernel(const LoopCommitArgs a) {
    extern __shared__ uint32_t sres[];
    __shared__ uint32_t sacc;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int q0 = a.lo >> 2, nq = (a.hi - a.lo) >> 2, span = a.hi - a.lo;
    uint32_t *row32 = (uint32_t *)(a.resid + (int64_t)b * a.res_stride);
    for (int q = tid; q < nq; q += 256) sres[q] = row32[q0 + q];
    if (tid == 0) sacc = 0;
    __syncthreads();
    const uint8_t *est_b = a.est + (int64_t)b * a.est_stride;
    uint8_t *out_b = a.total + (int64_t)b * a.total_stride + a.col0;
    for (int i = tid; i < a.commit; i += 256) {
        const uint8_t hv = est_b[i] ? 1 : 0;
        out_b[i] = hv;
        if (hv) {
            const int c = a.col0 + i;
            if (a.obs_mask) { const uint32_t om = a.obs_mask[c]; if (om) atomicXor(&sacc, om); }
            for (int e = a.chk_colptr[c]; e < a.chk_colptr[c + 1]; ++e) {
                const int r = a.chk_rows[e] - a.lo;
                if ((unsigned)r < (unsigned)span) atomicXor(&sres[r >> 2], 1u << ((r & 3) * 8)); // (always: the span was taken from these columns)
            }
        }
    }
    __syncthreads();
    for (int q = tid; q < nq; q += 256) row32[q0 + q] = sres[q];
    if (a.stats && tid < SWD_STAT_WORDS) a.stats[((int64_t)b * a.W + a.t) * SWD_STAT_WORDS + tid] = a.stats_w[(int64_t)b * SWD_STAT_WORDS + tid];
    if (a.min_pm && tid == 0) a.min_pm[(int64_t)b * a.W + a.t] = a.pm_w[b];
    int any = 0;
    if (a.last) {
        int nz = 0;
        for (int q = tid; q < (int)(a.res_stride >> 2); q += 256) nz |= ((unsigned)(q - q0) < (unsigned)nq ? sres[q - q0] : row32[q]) != 0u;
        any = __syncthreads_or(nz);
    }
    if (tid == 0) {
        const uint32_t ac = a.acc[b] ^ sacc;
        a.acc[b] = ac;
        if (a.last && a.shot_result) { a.shot_result[2 * b] = (int32_t)ac; a.shot_result[2 * b + 1] = any ? 1 : 0; }
    }
}

constexpr int LOOP_MAX_SPAN = 65536; // rows one commit stages: 64 KB of LDS

struct LoopWindow {
    int dec = 0;                          // index into WindowLoop::decs
    int m = 0, n = 0, row0 = 0, col0 = 0, commit = 0;
    int lo = 0, hi = 0;                   // committed-row span, whole words
};

struct WindowLoop {
    int device = 0, kind = 0;             // kind: 0 osd_window, 1 guessing family
    int num_det = 0, num_col = 0, nmax = 0;
    int64_t res_stride = 0;
    std::vector<LoopWindow> wins;
    std::vector<void *> decs;             // swd_osdw* / swd_gdg*, one per distinct window
    DevBuf graph;                         // [ col_ptr | row_idx | obs_mask ]
    const int32_t *d_colptr = nullptr, *d_rows = nullptr;
    const uint32_t *d_obs = nullptr;
    DevBuf resid, est, acc, stats_w, pm_w; // grow with B
    DevBuf io;                            // the host-buffer entry point's device arrays
    std::mutex mu;
    hipEvent_t ev = nullptr;              // recorded behind the last kernel of a decode: a decode on another stream waits for it
    hipStream_t last = nullptr;
    bool ev_set = false;

    ~WindowLoop() {
        for (void *d : decs)
            if (kind == 0) swd_osdw_destroy((swd_osdw *)d); else swd_gdg_destroy((swd_gdg *)d);
        if (ev) (void)hipEventDestroy(ev);
    }
    size_t device_bytes() const { return graph.cap + resid.cap + est.cap + acc.cap + stats_w.cap + pm_w.cap + io.cap; }
};

// what makes two windows the same decoder: the matrix (rows sorted) and the priors; new_n is one parameter of the whole loop
static std::string window_key(const swd_graph_desc &g) {
    std::vector<int32_t> ci(g.col_idx, g.col_idx + g.nnz);
    for (int r = 0; r < g.m; ++r) std::sort(ci.begin() + g.row_ptr[r], ci.begin() + g.row_ptr[r + 1]);
    std::string k;
    k.append((const char *)&g.m, 4).append((const char *)&g.n, 4).append((const char *)&g.nnz, 4);
    k.append((const char *)g.row_ptr, (size_t)(g.m + 1) * 4).append((const char *)ci.data(), ci.size() * 4);
    k.append((const char *)g.channel_probs, (size_t)g.n * 8);
    return k;
}

static int loop_check_graph(const swd_graph_desc *g, const char *what) {
    if (!g->row_ptr || !g->col_idx || g->m <= 0 || g->n <= 0 || g->nnz < 0 || g->row_ptr[0] != 0 || g->row_ptr[g->m] != g->nnz) {
        set_error(SWD_ERR_VALUE, "%s: empty or inconsistent matrix", what);
        return -1;
    }
    for (int r = 0; r < g->m; ++r)
        if (g->row_ptr[r] > g->row_ptr[r + 1]) { set_error(SWD_ERR_VALUE, "%s: row_ptr is not monotone", what); return -1; }
    for (int e = 0; e < g->nnz; ++e)
        if (g->col_idx[e] < 0 || g->col_idx[e] >= g->n) { set_error(SWD_ERR_VALUE, "%s: column out of range", what); return -1; }
    return 0;
}

static int loop_decode_dev(WindowLoop *l, int32_t B, const uint8_t *det, int64_t det_stride, uint8_t *total, int64_t total_stride,
                           int32_t *stats, double *min_pm, int32_t *shot_result, hipStream_t st) {
    SWD_HIP(hipSetDevice(l->device));
    if (l->resid.reserve((size_t)B * l->res_stride) || l->est.reserve((size_t)B * l->nmax) || l->acc.reserve((size_t)B * 4) ||
        l->stats_w.reserve((size_t)B * SWD_STAT_WORDS * 4) || (min_pm && l->pm_w.reserve((size_t)B * 8)))
        return -1;
    // the handle's buffers are shared by its decodes: one on another stream than the previous one starts behind it
    if (l->ev_set && l->last != st) SWD_HIP(hipStreamWaitEvent(st, l->ev, 0));
    uint8_t *resid = l->resid.as<uint8_t>();
    hipLaunchKernelGGL(loop_begin_kernel, dim3(B), dim3(256), 0, st, det, det_stride ? det_stride : (int64_t)l->num_det, l->num_det, resid,
                       l->res_stride, total, total_stride ? total_stride : (int64_t)l->num_col, l->num_col, l->acc.as<uint32_t>());
    SWD_HIP(hipGetLastError());
    int rc = 0;
    const int W = (int)l->wins.size();
    for (int t = 0; t < W && !rc; ++t) {
        const LoopWindow &w = l->wins[t];
        int32_t *sw = l->stats_w.as<int32_t>();
        double *pw = min_pm ? l->pm_w.as<double>() : nullptr;
        rc = l->kind == 0 ? swd_osdw_decode_batch_dev((swd_osdw *)l->decs[w.dec], B, resid + w.row0, l->res_stride, l->est.as<uint8_t>(), w.n, sw, pw,
                                                      nullptr, 0, nullptr, nullptr, st)
                          : swd_gdg_decode_batch_dev((swd_gdg *)l->decs[w.dec], B, resid + w.row0, l->res_stride, l->est.as<uint8_t>(), w.n, sw, pw, st);
        if (rc) break;
        LoopCommitArgs c{};
        c.resid = resid; c.res_stride = l->res_stride;
        c.est = l->est.as<uint8_t>(); c.est_stride = w.n;
        c.total = total; c.total_stride = total_stride ? total_stride : (int64_t)l->num_col;
        c.acc = l->acc.as<uint32_t>();
        c.chk_colptr = l->d_colptr; c.chk_rows = l->d_rows; c.obs_mask = l->d_obs;
        c.stats_w = sw; c.pm_w = pw;
        c.stats = stats; c.min_pm = min_pm; c.shot_result = shot_result;
        c.W = W; c.t = t; c.col0 = w.col0; c.commit = w.commit; c.lo = w.lo; c.hi = w.hi;
        c.num_det = l->num_det; c.last = t + 1 == W ? 1 : 0;
        hipLaunchKernelGGL(loop_commit_kernel, dim3(B), dim3(256), (size_t)(w.hi - w.lo), st, c);
        if (hipGetLastError() != hipSuccess) { set_error(SWD_ERR_DEVICE, "window loop: the commit launch of window %d failed", t); rc = -1; }
    }
    // (also after a failure: kernels may be queued that use the buffers)
    if (hipEventRecord(l->ev, st) == hipSuccess) { l->ev_set = true; l->last = st; }
    return rc;
}

} // namespace swd

using namespace swd;

extern "C" swd_window_loop *swd_window_loop_create(int32_t num_windows, const swd_window_desc *wins, const swd_graph_desc *chk,
                                                   const swd_graph_desc *obs, int32_t decoder, const void *params, int device) {
    if (!wins || !chk || !params || num_windows <= 0) { set_error("null argument"); return nullptr; }
    if (decoder != 0 && decoder != 1) { set_error(SWD_ERR_VALUE, "window loop: decoder %d (0 = osd_window, 1 = guessing family)", decoder); return nullptr; }
    if (loop_check_graph(chk, "window loop: global check matrix")) return nullptr;
    if (obs) {
        if (loop_check_graph(obs, "window loop: observable matrix")) return nullptr;
        if (obs->m > 32) { set_error("at most 32 observables are supported (got %d)", obs->m); return nullptr; }
        if (obs->n != chk->n) { set_error(SWD_ERR_VALUE, "observable matrix has %d columns, expected %d", obs->n, chk->n); return nullptr; }
    }
    std::unique_ptr<WindowLoop> l(new WindowLoop());
    l->device = device; l->kind = decoder;
    l->num_det = chk->m; l->num_col = chk->n;
    l->res_stride = ((int64_t)chk->m + 3) & ~(int64_t)3;
    // CSC of the global check matrix, int32 rows
    const int n = chk->n;
    std::vector<int32_t> col_ptr(n + 1, 0), row_idx((size_t)chk->nnz);
    for (int e = 0; e < chk->nnz; ++e) col_ptr[chk->col_idx[e] + 1]++;
    for (int c = 0; c < n; ++c) col_ptr[c + 1] += col_ptr[c];
    {
        std::vector<int32_t> at(col_ptr.begin(), col_ptr.end() - 1);
        for (int r = 0; r < chk->m; ++r)
            for (int e = chk->row_ptr[r]; e < chk->row_ptr[r + 1]; ++e) row_idx[at[chk->col_idx[e]]++] = r;
    }
    std::map<std::string, int> seen;
    for (int t = 0; t < num_windows; ++t) {
        const swd_window_desc &wd = wins[t];
        const swd_graph_desc &g = wd.graph;
        if (!g.row_ptr || !g.col_idx || !g.channel_probs || g.m <= 0 || g.n <= 0 || g.nnz <= 0 || g.row_ptr[0] != 0 || g.row_ptr[g.m] != g.nnz) {
            set_error(SWD_ERR_VALUE, "window %d: empty or inconsistent check matrix", t);
            return nullptr;
        }
        if (wd.row0 < 0 || (int64_t)wd.row0 + g.m > chk->m || wd.col0 < 0 || wd.commit < 0 || wd.commit > g.n || (int64_t)wd.col0 + wd.commit > n) {
            set_error(SWD_ERR_VALUE, "window %d: rows [%d, %d) / committed columns [%d, %d) lie outside the %d x %d check matrix or the window's %d columns",
                      t, wd.row0, wd.row0 + g.m, wd.col0, wd.col0 + wd.commit, chk->m, n, g.n);
            return nullptr;
        }
        for (int r = 0; r < g.m; ++r)
            if (g.row_ptr[r] > g.row_ptr[r + 1]) { set_error(SWD_ERR_VALUE, "window %d: row_ptr is not monotone", t); return nullptr; }
        LoopWindow w;
        w.m = g.m; w.n = g.n; w.row0 = wd.row0; w.col0 = wd.col0; w.commit = wd.commit;
        int lo = chk->m, hi = 0;
        for (int e = col_ptr[wd.col0]; e < col_ptr[wd.col0 + wd.commit]; ++e) { lo = std::min(lo, row_idx[e]); hi = std::max(hi, row_idx[e] + 1); }
        if (hi <= lo) lo = hi = 0;
        w.lo = lo & ~3; w.hi = (hi + 3) & ~3;
        if (w.hi - w.lo > LOOP_MAX_SPAN) {
            set_error(SWD_ERR_CAPACITY, "window %d: its committed columns reach rows %d..%d, the commit stages at most %d rows", t, lo, hi - 1, LOOP_MAX_SPAN);
            return nullptr;
        }
        const auto ins = seen.emplace(window_key(g), (int)l->decs.size());
        if (ins.second) {
            void *d = decoder == 0 ? (void *)swd_osdw_create(&g, (const swd_osdw_params *)params, device)
                                   : (void *)swd_gdg_create(&g, (const swd_gdg_params *)params, device);
            if (!d) { // that create's class and message stand, with the window in front
                const std::string msg = last_error();
                set_error(last_error_class(), "window %d: %s", t, msg.c_str());
                return nullptr;
            }
            l->decs.push_back(d);
        }
        w.dec = ins.first->second;
        l->nmax = std::max(l->nmax, g.n);
        l->wins.push_back(w);
    }
    if (hipSetDevice(device) != hipSuccess) { set_error(SWD_ERR_DEVICE, "hipSetDevice(%d) failed", device); return nullptr; }
    std::vector<uint32_t> mask;
    if (obs) {
        mask.assign(n, 0);
        for (int k = 0; k < obs->m; ++k)
            for (int e = obs->row_ptr[k]; e < obs->row_ptr[k + 1]; ++e) mask[obs->col_idx[e]] ^= 1u << k;
    }
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_rows = al((size_t)(n + 1) * 4), o_obs = o_rows + al(row_idx.size() * 4), bytes = o_obs + al(mask.size() * 4);
    if (l->graph.reserve(bytes)) return nullptr;
    char *dv = (char *)l->graph.p;
    if (hipMemcpy(dv, col_ptr.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice) != hipSuccess ||
        (!row_idx.empty() && hipMemcpy(dv + o_rows, row_idx.data(), row_idx.size() * 4, hipMemcpyHostToDevice) != hipSuccess) ||
        (!mask.empty() && hipMemcpy(dv + o_obs, mask.data(), mask.size() * 4, hipMemcpyHostToDevice) != hipSuccess)) {
        set_error(SWD_ERR_DEVICE, "window loop: hipMemcpy of the check matrix failed");
        return nullptr;
    }
    l->d_colptr = (const int32_t *)dv; l->d_rows = (const int32_t *)(dv + o_rows);
    l->d_obs = mask.empty() ? nullptr : (const uint32_t *)(dv + o_obs);
    if (hipEventCreateWithFlags(&l->ev, hipEventDisableTiming) != hipSuccess) { set_error(SWD_ERR_DEVICE, "window loop: hipEventCreate failed"); return nullptr; }
    {   // the LDS limit belongs to the function: up to LOOP_MAX_SPAN staged rows against the default limit's 48 KB
        static std::mutex attr_mu;
        std::lock_guard<std::mutex> lk(attr_mu);
        (void)hipFuncSetAttribute((const void *)loop_commit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LOOP_MAX_SPAN);
    }
    return (swd_window_loop *)l.release();
}

extern "C" void swd_window_loop_destroy(swd_window_loop *h) {
    WindowLoop *l = (WindowLoop *)h;
    if (!l) return;
    (void)hipSetDevice(l->device);
    if (l->ev_set) (void)hipEventSynchronize(l->ev); // the buffers may still be in use
    delete l;
}

extern "C" int swd_window_loop_info(const swd_window_loop *h, int32_t *num_windows, int32_t *num_det, int32_t *num_col,
                                    int32_t *distinct_decoders, int64_t *device_bytes) {
    const WindowLoop *l = (const WindowLoop *)h;
    if (!l) { set_error("null window loop"); return -1; }
    if (num_windows) *num_windows = (int32_t)l->wins.size();
    if (num_det) *num_det = l->num_det;
    if (num_col) *num_col = l->num_col;
    if (distinct_decoders) *distinct_decoders = (int32_t)l->decs.size();
    if (device_bytes) *device_bytes = (int64_t)l->device_bytes();
    return 0;
}

extern "C" int swd_window_loop_decode_dev(swd_window_loop *h, int32_t B, const uint8_t *det, int64_t det_stride, uint8_t *total,
                                          int64_t total_stride, int32_t *stats, double *min_pm, int32_t *shot_result, void *stream) {
    WindowLoop *l = (WindowLoop *)h;
    if (!l) { set_error("null window loop"); return -1; }
    if (B <= 0) return 0;
    if (!det || !total) { set_error("null output/input pointer"); return -1; }
    std::lock_guard<std::mutex> lk(l->mu);
    return loop_decode_dev(l, B, det, det_stride, total, total_stride, stats, min_pm, shot_result, (hipStream_t)stream);
}

extern "C" int swd_window_loop_decode(swd_window_loop *h, int32_t B, const uint8_t *det, uint8_t *total, int32_t *stats, double *min_pm,
                                      int32_t *shot_result) {
    WindowLoop *l = (WindowLoop *)h;
    if (!l) { set_error("null window loop"); return -1; }
    if (B <= 0) return 0;
    if (!det || !total) { set_error("null output/input pointer"); return -1; }
    std::lock_guard<std::mutex> lk(l->mu);
    SWD_HIP(hipSetDevice(l->device));
    const size_t W = l->wins.size();
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t n_det = (size_t)B * l->num_det, n_tot = (size_t)B * l->num_col, n_st = (size_t)B * W * SWD_STAT_WORDS * 4, n_pm = (size_t)B * W * 8,
                 n_sr = (size_t)B * 8;
    const size_t o_tot = al(n_det), o_st = o_tot + al(n_tot), o_pm = o_st + al(n_st), o_sr = o_pm + al(n_pm), bytes = o_sr + al(n_sr);
    if (l->io.reserve(bytes)) return -1;
    char *dv = (char *)l->io.p;
    hipStream_t st = nullptr;
    SWD_HIP(hipMemcpyAsync(dv, det, n_det, hipMemcpyHostToDevice, st));
    if (loop_decode_dev(l, B, (const uint8_t *)dv, 0, (uint8_t *)(dv + o_tot), 0, stats ? (int32_t *)(dv + o_st) : nullptr,
                        min_pm ? (double *)(dv + o_pm) : nullptr, shot_result ? (int32_t *)(dv + o_sr) : nullptr, st))
        return -1;
    SWD_HIP(hipMemcpyAsync(total, dv + o_tot, n_tot, hipMemcpyDeviceToHost, st));
    if (stats) SWD_HIP(hipMemcpyAsync(stats, dv + o_st, n_st, hipMemcpyDeviceToHost, st));
    if (min_pm) SWD_HIP(hipMemcpyAsync(min_pm, dv + o_pm, n_pm, hipMemcpyDeviceToHost, st));
    if (shot_result) SWD_HIP(hipMemcpyAsync(shot_result, dv + o_sr, n_sr, hipMemcpyDeviceToHost, st));
    SWD_HIP(hipStreamSynchronize(st));
    return 0;
}
