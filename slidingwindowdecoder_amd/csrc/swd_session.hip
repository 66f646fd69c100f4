// Online sessions of the sliding-window pipeline (include/swd.h: swd_pipeline_session_*): the window loop of the reference harness
// (/root/reference/osd.py:130-179) driven by the ARRIVAL of detector rows.  A session keeps, for one batch of shots, the residual
// syndrome, total_e_hat, the observable accumulators and the per-window records on the device between calls:
//   arrival of rows [r, r + k):  resid[:, r : r + k] ^= rows                                  (session_merge_kernel)
//   window t ready (rows received >= its last row, window t - 1 committed):
//       decode it on resid[:, row0 : row1]     -- the plan's own pipeline kernel, launched for window t alone as a pipeline of length 1
//       commit the first `commit` columns, XOR their columns of the global check matrix into resid -- rows that have not arrived
//       yet included -- and their observable masks into the accumulator                        (session_commit_kernel)
//   after the last window: flagged = resid != 0, records transposed to [shot][window]          (session_finish_kernel)
// The window loop is causal (window t reads rows < row1 of det ^ chk @ total_e_hat only) and XOR commutes, so every result equals the
// one-launch decode's whatever the chunking.  The residual syndrome is one byte per bit inside 32-bit words, as in the decode
// kernels' LDS copy and state record (byte r & 3 of word r >> 2).
#include <mutex>

#include "swd_plan.h"

namespace swd {

// thread = one 32-bit word of one shot's residual syndrome that the arriving rows [r, r + k) touch (r, k: any values)
__global__ void __launch_bounds__(256) session_merge_kernel(uint8_t *resid, int64_t res_stride, const uint8_t *in, int64_t in_stride,
                                                            int B, int r, int k) {
    const int q0 = r >> 2, nq = ((r + k - 1) >> 2) - q0 + 1;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)B * nq) return;
    const int b = (int)(t / nq), q = q0 + (int)(t - (long long)b * nq);
    const uint8_t *src = in + (int64_t)b * in_stride;
    uint32_t x = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 4 * q + j;
        if (row >= r && row < r + k && src[row - r]) x |= 1u << (8 * j);
    }
    if (x) ((uint32_t *)(resid + (int64_t)b * res_stride))[q] ^= x;
}

struct SessionCommitArgs {
    uint8_t *resid; int64_t res_stride;
    const uint8_t *est; int64_t est_stride;   // the window's full estimate (win_out of the decode launch)
    uint8_t *total; int64_t total_stride;
    uint32_t *acc;                            // [B] observable accumulators
    const uint32_t *chk_colptr; const uint16_t *chk_rows; const uint32_t *obs_mask;
    int32_t num_det, col0, commit;
};

// one workgroup per shot: the shot's residual words staged in LDS, the committed faults' columns of the global check matrix folded in
// with LDS atomics (as the epilogue of pipeline_kernel does), written back whole (osd.py:170-178)
__global__ void __launch_bounds__(256) session_commit_kernel(const SessionCommitArgs a) {
    extern __shared__ uint32_t sres[];
    __shared__ uint32_t sacc;
    const int tid = threadIdx.x, b = blockIdx.x, nw = (a.num_det + 3) >> 2;
    uint32_t *res32 = (uint32_t *)(a.resid + (int64_t)b * a.res_stride);
    for (int q = tid; q < nw; q += 256) sres[q] = res32[q];
    if (tid == 0) sacc = 0;
    __syncthreads();
    const uint8_t *est_b = a.est + (int64_t)b * a.est_stride;
    uint8_t *tot_b = a.total + (int64_t)b * a.total_stride + a.col0;
    for (int i = tid; i < a.commit; i += 256) {
        const uint8_t hv = est_b[i];
        tot_b[i] = hv;
        if (hv) {
            const int c = a.col0 + i;
            if (a.obs_mask) { const uint32_t om = a.obs_mask[c]; if (om) atomicXor(&sacc, om); }
            for (uint32_t e = a.chk_colptr[c]; e < a.chk_colptr[c + 1]; ++e) {
                const int r = a.chk_rows[e];
                atomicXor(&sres[r >> 2], 1u << ((r & 3) * 8));
            }
        }
    }
    __syncthreads();
    for (int q = tid; q < nw; q += 256) res32[q] = sres[q];
    if (tid == 0 && sacc) a.acc[b] ^= sacc;
}

// one workgroup per shot: shot_result as swd_pipeline_decode returns it (osd.py:184-187), the per-window records [t][shot] -> [shot][t]
__global__ void __launch_bounds__(256) session_finish_kernel(const uint8_t *resid, int64_t res_stride, int num_det, const uint32_t *acc,
                                                             const int32_t *stats_w, const double *pm_w, int64_t wstride, int W,
                                                             int32_t *stats, double *min_pm, int32_t *shot_result) {
    const int tid = threadIdx.x, b = blockIdx.x, nw = (num_det + 3) >> 2;
    const uint32_t *res32 = (const uint32_t *)(resid + (int64_t)b * res_stride);
    int nz = 0;
    for (int q = tid; q < nw; q += 256) nz |= res32[q] != 0u;
    const int any = __syncthreads_or(nz);
    if (tid == 0) { shot_result[2 * b] = (int32_t)acc[b]; shot_result[2 * b + 1] = any ? 1 : 0; }
    for (int i = tid; i < W * SWD_STAT_WORDS; i += 256) {
        const int t = i / SWD_STAT_WORDS, k = i % SWD_STAT_WORDS;
        stats[((int64_t)b * W + t) * SWD_STAT_WORDS + k] = stats_w[((int64_t)t * wstride + b) * SWD_STAT_WORDS + k];
    }
    for (int t = tid; t < W; t += 256) min_pm[(int64_t)b * W + t] = pm_w[(int64_t)t * wstride + b];
}

// the plan a session call works on; NULL (with a message) once the pipeline has been destroyed
static Plan *session_plan(Session *s) {
    if (!s->plan) set_error("the pipeline of this session has been destroyed");
    return s->plan;
}

// rows that must have arrived before window t is decoded: its last row; the last window closes the experiment and waits for every row
static int session_need(const Plan *d, int t) {
    return t + 1 == (int)d->wins.size() ? d->num_det : d->wins[t].row0 + d->wins[t].g->m;
}

// work on the state is ordered by one event: a call on another stream than the previous one waits for it first
static int session_enter(Session *s, hipStream_t st) {
    if (s->ev_set && s->last != st) SWD_HIP(hipStreamWaitEvent(st, s->ev, 0));
    return 0;
}
static int session_leave(Session *s, hipStream_t st) {
    SWD_HIP(hipEventRecord(s->ev, st));
    s->ev_set = true; s->last = st;
    return 0;
}

static int session_push_dev(Session *s, int32_t nrows, const uint8_t *det_rows, int64_t stride, int32_t *first, int32_t *count, hipStream_t st) {
    Plan *d = session_plan(s);
    if (!d) return -1;
    const int W = s->W;
    if (!s->B) { set_error("session push: call swd_pipeline_session_begin first"); return -1; }
    if (s->done == W) { set_error("session push: the last window has been committed (all %d rows received); finish or begin a new batch", s->rows); return -1; }
    if (nrows < 0 || s->rows + (int64_t)nrows > s->num_det) {
        set_error("session push: %d rows after %d received, the experiment has %d detector rows", nrows, s->rows, s->num_det);
        return -1;
    }
    if (nrows > 0 && !det_rows) { set_error("null input pointer"); return -1; }
    SWD_HIP(hipSetDevice(d->device));
    if (session_enter(s, st)) return -1;
    char *dv = (char *)s->dev.p;
    const int B = s->B;
    if (nrows > 0) {
        const long long nthr = (long long)B * (((s->rows + nrows - 1) >> 2) - (s->rows >> 2) + 1);
        hipLaunchKernelGGL(session_merge_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, (uint8_t *)dv, s->res_stride, det_rows,
                           stride ? stride : (int64_t)nrows, B, s->rows, nrows);
        SWD_HIP(hipGetLastError());
        s->rows += nrows;
    }
    const int first_w = s->done;
    int rc = 0;
    while (s->done < W && s->rows >= session_need(d, s->done)) {
        const int t = s->done;
        const WindowHost &w = d->wins[t];
        // the window decode: the plan's kernel on window t alone -- a pipeline of length 1 whose `det` is the residual syndrome (the
        // kernel's window-0 path reads absolute rows row0..), full estimate through win_out, nothing committed by the kernel
        SwdPipeArgs a{};
        a.wins = d->d_wins.as<SwdWindowDev>() + t; a.W = 1; a.B = B;
        a.slot_scratch = 1;
        fill_params(d, a.P, false, false);
        a.det = (const uint8_t *)dv; a.det_stride = s->res_stride; a.num_det = d->num_det; a.off_det = d->off_det;
        a.total = nullptr; a.win_out = (uint8_t *)(dv + s->o_est); a.win_out_stride = s->est_stride;
        a.stats = (int32_t *)(dv + s->o_stats) + (size_t)t * s->max_shots * SWD_STAT_WORDS;
        a.min_pm = (double *)(dv + s->o_pm) + (size_t)t * s->max_shots;
        a.hist = nullptr; a.hist_stride = 4 * (int64_t)d->nmax;
        if ((rc = launch(d, a, st)) != 0) break;
        SessionCommitArgs c{};
        c.resid = (uint8_t *)dv; c.res_stride = s->res_stride;
        c.est = (const uint8_t *)(dv + s->o_est); c.est_stride = s->est_stride;
        c.total = (uint8_t *)(dv + s->o_total); c.total_stride = s->num_col;
        c.acc = (uint32_t *)(dv + s->o_acc);
        c.chk_colptr = d->d_colptr; c.chk_rows = d->d_rows; c.obs_mask = d->d_obs.p ? d->d_obs.as<uint32_t>() : nullptr;
        c.num_det = s->num_det; c.col0 = w.col0; c.commit = w.commit;
        hipLaunchKernelGGL(session_commit_kernel, dim3(B), dim3(256), (size_t)((s->num_det + 3) / 4) * 4, st, c);
        SWD_HIP(hipGetLastError());
        s->done++;
    }
    if (session_leave(s, st)) return -1;
    if (first) *first = first_w;
    if (count) *count = s->done - first_w;
    return rc;
}

} // namespace swd

using namespace swd;

extern "C" swd_session *swd_pipeline_session_create(swd_pipeline *h, int32_t max_shots) {
    Plan *d = (Plan *)h;
    if (!d) { set_error("null pipeline"); return nullptr; }
    if (d->wins.empty() || d->num_col <= 0) { set_error("a session needs a sliding-window pipeline"); return nullptr; }
    if (max_shots <= 0) { set_error("max_shots must be positive"); return nullptr; }
    if (hipSetDevice(d->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", d->device); return nullptr; }
    Session *s = new Session();
    s->plan = d; s->device = d->device; s->max_shots = max_shots;
    s->W = (int)d->wins.size(); s->num_det = d->num_det; s->num_col = d->num_col;
    s->est_stride = align_up(d->nmax, 16);
    s->res_stride = align_up(d->num_det, 16);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t B = (size_t)max_shots, W = (size_t)s->W;
    s->o_total = al(B * s->res_stride);
    s->o_est = s->o_total + al(B * s->num_col);
    s->o_acc = s->o_est + al(B * s->est_stride);
    s->o_stats = s->o_acc + al(B * 4);
    s->o_pm = s->o_stats + al(W * B * SWD_STAT_WORDS * 4);
    s->o_fin = s->o_pm + al(W * B * 8);
    s->f_pm = al(B * W * SWD_STAT_WORDS * 4);
    s->f_shot = s->f_pm + al(B * W * 8);
    s->fin_bytes = s->f_shot + al(B * 8);
    s->o_in = s->o_fin + s->fin_bytes;
    if (s->dev.reserve(s->o_in + al(B * s->num_det)) || hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev, hipEventDisableTiming) != hipSuccess) {
        if (s->dev.p) set_error("session: stream / event creation failed");
        delete s;
        return nullptr;
    }
    static std::mutex attr_mu; // (the attribute belongs to the function: a residual syndrome of up to 65 535 rows, one word per four)
    {
        std::lock_guard<std::mutex> lk(attr_mu);
        (void)hipFuncSetAttribute((const void *)session_commit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    }
    { std::lock_guard<std::recursive_mutex> lk(d->mu); d->sessions.push_back(s); }
    return (swd_session *)s;
}

extern "C" void swd_pipeline_session_destroy(swd_session *h) {
    Session *s = (Session *)h;
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (Plan *d = s->plan) { // (a session whose pipeline went first was detached by ~Plan and only frees its own buffers)
        std::lock_guard<std::recursive_mutex> lk(d->mu);
        d->sessions.erase(std::remove(d->sessions.begin(), d->sessions.end(), s), d->sessions.end());
    }
    delete s;
}

extern "C" int swd_pipeline_session_begin(swd_session *h, int32_t B) {
    Session *s = (Session *)h;
    if (!s) { set_error("null session"); return -1; }
    std::lock_guard<std::mutex> lk(s->mu);
    Plan *d = session_plan(s);
    if (!d) return -1;
    if (B <= 0 || B > s->max_shots) { set_error("session begin: %d shots, the session was created for 1..%d", B, s->max_shots); return -1; }
    SWD_HIP(hipSetDevice(d->device));
    if (session_enter(s, s->st)) return -1;
    // zero residual syndrome, total_e_hat and accumulators of the batch's shots
    SWD_HIP(hipMemsetAsync(s->dev.p, 0, (size_t)B * s->res_stride, s->st));
    SWD_HIP(hipMemsetAsync((char *)s->dev.p + s->o_total, 0, (size_t)B * s->num_col, s->st));
    SWD_HIP(hipMemsetAsync((char *)s->dev.p + s->o_acc, 0, (size_t)B * 4, s->st));
    s->B = B; s->rows = 0; s->done = 0;
    return session_leave(s, s->st);
}

extern "C" int swd_pipeline_session_push_dev(swd_session *h, int32_t nrows, const uint8_t *det_rows, int64_t stride, int32_t *first,
                                             int32_t *count, void *stream) {
    Session *s = (Session *)h;
    if (!s) { set_error("null session"); return -1; }
    std::lock_guard<std::mutex> lk(s->mu);
    return session_push_dev(s, nrows, det_rows, stride, first, count, (hipStream_t)stream);
}

extern "C" int swd_pipeline_session_push(swd_session *h, int32_t nrows, const uint8_t *det_rows, int32_t *first, int32_t *count) {
    Session *s = (Session *)h;
    if (!s) { set_error("null session"); return -1; }
    std::lock_guard<std::mutex> lk(s->mu);
    Plan *d = session_plan(s);
    if (!d) return -1;
    const uint8_t *src = nullptr;
    if (nrows > 0 && det_rows && s->B && s->done < s->W && s->rows + (int64_t)nrows <= s->num_det) { // (anything else: session_push_dev refuses it with its message)
        SWD_HIP(hipSetDevice(d->device));
        // the call is synchronous, so the page-locked block is free here: rows in, one copy to the device
        const size_t bytes = (size_t)s->B * nrows;
        if (s->hin.reserve(bytes)) return -1;
        memcpy(s->hin.p, det_rows, bytes);
        if (session_enter(s, s->st)) return -1;
        SWD_HIP(hipMemcpyAsync((char *)s->dev.p + s->o_in, s->hin.p, bytes, hipMemcpyHostToDevice, s->st));
        if (session_leave(s, s->st)) return -1;
        src = (const uint8_t *)s->dev.p + s->o_in;
    }
    const int rc = session_push_dev(s, nrows, src ? src : det_rows, 0, first, count, s->st); // (det_rows itself only on the refused paths)
    if (rc) return rc;
    SWD_HIP(hipStreamSynchronize(s->st));
    return 0;
}

// device -> host through the page-locked block, after everything queued on the session's state
static int session_fetch(Session *s, size_t dev_off, size_t bytes) {
    if (s->hout.reserve(std::max(bytes, (size_t)4096))) return -1;
    if (session_enter(s, s->st)) return -1;
    SWD_HIP(hipMemcpyAsync(s->hout.p, (const char *)s->dev.p + dev_off, bytes, hipMemcpyDeviceToHost, s->st));
    if (session_leave(s, s->st)) return -1;
    SWD_HIP(hipStreamSynchronize(s->st));
    return 0;
}

extern "C" int swd_pipeline_session_window(swd_session *h, int32_t t, uint8_t *faults, int32_t *stats, double *min_pm) {
    Session *s = (Session *)h;
    if (!s) { set_error("null session"); return -1; }
    std::lock_guard<std::mutex> lk(s->mu);
    Plan *d = session_plan(s);
    if (!d) return -1;
    if (t < 0 || t >= s->done) { set_error("session window: window %d has not been committed (%d of %d are)", t, s->done, s->W); return -1; }
    SWD_HIP(hipSetDevice(d->device));
    const size_t B = (size_t)s->B;
    const WindowHost &w = d->wins[t];
    if (faults && w.commit > 0) { // the committed columns are never written again: read them out of total_e_hat
        if (session_enter(s, s->st)) return -1;
        SWD_HIP(hipMemcpy2DAsync(faults, (size_t)w.commit, (const char *)s->dev.p + s->o_total + w.col0, (size_t)s->num_col, (size_t)w.commit, B,
                                 hipMemcpyDeviceToHost, s->st));
        if (session_leave(s, s->st)) return -1;
        SWD_HIP(hipStreamSynchronize(s->st));
    }
    if (stats) {
        if (session_fetch(s, s->o_stats + (size_t)t * s->max_shots * SWD_STAT_WORDS * 4, B * SWD_STAT_WORDS * 4)) return -1;
        memcpy(stats, s->hout.p, B * SWD_STAT_WORDS * 4);
    }
    if (min_pm) {
        if (session_fetch(s, s->o_pm + (size_t)t * s->max_shots * 8, B * 8)) return -1;
        memcpy(min_pm, s->hout.p, B * 8);
    }
    return 0;
}

extern "C" int swd_pipeline_session_finish(swd_session *h, uint8_t *total, int32_t *stats, double *min_pm, int32_t *shot_result) {
    Session *s = (Session *)h;
    if (!s) { set_error("null session"); return -1; }
    std::lock_guard<std::mutex> lk(s->mu);
    Plan *d = session_plan(s);
    if (!d) return -1;
    if (!s->B) { set_error("session finish: call swd_pipeline_session_begin first"); return -1; }
    if (s->done < s->W) {
        set_error("session finish: window %d of %d waits for detector rows %d..%d (%d of %d received)", s->done, s->W, s->rows,
                  session_need(d, s->done) - 1, s->rows, s->num_det);
        return -1;
    }
    SWD_HIP(hipSetDevice(d->device));
    char *dv = (char *)s->dev.p;
    const size_t B = (size_t)s->B, W = (size_t)s->W;
    if (session_enter(s, s->st)) return -1;
    hipLaunchKernelGGL(session_finish_kernel, dim3((unsigned)B), dim3(256), 0, s->st, (const uint8_t *)dv, s->res_stride, s->num_det,
                       (const uint32_t *)(dv + s->o_acc), (const int32_t *)(dv + s->o_stats), (const double *)(dv + s->o_pm),
                       (int64_t)s->max_shots, s->W, (int32_t *)(dv + s->o_fin), (double *)(dv + s->o_fin + s->f_pm),
                       (int32_t *)(dv + s->o_fin + s->f_shot));
    SWD_HIP(hipGetLastError());
    if (total) SWD_HIP(hipMemcpyAsync(total, dv + s->o_total, B * s->num_col, hipMemcpyDeviceToHost, s->st));
    if (session_leave(s, s->st)) return -1;
    if (session_fetch(s, s->o_fin, s->fin_bytes)) return -1;
    const char *ho = (const char *)s->hout.p;
    if (stats) memcpy(stats, ho, B * W * SWD_STAT_WORDS * 4);
    if (min_pm) memcpy(min_pm, ho + s->f_pm, B * W * 8);
    if (shot_result) memcpy(shot_result, ho + s->f_shot, B * 8);
    return 0;
}

extern "C" int swd_pipeline_session_buffers(swd_session *h, uint8_t **total, int64_t *total_stride, int32_t *rows_received,
                                            int32_t *windows_done) {
    Session *s = (Session *)h;
    if (!s) { set_error("null session"); return -1; }
    std::lock_guard<std::mutex> lk(s->mu);
    if (!session_plan(s)) return -1;
    if (total) *total = (uint8_t *)s->dev.p + s->o_total;
    if (total_stride) *total_stride = s->num_col;
    if (rows_received) *rows_received = s->rows;
    if (windows_done) *windows_done = s->done;
    return 0;
}
