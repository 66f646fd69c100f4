// Online sessions of the sliding-window pipeline (include/swd.h: swd_pipeline_session_*): the window loop of the reference harness
// (/root/reference/osd.py:130-179) driven by the ARRIVAL of detector rows.  A session keeps, for one batch of shots, the residual
// syndrome, total_e_hat, the observable accumulators and the per-window records on the device between calls:
//   arrival of rows [r, r + k):  resid[:, r : r + k] ^= rows                                  (session_merge_kernel)
//   window t ready (rows received >= its last row, window t - 1 committed):
//       decode it on resid[:, row0 : row1]     -- the plan's own pipeline kernel, launched for window t alone as a pipeline of length 1
//       commit the first `commit` columns, XOR their columns of the global check matrix into resid -- rows that have not arrived
//       yet included -- and their observable masks into the accumulator                        (window_commit_kernel, shift 0)
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

struct WindowCommitArgs {
    uint8_t *rows; int64_t rows_stride;       // the staged rows of a shot: the fixed session's residual syndrome, the rolling session's frame
    const uint8_t *est; int64_t est_stride;   // the window's full estimate (win_out of the decode launch)
    uint8_t *out; int64_t out_stride;         // [B][out_stride]: the committed faults of this step
    uint32_t *acc, *flag;                     // [B] observable accumulators; sticky flagged words (nullable: the fixed session has none)
    const uint32_t *chk_colptr; const uint16_t *chk_rows; const uint32_t *obs_mask;
    int32_t *shot_result;                     // nullable [B][2]: written by the step that closes a rolling experiment
    int32_t nrows, col0, commit, row_off;     // committed columns [col0, col0 + commit) of chk; staged row = row - row_off
    int32_t shift;                            // rows that leave after this step (0, the fixed session: none)
};

// one workgroup per shot: the shot's rows staged in LDS (one byte per bit inside 32-bit words), the committed faults written out, their
// columns of the global check matrix folded in with LDS atomics (as the epilogue of pipeline_kernel does; osd.py:170-178), their
// observable masks XORed into the accumulator.  shift == 0: the words are written back as they are.  shift > 0: the outgoing rows are
// ORed into the flagged word and the rest is written back moved down by `shift` rows (any number: the bytes, 0 or 1 each, are gathered
// one by one) with zeros behind.
__global__ void __launch_bounds__(256) window_commit_kernel(const WindowCommitArgs a) {
    extern __shared__ uint32_t sres[];
    __shared__ uint32_t sacc;
    const int tid = threadIdx.x, b = blockIdx.x, nw = (a.nrows + 3) >> 2;
    uint32_t *row32 = (uint32_t *)(a.rows + (int64_t)b * a.rows_stride);
    for (int q = tid; q < nw; q += 256) sres[q] = row32[q];
    if (tid == 0) sacc = 0;
    __syncthreads();
    const uint8_t *est_b = a.est + (int64_t)b * a.est_stride;
    uint8_t *out_b = a.out + (int64_t)b * a.out_stride;
    for (int i = tid; i < a.commit; i += 256) {
        const uint8_t hv = est_b[i];
        out_b[i] = hv;
        if (hv) {
            const int c = a.col0 + i;
            if (a.obs_mask) { const uint32_t om = a.obs_mask[c]; if (om) atomicXor(&sacc, om); }
            for (uint32_t e = a.chk_colptr[c]; e < a.chk_colptr[c + 1]; ++e) {
                const int r = (int)a.chk_rows[e] - a.row_off;
                if ((unsigned)r < (unsigned)a.nrows) atomicXor(&sres[r >> 2], 1u << ((r & 3) * 8)); // (always: row_off 0, or checked at creation)
            }
        }
    }
    __syncthreads();
    int any = 0;
    if (a.shift == 0) {
        for (int q = tid; q < nw; q += 256) row32[q] = sres[q];
    } else {
        const uint8_t *sb = (const uint8_t *)sres;
        int nz = 0;
        for (int r = tid; r < a.shift; r += 256) nz |= sb[r];
        any = __syncthreads_or(nz);
        for (int q = tid; q < nw; q += 256) {
            uint32_t x = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int src = 4 * q + j + a.shift;
                if (src < a.nrows && sb[src]) x |= 1u << (8 * j);
            }
            row32[q] = x;
        }
    }
    if (tid == 0) {
        const uint32_t ac = a.acc[b] ^ sacc;
        uint32_t fl = 0;
        a.acc[b] = ac;
        if (a.flag) { fl = a.flag[b] | (any ? 1u : 0u); a.flag[b] = fl; }
        if (a.shot_result) { a.shot_result[2 * b] = (int32_t)ac; a.shot_result[2 * b + 1] = fl ? 1 : 0; }
    }
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
static Plan *session_plan(SessionBase *s) {
    if (!s->plan) set_error("the pipeline of this session has been destroyed");
    return s->plan;
}

// the prologue of every entry point after create: null handle -> message, the session's lock, its plan `d` or the message that it is gone
#define SWD_SESSION_PROLOGUE(T, s, h)                 \
    T *s = (T *)(h);                                  \
    if (!s) { set_error("null session"); return -1; } \
    std::lock_guard<std::mutex> lk(s->mu);            \
    Plan *d = session_plan(s);                        \
    if (!d) return -1

// rows that must have arrived before window t is decoded: its last row; the last window closes the experiment and waits for every row
static int session_need(const Plan *d, int t) {
    return t + 1 == (int)d->wins.size() ? d->num_det : d->wins[t].row0 + d->wins[t].g->m;
}

// work on the state is ordered by one event: a call on another stream than the previous one waits for it first
static int session_enter(SessionBase *s, hipStream_t st) {
    if (s->ev_set && s->last != st) SWD_HIP(hipStreamWaitEvent(st, s->ev, 0));
    return 0;
}
static int session_leave(SessionBase *s, hipStream_t st) {
    SWD_HIP(hipEventRecord(s->ev, st));
    s->ev_set = true; s->last = st;
    return 0;
}

// the tail of both creates: the LDS limit of the commit kernel (the attribute belongs to the function: up to 65 535 staged rows, one
// word per four, against the default limit's 16 384 words) and the plan's list of live sessions
static void session_attach(SessionBase *s, Plan *d) {
    static std::mutex attr_mu;
    {
        std::lock_guard<std::mutex> lk(attr_mu);
        (void)hipFuncSetAttribute((const void *)window_commit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    }
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    d->sessions.push_back(s);
}

static void session_destroy(SessionBase *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (Plan *d = s->plan) { // (a session whose pipeline went first was detached by ~Plan and only frees its own buffers)
        std::lock_guard<std::recursive_mutex> lk(d->mu);
        d->sessions.erase(std::remove(d->sessions.begin(), d->sessions.end(), s), d->sessions.end());
    }
    delete s;
}

// begin of both forms: the batch's shots zeroed in the given ranges of `dev` ({offset, bytes per shot}); the caller resets its counters
static int session_begin(SessionBase *s, Plan *d, int32_t B, const char *form, std::initializer_list<std::pair<size_t, size_t>> zero) {
    if (B <= 0 || B > s->max_shots) { set_error("%s begin: %d shots, the session was created for 1..%d", form, B, s->max_shots); return -1; }
    SWD_HIP(hipSetDevice(d->device));
    if (session_enter(s, s->st)) return -1;
    for (const auto &z : zero) SWD_HIP(hipMemsetAsync((char *)s->dev.p + z.first, 0, (size_t)B * z.second, s->st));
    s->B = B;
    return session_leave(s, s->st);
}

// host rows [B][k] (row stride `stride`) through the page-locked block -- free here: every step of a host call ends synchronised --
// to dev + o_in, packed [B][k]; `room`: bytes the block is sized for
static int session_stage(SessionBase *s, size_t o_in, int k, const uint8_t *rows, int64_t stride, size_t room, hipStream_t st) {
    if (s->hin.reserve(room)) return -1;
    for (int b = 0; b < s->B; ++b) memcpy((char *)s->hin.p + (size_t)b * k, rows + (size_t)b * stride, (size_t)k);
    SWD_HIP(hipMemcpyAsync((char *)s->dev.p + o_in, s->hin.p, (size_t)s->B * k, hipMemcpyHostToDevice, st));
    return 0;
}

// rows [r, r + k) of the staged rows ^= the arriving rows
static int launch_merge(uint8_t *rows, int64_t rows_stride, const uint8_t *in, int64_t in_stride, int B, int r, int k, hipStream_t st) {
    const long long nthr = (long long)B * (((r + k - 1) >> 2) - (r >> 2) + 1);
    hipLaunchKernelGGL(session_merge_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, rows, rows_stride, in, in_stride, B, r, k);
    SWD_HIP(hipGetLastError());
    return 0;
}

// the window decode: the plan's kernel on one window alone -- a pipeline of length 1 whose `det` is the staged rows (the kernel's
// window-0 path reads absolute rows row0..), the full estimate through win_out, nothing committed by the kernel
static int launch_window(Plan *d, const SwdWindowDev *win, int B, const uint8_t *rows, int64_t rows_stride, int nrows, uint8_t *est,
                         int64_t est_stride, int32_t *stats, double *min_pm, hipStream_t st) {
    SwdPipeArgs a{};
    a.wins = win; a.W = 1; a.B = B;
    a.slot_scratch = 1;
    fill_params(d, a.P, false, false);
    a.det = rows; a.det_stride = rows_stride; a.num_det = nrows; a.off_det = d->off_det;
    a.total = nullptr; a.win_out = est; a.win_out_stride = est_stride;
    a.stats = stats; a.min_pm = min_pm;
    a.hist = nullptr; a.hist_stride = 4 * (int64_t)d->nmax;
    return launch(d, a, st);
}

// ... and its commit, on the rows and the estimate of that launch: the plan's chk / obs are filled in here, the rest is the caller's
static int launch_commit(Plan *d, WindowCommitArgs c, int B, hipStream_t st) {
    c.chk_colptr = d->d_colptr; c.chk_rows = d->d_rows; c.obs_mask = d->d_obs.p ? d->d_obs.as<uint32_t>() : nullptr;
    hipLaunchKernelGGL(window_commit_kernel, dim3(B), dim3(256), (size_t)((c.nrows + 3) / 4) * 4, st, c);
    SWD_HIP(hipGetLastError());
    return 0;
}

static int session_push_dev(Session *s, Plan *d, int32_t nrows, const uint8_t *det_rows, int64_t stride, int32_t *first, int32_t *count,
                            hipStream_t st) {
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
        if (launch_merge((uint8_t *)dv, s->res_stride, det_rows, stride ? stride : (int64_t)nrows, B, s->rows, nrows, st)) return -1;
        s->rows += nrows;
    }
    const int first_w = s->done;
    int rc = 0;
    while (s->done < W && s->rows >= session_need(d, s->done)) {
        const int t = s->done;
        const WindowHost &w = d->wins[t];
        WindowCommitArgs c{}; // (no flag, no shift: the residual syndrome stays where it is, rows that have not arrived yet included)
        c.rows = (uint8_t *)dv; c.rows_stride = s->res_stride; c.nrows = s->num_det;
        c.est = (const uint8_t *)(dv + s->o_est); c.est_stride = s->est_stride;
        c.out = (uint8_t *)(dv + s->o_total) + w.col0; c.out_stride = s->num_col;
        c.acc = (uint32_t *)(dv + s->o_acc);
        c.col0 = w.col0; c.commit = w.commit;
        if ((rc = launch_window(d, d->d_wins.as<SwdWindowDev>() + t, B, c.rows, c.rows_stride, c.nrows, (uint8_t *)(dv + s->o_est), s->est_stride,
                                (int32_t *)(dv + s->o_stats) + (size_t)t * s->max_shots * SWD_STAT_WORDS,
                                (double *)(dv + s->o_pm) + (size_t)t * s->max_shots, st)) != 0 ||
            (rc = launch_commit(d, c, B, st)) != 0)
            break;
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
    if (hipSetDevice(d->device) != hipSuccess) { set_error(SWD_ERR_DEVICE, "hipSetDevice(%d) failed", d->device); return nullptr; }
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
        if (s->dev.p) set_error(SWD_ERR_DEVICE, "session: stream / event creation failed");
        delete s;
        return nullptr;
    }
    session_attach(s, d);
    return (swd_session *)s;
}

extern "C" void swd_pipeline_session_destroy(swd_session *h) { session_destroy((Session *)h); }

extern "C" int swd_pipeline_session_begin(swd_session *h, int32_t B) {
    SWD_SESSION_PROLOGUE(Session, s, h);
    // residual syndrome, total_e_hat and accumulators of the batch's shots
    if (session_begin(s, d, B, "session", {{0, (size_t)s->res_stride}, {s->o_total, (size_t)s->num_col}, {s->o_acc, 4}})) return -1;
    s->rows = 0; s->done = 0;
    return 0;
}

extern "C" int swd_pipeline_session_push_dev(swd_session *h, int32_t nrows, const uint8_t *det_rows, int64_t stride, int32_t *first,
                                             int32_t *count, void *stream) {
    SWD_SESSION_PROLOGUE(Session, s, h);
    return session_push_dev(s, d, nrows, det_rows, stride, first, count, (hipStream_t)stream);
}

extern "C" int swd_pipeline_session_push(swd_session *h, int32_t nrows, const uint8_t *det_rows, int32_t *first, int32_t *count) {
    SWD_SESSION_PROLOGUE(Session, s, h);
    const uint8_t *src = nullptr;
    if (nrows > 0 && det_rows && s->B && s->done < s->W && s->rows + (int64_t)nrows <= s->num_det) { // (anything else: session_push_dev refuses it with its message)
        SWD_HIP(hipSetDevice(d->device));
        if (session_enter(s, s->st) || session_stage(s, s->o_in, nrows, det_rows, nrows, (size_t)s->B * nrows, s->st) || session_leave(s, s->st)) return -1;
        src = (const uint8_t *)s->dev.p + s->o_in;
    }
    const int rc = session_push_dev(s, d, nrows, src ? src : det_rows, 0, first, count, s->st); // (det_rows itself only on the refused paths)
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
    SWD_SESSION_PROLOGUE(Session, s, h);
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
    SWD_SESSION_PROLOGUE(Session, s, h);
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
    SWD_SESSION_PROLOGUE(Session, s, h);
    (void)d;
    if (total) *total = (uint8_t *)s->dev.p + s->o_total;
    if (total_stride) *total_stride = s->num_col;
    if (rows_received) *rows_received = s->rows;
    if (windows_done) *windows_done = s->done;
    return 0;
}

// ---- rolling sessions (include/swd.h: swd_pipeline_rolling_*) ------------------------------------------------------------------------
// The plan of R0 rounds is a template: head = window 0, body = window 1, tail = last window.  Per shot the session keeps a FRAME of
// residual rows whose row 0 is the first row of the window decoded next (so all three windows sit at frame row 0), the observable
// accumulator and a sticky flagged word -- nothing that grows with the experiment:
//   arrival of k rows:      frame[:, fill : fill + k] ^= rows                                           (session_merge_kernel)
//   frame holds a window:   decode it on frame[:, 0 : m] -- the plan's kernel as a pipeline of length 1 on a descriptor whose row0 is 0 --
//                           commit, fold chk, accumulate observables, flag and drop the F * h rows that leave   (window_commit_kernel, shift > 0)
//   finish:                 the last rows, the tail window, committed whole; every row left in the frame goes into the flag
// The global check matrix of the template serves every window: body window t of a long experiment commits the columns of the
// template's window 1, and its rows are those of window 1 moved down -- in frame rows both are `row - row0 of window 1`.
namespace swd {

// the state of a rolling session: nothing in it grows with the experiment
struct Rolling : SessionBase {
    enum { HEAD = 0, BODY = 1, TAIL = 2 };
    struct Kind { int col0, commit, row_off, rows; } kd[3]{};
    int frame_rows = 0, row_stride = 0, cmax = 0, call = 0; // cmax: head / body commits; call: the tail's too
    int64_t frame_stride = 0;
    int fill = 0;                 // rows in the frame
    long long rows64 = 0, done64 = 0;
    bool closed = false;          // finish has run: begin first
    DevBuf wins3;                 // head, body, tail descriptors with row0 = 0
    // dev: [ frame | flag | acc | window estimate | step output: faults [B][call] | stats | min_pm | shot_result ] [ rows in ]
    size_t o_flag = 0, o_acc = 0, o_est = 0, o_out = 0, s_stats = 0, s_pm = 0, s_shot = 0, out_bytes = 0, o_in = 0, dev_bytes = 0;
};

// where the results of the windows of one call go: device arrays of the caller (window k at its offset), or the session's one-step
// block -- then copied to the caller's HOST arrays after every window
struct RollingOut {
    uint8_t *faults = nullptr; int32_t *stats = nullptr; double *min_pm = nullptr; int32_t *shot_result = nullptr;
    bool host = false;
    bool decode_windows = true; // false (finish): the rows complete no head / body window, the tail follows
    int max_windows = 0, count = 0;
};

static const char *rolling_lengths(const Rolling *r, char *buf, size_t n) {
    // the rows of an experiment served: tail rows + one stride per window before the tail, at least one (the head)
    snprintf(buf, n, "%d + %d k detector rows, k >= 1 (the final block included)", r->kd[Rolling::TAIL].rows, r->row_stride);
    return buf;
}

// decode + commit the window the frame holds (kind: head / body / tail); results to `o` slot k
static int rolling_step(Rolling *r, Plan *d, int kind, RollingOut &o, hipStream_t st) {
    char *dv = (char *)r->dev.p;
    const int B = r->B, k = o.count;
    const Rolling::Kind &K = r->kd[kind];
    const int64_t fstride = kind == Rolling::TAIL ? K.commit : r->cmax;
    // the caller's device array (slot k of this call) or the session's one-step block
    auto dest = [&](auto *caller, size_t slot_elems, size_t own_off) {
        return (!o.host && caller) ? caller + (size_t)k * slot_elems : (decltype(caller))(dv + r->o_out + own_off);
    };
    WindowCommitArgs c{};
    c.rows = (uint8_t *)dv; c.rows_stride = r->frame_stride; c.nrows = r->frame_rows;
    c.est = (const uint8_t *)(dv + r->o_est); c.est_stride = r->est_stride;
    c.out = dest(o.faults, (size_t)B * fstride, 0); c.out_stride = fstride;
    c.acc = (uint32_t *)(dv + r->o_acc); c.flag = (uint32_t *)(dv + r->o_flag);
    c.shot_result = kind == Rolling::TAIL ? dest(o.shot_result, 0, r->s_shot) : nullptr;
    c.col0 = K.col0; c.commit = K.commit; c.row_off = K.row_off;
    c.shift = kind == Rolling::TAIL ? r->frame_rows : r->row_stride;
    if (launch_window(d, r->wins3.as<SwdWindowDev>() + kind, B, c.rows, c.rows_stride, c.nrows, (uint8_t *)(dv + r->o_est), r->est_stride,
                      dest(o.stats, (size_t)B * SWD_STAT_WORDS, r->s_stats), dest(o.min_pm, (size_t)B, r->s_pm), st) ||
        launch_commit(d, c, B, st))
        return -1;
    if (o.host) { // the one-step block -> the caller's host arrays, before the next window overwrites it
        if (r->hout.reserve(std::max(r->out_bytes, (size_t)4096))) return -1;
        SWD_HIP(hipMemcpyAsync(r->hout.p, dv + r->o_out, r->out_bytes, hipMemcpyDeviceToHost, st));
        SWD_HIP(hipStreamSynchronize(st));
        const char *ho = (const char *)r->hout.p;
        if (o.faults) { // (staged rows: [B][fstride])
            for (int b = 0; b < B; ++b) memcpy(o.faults + ((size_t)k * B + b) * fstride, ho + (size_t)b * fstride, (size_t)K.commit);
        }
        if (o.stats) memcpy(o.stats + (size_t)k * B * SWD_STAT_WORDS, ho + r->s_stats, (size_t)B * SWD_STAT_WORDS * 4);
        if (o.min_pm) memcpy(o.min_pm + (size_t)k * B, ho + r->s_pm, (size_t)B * 8);
        if (o.shot_result && kind == Rolling::TAIL) memcpy(o.shot_result, ho + r->s_shot, (size_t)B * 8);
    }
    o.count++;
    return 0;
}

// windows that nrows more rows complete
static long long rolling_windows_for(const Rolling *r, long long nrows) {
    const long long have = r->fill + nrows, need = r->kd[Rolling::HEAD].rows;
    return have < need ? 0 : (have - need) / r->row_stride + 1;
}

// XOR rows [0, nrows) of `rows` (device, or host when o.host) into the frame piece by piece, decoding every window that completes
static int rolling_rows(Rolling *r, Plan *d, int nrows, const uint8_t *rows, int64_t stride, RollingOut &o, hipStream_t st) {
    char *dv = (char *)r->dev.p;
    const int B = r->B;
    if (!stride) stride = nrows;
    int done = 0;
    while (done < nrows) {
        const int k = std::min(nrows - done, r->frame_rows - r->fill); // (> 0: a frame that holds a window has been decoded)
        const uint8_t *src = rows + done;
        int64_t sstride = stride;
        if (o.host) {
            if (session_stage(r, r->o_in, k, src, stride, std::max((size_t)B * r->frame_rows, (size_t)4096), st)) return -1;
            src = (const uint8_t *)(dv + r->o_in); sstride = k;
        }
        if (launch_merge((uint8_t *)dv, r->frame_stride, src, sstride, B, r->fill, k, st)) return -1;
        r->fill += k; r->rows64 += k; done += k;
        if (o.host) SWD_HIP(hipStreamSynchronize(st)); // (hin is reused by the next piece)
        while (o.decode_windows && r->fill >= r->kd[Rolling::HEAD].rows) {
            if (rolling_step(r, d, r->done64 == 0 ? Rolling::HEAD : Rolling::BODY, o, st)) return -1;
            r->fill -= r->row_stride; r->done64++;
        }
    }
    return 0;
}

static int rolling_push(Rolling *r, Plan *d, int32_t nrows, const uint8_t *rows, int64_t stride, RollingOut &o, int64_t *first, int32_t *count,
                        hipStream_t st) {
    if (!r->B) { set_error("rolling push: call swd_pipeline_rolling_begin first"); return -1; }
    if (r->closed) { set_error("rolling push: the experiment has been finished; begin a new batch"); return -1; }
    if (nrows < 0 || (nrows > 0 && !rows)) { set_error(nrows < 0 ? "rolling push: negative row count" : "null input pointer"); return -1; }
    const long long nwin = rolling_windows_for(r, nrows);
    if (nwin > o.max_windows) {
        set_error("rolling push: %d rows complete %lld windows, the output arrays hold %d", nrows, nwin, o.max_windows);
        return -1;
    }
    SWD_HIP(hipSetDevice(d->device));
    if (session_enter(r, st)) return -1;
    const long long first_w = r->done64;
    const int rc = rolling_rows(r, d, nrows, rows, stride, o, st);
    if (session_leave(r, st)) return -1;
    if (first) *first = first_w;
    if (count) *count = o.count;
    return rc;
}

static int rolling_finish(Rolling *r, Plan *d, int32_t nrows, const uint8_t *rows, int64_t stride, RollingOut &o, hipStream_t st) {
    if (!r->B) { set_error("rolling finish: call swd_pipeline_rolling_begin first"); return -1; }
    if (r->closed) { set_error("rolling finish: the experiment has been finished; begin a new batch"); return -1; }
    if (nrows < 0 || (nrows > 0 && !rows)) { set_error(nrows < 0 ? "rolling finish: negative row count" : "null input pointer"); return -1; }
    char buf[160];
    const long long total = r->rows64 + nrows;
    if (nrows == 0) {
        set_error("rolling finish: no final rows -- the final block must go to finish, not to push (%lld rows pushed; this template serves %s)",
                  r->rows64, rolling_lengths(r, buf, sizeof buf));
        return -1;
    }
    if (r->done64 == 0) {
        set_error("rolling finish: %lld detector rows are fewer than the first and the last window need; this template serves %s", total,
                  rolling_lengths(r, buf, sizeof buf));
        return -1;
    }
    if (r->fill + (long long)nrows != r->kd[Rolling::TAIL].rows) {
        set_error("rolling finish: %lld detector rows (%lld pushed, %d final) do not make an experiment this template serves: %s", total,
                  r->rows64, nrows, rolling_lengths(r, buf, sizeof buf));
        return -1;
    }
    SWD_HIP(hipSetDevice(d->device));
    if (session_enter(r, st)) return -1;
    o.decode_windows = false; // (the frame holds the tail's rows)
    int rc = rolling_rows(r, d, nrows, rows, stride, o, st);
    if (!rc) rc = rolling_step(r, d, Rolling::TAIL, o, st);
    if (!rc) { r->fill = 0; r->done64++; r->closed = true; }
    if (session_leave(r, st)) return -1;
    return rc;
}

} // namespace swd

extern "C" swd_rolling *swd_pipeline_rolling_create(swd_pipeline *h, int32_t max_shots) {
    Plan *d = (Plan *)h;
    if (!d) { set_error("null pipeline"); return nullptr; }
    if (d->wins.empty() || d->num_col <= 0) { set_error("a rolling session needs a sliding-window pipeline"); return nullptr; }
    if (max_shots <= 0) { set_error("max_shots must be positive"); return nullptr; }
    const int n = (int)d->wins.size();
    if (n < 3) { set_error("rolling template: %d windows, a first, a body and a last window are needed", n); return nullptr; }
    if (hipSetDevice(d->device) != hipSuccess) { set_error(SWD_ERR_DEVICE, "hipSetDevice(%d) failed", d->device); return nullptr; }
    const WindowHost &w0 = d->wins[0], &w1 = d->wins[1], &wl = d->wins[n - 1];
    const int rs = d->wins[2].row0 - w1.row0, cs = d->wins[2].col0 - w1.col0;
    if (rs <= 0 || cs <= 0 || w0.row0 != 0 || w0.col0 != 0 || w1.row0 != rs || w1.g->m != w0.g->m || w1.commit != cs || w0.commit != w1.col0 ||
        wl.row0 + wl.g->m != d->num_det || wl.col0 + wl.commit != d->num_col) {
        set_error("rolling template: windows are not periodic (placement of the first, second and last window)");
        return nullptr;
    }
    for (int k = 2; k < n; ++k) {
        const WindowHost &w = d->wins[k];
        if (w.row0 - d->wins[k - 1].row0 != rs || w.col0 - d->wins[k - 1].col0 != cs) { set_error("rolling template: window %d is not placed one stride after window %d", k, k - 1); return nullptr; }
        if (k < n - 1 && (w.g != w1.g || w.commit != w1.commit || w.new_n != w1.new_n)) { set_error("rolling template: window %d is not periodic (matrix, priors or commit differ from window 1)", k); return nullptr; }
    }
    // the plan's host copy of the CSC of chk and the observable masks: periodicity of the committed columns, and the rows they reach
    const std::vector<uint32_t> &cp = d->h_colptr, &om = d->h_obs;
    const std::vector<uint16_t> &rows = d->h_rows;
    for (int k = 2; k < n - 1; ++k)
        for (int i = 0; i < cs; ++i) {
            const int ca = w1.col0 + i, cb = d->wins[k].col0 + i;
            bool same = cp[ca + 1] - cp[ca] == cp[cb + 1] - cp[cb] && (om.empty() || om[ca] == om[cb]);
            for (uint32_t e = 0; same && e < cp[ca + 1] - cp[ca]; ++e) same = rows[cp[ca] + e] + (k - 1) * rs == rows[cp[cb] + e];
            if (!same) { set_error("rolling template: chk / obs are not periodic (column %d of window %d against window 1)", i, k); return nullptr; }
        }
    Rolling *r = new Rolling();
    const int idx[3] = {0, 1, n - 1};
    std::vector<SwdWindowDev> hw(3); // the three descriptors: the plan's own, at frame row 0
    int frame = 0;
    for (int j = 0; j < 3; ++j) {
        const WindowHost &w = d->wins[idx[j]];
        r->kd[j] = {w.col0, w.commit, w.row0, w.g->m};
        hw[j] = d->h_wins[idx[j]];
        hw[j].row0 = 0;
        frame = std::max(frame, w.g->m);
        for (uint32_t e = cp[w.col0]; e < cp[w.col0 + w.commit]; ++e) {
            if (rows[e] < w.row0) { set_error("rolling template: a committed column of window %d touches row %d, before the window", idx[j], (int)rows[e]); delete r; return nullptr; }
            frame = std::max(frame, (int)rows[e] - w.row0 + 1);
        }
    }
    if (frame > d->num_det) { set_error("rolling template: the frame (%d rows) exceeds the template's %d detector rows", frame, d->num_det); delete r; return nullptr; }
    r->plan = d; r->device = d->device; r->max_shots = max_shots;
    r->frame_rows = frame; r->row_stride = rs;
    r->cmax = std::max(w0.commit, w1.commit); r->call = std::max(r->cmax, wl.commit);
    r->est_stride = align_up(d->nmax, 16);
    r->frame_stride = align_up(frame, 16);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t B = (size_t)max_shots;
    r->o_flag = al(B * r->frame_stride);
    r->o_acc = r->o_flag + al(B * 4);
    r->o_est = r->o_acc + al(B * 4);
    r->o_out = r->o_est + al(B * r->est_stride);
    r->s_stats = al(B * r->call);
    r->s_pm = r->s_stats + al(B * SWD_STAT_WORDS * 4);
    r->s_shot = r->s_pm + al(B * 8);
    r->out_bytes = r->s_shot + al(B * 8);
    r->o_in = r->o_out + r->out_bytes;
    r->dev_bytes = r->o_in + al(B * (size_t)frame);
    if (r->dev.reserve(r->dev_bytes) || r->wins3.reserve(3 * sizeof(SwdWindowDev)) ||
        hipMemcpy(r->wins3.p, hw.data(), 3 * sizeof(SwdWindowDev), hipMemcpyHostToDevice) != hipSuccess ||
        hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&r->ev, hipEventDisableTiming) != hipSuccess) {
        if (r->dev.p) set_error(SWD_ERR_DEVICE, "rolling session: descriptor copy / stream / event creation failed");
        delete r;
        return nullptr;
    }
    r->dev_bytes = r->dev.cap + r->wins3.cap;
    session_attach(r, d);
    return (swd_rolling *)r;
}

extern "C" void swd_pipeline_rolling_destroy(swd_rolling *h) { session_destroy((Rolling *)h); }

extern "C" int swd_pipeline_rolling_begin(swd_rolling *h, int32_t B) {
    SWD_SESSION_PROLOGUE(Rolling, r, h);
    // frames, flagged words and accumulators of the batch's shots
    if (session_begin(r, d, B, "rolling", {{0, (size_t)r->frame_stride}, {r->o_flag, 4}, {r->o_acc, 4}})) return -1;
    r->fill = 0; r->rows64 = 0; r->done64 = 0; r->closed = false;
    return 0;
}

extern "C" int swd_pipeline_rolling_push_dev(swd_rolling *h, int32_t nrows, const uint8_t *det_rows, int64_t stride, int32_t max_windows,
                                             uint8_t *faults, int32_t *stats, double *min_pm, int64_t *first, int32_t *count, void *stream) {
    SWD_SESSION_PROLOGUE(Rolling, r, h);
    RollingOut o;
    o.faults = faults; o.stats = stats; o.min_pm = min_pm; o.max_windows = std::max(max_windows, 0);
    return rolling_push(r, d, nrows, det_rows, stride, o, first, count, (hipStream_t)stream);
}

extern "C" int swd_pipeline_rolling_push(swd_rolling *h, int32_t nrows, const uint8_t *det_rows, int32_t max_windows, uint8_t *faults,
                                         int32_t *stats, double *min_pm, int64_t *first, int32_t *count) {
    SWD_SESSION_PROLOGUE(Rolling, r, h);
    RollingOut o;
    o.faults = faults; o.stats = stats; o.min_pm = min_pm; o.max_windows = std::max(max_windows, 0); o.host = true;
    if (rolling_push(r, d, nrows, det_rows, 0, o, first, count, r->st)) return -1;
    SWD_HIP(hipStreamSynchronize(r->st));
    return 0;
}

extern "C" int swd_pipeline_rolling_finish_dev(swd_rolling *h, int32_t nrows, const uint8_t *final_rows, int64_t stride, uint8_t *faults,
                                               int32_t *stats, double *min_pm, int32_t *shot_result, void *stream) {
    SWD_SESSION_PROLOGUE(Rolling, r, h);
    RollingOut o;
    o.faults = faults; o.stats = stats; o.min_pm = min_pm; o.shot_result = shot_result;
    return rolling_finish(r, d, nrows, final_rows, stride, o, (hipStream_t)stream);
}

extern "C" int swd_pipeline_rolling_finish(swd_rolling *h, int32_t nrows, const uint8_t *final_rows, uint8_t *faults, int32_t *stats,
                                           double *min_pm, int32_t *shot_result) {
    SWD_SESSION_PROLOGUE(Rolling, r, h);
    RollingOut o;
    o.faults = faults; o.stats = stats; o.min_pm = min_pm; o.shot_result = shot_result; o.host = true;
    if (rolling_finish(r, d, nrows, final_rows, 0, o, r->st)) return -1;
    SWD_HIP(hipStreamSynchronize(r->st));
    return 0;
}

extern "C" int swd_pipeline_rolling_state(swd_rolling *h, int64_t *rows_received, int64_t *windows_done, int32_t *frame_fill, int32_t *info,
                                          int64_t *device_bytes) {
    SWD_SESSION_PROLOGUE(Rolling, r, h);
    (void)d;
    if (rows_received) *rows_received = r->rows64;
    if (windows_done) *windows_done = r->done64;
    if (frame_fill) *frame_fill = r->fill;
    if (info) {
        const int v[8] = {r->frame_rows, r->kd[Rolling::HEAD].rows, r->row_stride, r->kd[Rolling::TAIL].rows, r->kd[Rolling::HEAD].commit,
                          r->kd[Rolling::BODY].commit, r->kd[Rolling::TAIL].commit, r->cmax};
        for (int i = 0; i < 8; ++i) info[i] = v[i];
    }
    if (device_bytes) *device_bytes = (int64_t)r->dev_bytes;
    return 0;
}
