// Detector front end (include/swd.h: swd_frontend_*): raw measurement records in, detector rows out, on the device.
// Every detector of a memory experiment is the parity of measurements of its own round and of the round before it, and the rounds
// after the first are translates of one another (measurements.py, MeasurementMap.blocks).  Three templates over
// [previous round | this block] therefore state the whole map -- HEAD for round 0, BODY for every later syndrome round, TAIL for the
// final block, with the observables -- and a front end keeps, per shot, only the last complete round's outcomes and the bits of the
// round under way, one byte per bit:  state[b] = [ previous round: mpr | round under way: mpr ].
// A push stages  [ previous round | round under way | the call's new bits ]  of a shot in LDS, one lane per detector row of every
// round that is now complete gathers and XORs its template entries (u16 offsets into the staged bytes), the rows go out as
// consecutive bytes, and the last complete round and the unfinished rest become the new state.  One launch per push.
#include <mutex>

#include "swd_host.h"

namespace swd {

namespace {

constexpr int kFeThreads = 64;      // one wave per shot
constexpr int kFeStage = 32768;     // staged bytes of a launch (LDS); a longer push is cut into several launches

struct FeArgs {
    uint8_t *state; int64_t state_stride;       // [B][2 mpr]
    const uint8_t *meas; int64_t meas_stride;   // the call's buffer of a shot: bytes, or bits (bit i & 7 of byte i >> 3)
    uint8_t *det; int64_t det_stride;           // rows of this launch: [B][rounds h (+ h with the tail)]
    uint32_t *raw_obs;                          // [B], written by a tail launch
    const uint32_t *rowptr; const uint16_t *off; // templates: rows [0, h) HEAD, [h, 2h) BODY, [2h, 3h) TAIL, [3h, 3h + nobs) observables
    int32_t mpr, mfin, h, nobs;
    int32_t fill;       // bits of the round under way in the state
    int32_t src0, n;    // the launch takes items [src0, src0 + n) of the buffer
    int32_t packed, vec; // vec: every shot's buffer is 8-byte aligned
    int32_t first_round; // rounds completed before this launch (0: its first round takes HEAD)
    int32_t tail;       // 1: the items end with the final block
};

// parity of one template row over the staged bytes at `base`
__device__ __forceinline__ uint32_t fe_row(const FeArgs &a, const uint8_t *base, int row) {
    uint32_t x = 0;
    for (uint32_t e = a.rowptr[row], e1 = a.rowptr[row + 1]; e < e1; ++e) x ^= base[a.off[e]];
    return x;
}

__global__ void __launch_bounds__(kFeThreads) frontend_kernel(const FeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fe_lds[]; // [mpr | fill | n]
    const int tid = threadIdx.x, b = blockIdx.x;
    const int mpr = a.mpr, have = a.fill + a.n;               // bits behind the previous round
    uint8_t *st = a.state + (int64_t)b * a.state_stride;
    for (int i = tid; i < mpr + a.fill; i += kFeThreads) fe_lds[i] = st[i];
    uint8_t *nb = fe_lds + mpr + a.fill;
    const uint8_t *src = a.meas + (int64_t)b * a.meas_stride;
    const int s0 = a.src0, s1 = a.src0 + a.n;
    if (a.n > 0) {
        // 8 source bytes per lane and step: 64 bits of a packed buffer, 8 items of a byte buffer
        const int per = a.packed ? 64 : 8, nbytes = a.packed ? (s1 + 7) >> 3 : s1;
        for (int w = s0 / per + tid; w * per < s1; w += kFeThreads) {
            uint64_t x = 0;
            if (a.vec && 8 * w + 8 <= nbytes) x = *(const uint64_t *)(src + 8 * (int64_t)w);
            else
                for (int j = 0; j < 8; ++j)
                    if (8 * w + j < nbytes) x |= (uint64_t)src[8 * (int64_t)w + j] << (8 * j);
            const int lo = max(s0, w * per), hi = min(s1, (w + 1) * per);
            if (a.packed)
                for (int s = lo; s < hi; ++s) nb[s - s0] = (uint8_t)((x >> (s & 63)) & 1u);
            else
                for (int s = lo; s < hi; ++s) nb[s - s0] = (uint8_t)(((x >> (8 * (s & 7))) & 0xFFu) != 0);
        }
    }
    __syncthreads();
    const int h = a.h;
    const int nr = a.tail ? (have - a.mfin) / mpr : have / mpr; // syndrome rounds complete now
    uint8_t *out = a.det + (int64_t)b * a.det_stride;
    for (int i = tid; i < nr * h; i += kFeThreads) {
        const int k = i / h, r = i - k * h;
        out[i] = (uint8_t)fe_row(a, fe_lds + k * mpr, (a.first_round + k ? h : 0) + r);
    }
    if (a.tail) {
        const uint8_t *base = fe_lds + nr * mpr; // [last syndrome round | final block]
        for (int r = tid; r < h; r += kFeThreads) out[nr * h + r] = (uint8_t)fe_row(a, base, 2 * h + r);
        // observable k on lane k of the wave: the ballot is the mask
        const uint32_t bit = tid < a.nobs ? fe_row(a, base, 3 * h + tid) : 0u;
        const uint64_t mask = __ballot(bit != 0);
        if (tid == 0) a.raw_obs[b] = (uint32_t)mask;
        return; // the experiment is over: the state is dead until the next begin
    }
    // carry: the last complete round, then the unfinished rest (every staged byte was read before the barrier above)
    if (nr > 0)
        for (int i = tid; i < mpr; i += kFeThreads) st[i] = fe_lds[nr * mpr + i];
    const int rest = have - nr * mpr, from = nr > 0 ? 0 : a.fill;
    for (int i = from + tid; i < rest; i += kFeThreads) st[mpr + i] = fe_lds[(nr + 1) * mpr + i];
}

struct FrontEnd {
    int device = 0, max_shots = 0, B = 0;
    int mpr = 0, mfin = 0, h = 0, nobs = 0;
    int64_t state_stride = 0;
    int64_t bits = 0, rounds = 0; // since begin
    int fill = 0;
    bool finished = false;
    DevBuf dev;       // templates, then the state
    DevBuf hin, hdet; // device staging of the host-pointer twins
    size_t o_off = 0, o_state = 0, bytes = 0;
    hipStream_t st = nullptr, last = nullptr; // own stream (host twins, begin); the stream of the most recent work on the state
    hipEvent_t ev = nullptr;
    bool used = false;
    std::mutex mu;
    ~FrontEnd() {
        if (ev) (void)hipEventDestroy(ev);
        if (st) (void)hipStreamDestroy(st);
    }
};

// work on the state is ordered by one event, as in the sessions: a call on another stream than the previous one waits for it first
int fe_enter(FrontEnd *f, hipStream_t st) {
    if (f->used && f->last != st) SWD_HIP(hipStreamWaitEvent(st, f->ev, 0));
    return 0;
}
int fe_leave(FrontEnd *f, hipStream_t st) {
    SWD_HIP(hipEventRecord(f->ev, st));
    f->used = true; f->last = st;
    return 0;
}

// the launches of `n` items from item `src0` of the buffer on; tail: they end with the final block.  -> rows written per shot
int fe_launch(FrontEnd *f, int n, int src0, const uint8_t *meas, int64_t stride, int packed, uint8_t *det, int64_t det_stride, uint32_t *raw_obs,
              bool tail, hipStream_t st) {
    FeArgs a{};
    char *dv = (char *)f->dev.p;
    a.state = (uint8_t *)(dv + f->o_state); a.state_stride = f->state_stride;
    a.meas = meas; a.meas_stride = stride; a.det_stride = det_stride; a.raw_obs = raw_obs;
    a.rowptr = (const uint32_t *)dv; a.off = (const uint16_t *)(dv + f->o_off);
    a.mpr = f->mpr; a.mfin = f->mfin; a.h = f->h; a.nobs = f->nobs;
    a.packed = packed; a.vec = ((uintptr_t)meas % 8 == 0 && stride % 8 == 0) ? 1 : 0;
    // a tail launch holds the rest of one round and the final block (the caller sends the rounds before it ahead): 2 mpr + mfin bytes
    // at most; a push launch takes what the stage holds behind the state's bytes, at least mfin >= 1 items
    do {
        const int take = tail ? n : std::min(n, kFeStage - f->mpr - f->fill);
        const int nr = (f->fill + take - (tail ? f->mfin : 0)) / f->mpr;
        a.fill = f->fill; a.src0 = src0; a.n = take; a.first_round = f->rounds ? 1 : 0; a.tail = tail ? 1 : 0;
        a.det = det;
        hipLaunchKernelGGL(frontend_kernel, dim3((unsigned)f->B), dim3(kFeThreads), (size_t)(f->mpr + f->fill + take), st, a);
        SWD_HIP(hipGetLastError());
        f->fill = f->fill + take - nr * f->mpr - (tail ? f->mfin : 0);
        f->rounds += nr; f->bits += take;
        det += (int64_t)nr * f->h;
        src0 += take; n -= take;
    } while (n > 0);
    return 0;
}

int fe_check_push(FrontEnd *f, int32_t nbits, const uint8_t *meas, const uint8_t *det_rows) {
    if (!f->B) { set_error("front end push: call swd_frontend_begin first"); return -1; }
    if (f->finished) { set_error("front end push: the final block has been taken (%lld bits); begin a new batch", (long long)f->bits); return -1; }
    if (nbits < 0) { set_error("front end push: %d bits", nbits); return -1; }
    if (nbits > 0 && !meas) { set_error("null input pointer"); return -1; }
    if ((f->fill + (int64_t)nbits) / f->mpr > 0 && !det_rows) { set_error("null output pointer"); return -1; }
    return 0;
}

// bytes between the shots of a dense buffer of nbits items
int64_t fe_dense(int nbits, int packed) { return packed ? (nbits + 7) / 8 : nbits; }

int fe_push_dev(FrontEnd *f, int32_t nbits, const uint8_t *meas, int64_t stride, int32_t packed, uint8_t *det_rows, int64_t det_stride,
                int32_t *rows_out, hipStream_t st) {
    if (fe_check_push(f, nbits, meas, det_rows)) return -1;
    const int64_t rows = (f->fill + (int64_t)nbits) / f->mpr * f->h;
    stride = stride ? stride : fe_dense(nbits, packed); det_stride = det_stride ? det_stride : rows;
    if (stride < fe_dense(nbits, packed) || det_stride < rows) { set_error("front end push: a stride is shorter than a shot's %d bits / %lld rows", nbits, (long long)rows); return -1; }
    if (rows_out) *rows_out = (int32_t)rows;
    if (nbits == 0) return 0;
    SWD_HIP(hipSetDevice(f->device));
    if (fe_enter(f, st) || fe_launch(f, nbits, 0, meas, stride, packed ? 1 : 0, det_rows, det_stride, nullptr, false, st)) return -1;
    return fe_leave(f, st);
}

// the bits a finish must bring: the rest of the syndrome round under way (whole further rounds are taken too), then the final block
int fe_check_finish(FrontEnd *f, int32_t nbits, const uint8_t *meas, const uint8_t *det_rows, const uint32_t *raw_obs) {
    if (!f->B) { set_error("front end finish: call swd_frontend_begin first"); return -1; }
    if (f->finished) { set_error("front end finish: the final block has been taken already; begin a new batch"); return -1; }
    const int64_t pre = (int64_t)nbits - f->mfin;
    if (pre < 0 || (f->fill + pre) % f->mpr != 0 || f->rounds + (f->fill + pre) / f->mpr < 1) {
        set_error("front end finish: %d bits after %lld received (%lld whole rounds of %d and %d bits of the next) do not complete the last syndrome round "
                  "and bring the final block of %d", nbits, (long long)f->bits, (long long)f->rounds, f->mpr, f->fill, f->mfin);
        return -1;
    }
    if (!meas || !det_rows || !raw_obs) { set_error("null argument"); return -1; }
    return 0;
}

int fe_finish_dev(FrontEnd *f, int32_t nbits, const uint8_t *meas, int64_t stride, int32_t packed, uint8_t *det_rows, int64_t det_stride,
                  int32_t *rows_out, uint32_t *raw_obs, hipStream_t st) {
    if (fe_check_finish(f, nbits, meas, det_rows, raw_obs)) return -1;
    const int64_t q = (f->fill + (int64_t)nbits - f->mfin) / f->mpr, rows = (q + 1) * f->h;
    stride = stride ? stride : fe_dense(nbits, packed); det_stride = det_stride ? det_stride : rows;
    if (stride < fe_dense(nbits, packed) || det_stride < rows) { set_error("front end finish: a stride is shorter than a shot's %d bits / %lld rows", nbits, (long long)rows); return -1; }
    if (rows_out) *rows_out = (int32_t)rows;
    SWD_HIP(hipSetDevice(f->device));
    if (fe_enter(f, st)) return -1;
    // whole rounds before the last one go ahead as a push; the tail launch then holds the rest of one round and the final block
    const int ahead = q >= 2 ? (int)((q - 1) * f->mpr - f->fill) : 0;
    if (ahead && fe_launch(f, ahead, 0, meas, stride, packed ? 1 : 0, det_rows, det_stride, nullptr, false, st)) return -1;
    if (fe_launch(f, nbits - ahead, ahead, meas, stride, packed ? 1 : 0, det_rows + (q >= 2 ? (q - 1) * f->h : 0), det_stride, raw_obs, true, st)) return -1;
    f->finished = true;
    return fe_leave(f, st);
}

// one template into the joint CSR: rows appended to rowptr, entries to off
int fe_ingest(const swd_graph_desc *g, const char *name, int rows, int cols, int lo, std::vector<uint32_t> &rowptr, std::vector<uint16_t> &off) {
    if (!g || !g->row_ptr || (g->nnz > 0 && !g->col_idx)) { set_error("front end: null %s template", name); return -1; }
    if (g->m != rows || g->n != cols) { set_error("front end: the %s template is %d x %d, expected %d x %d", name, g->m, g->n, rows, cols); return -1; }
    if (g->row_ptr[0] != 0) { set_error("front end: %s template: row_ptr must start at 0", name); return -1; }
    for (int r = 0; r < rows; ++r)
        if (g->row_ptr[r + 1] < g->row_ptr[r]) { set_error("front end: %s template: row_ptr decreases at row %d", name, r); return -1; }
    if (g->row_ptr[rows] != g->nnz) { set_error("front end: %s template: row_ptr ends at %d, the descriptor has %d entries", name, g->row_ptr[rows], g->nnz); return -1; }
    for (int r = 0; r < rows; ++r) {
        for (int e = g->row_ptr[r]; e < g->row_ptr[r + 1]; ++e) {
            const int c = g->col_idx[e];
            if (c < lo || c >= cols) { set_error("front end: %s template: row %d reads column %d outside [%d, %d)", name, r, c, lo, cols); return -1; }
            off.push_back((uint16_t)c);
        }
        rowptr.push_back((uint32_t)off.size());
    }
    return 0;
}

} // namespace
} // namespace swd

using namespace swd;

#define SWD_FRONTEND_PROLOGUE(f, h)                     \
    FrontEnd *f = (FrontEnd *)(h);                      \
    if (!f) { set_error("null front end"); return -1; } \
    std::lock_guard<std::mutex> lk(f->mu)

extern "C" swd_frontend *swd_frontend_create(const swd_graph_desc *head, const swd_graph_desc *body, const swd_graph_desc *tail,
                                             const swd_graph_desc *obs_tail, int32_t meas_per_round, int32_t meas_final, int32_t n_half,
                                             int32_t max_shots, int device) {
    const int mpr = meas_per_round, mfin = meas_final, h = n_half;
    if (mpr <= 0 || mfin <= 0 || h <= 0) { set_error("front end: measurements per round, of the final block and rows per round must be positive"); return nullptr; }
    if (max_shots <= 0) { set_error("max_shots must be positive"); return nullptr; }
    if (2 * (int64_t)mpr + mfin > kFeStage) {
        set_error("front end: two rounds of %d measurements and a final block of %d exceed the %d bytes a launch stages", mpr, mfin, kFeStage);
        return nullptr;
    }
    const int nobs = obs_tail ? obs_tail->m : 0;
    if (nobs > 32) { set_error("front end: %d observables; at most 32", nobs); return nullptr; }
    std::vector<uint32_t> rowptr(1, 0);
    std::vector<uint16_t> off;
    // HEAD has no round before it: its entries lie in the second half
    if (fe_ingest(head, "head", h, 2 * mpr, mpr, rowptr, off) || fe_ingest(body, "body", h, 2 * mpr, 0, rowptr, off) ||
        fe_ingest(tail, "tail", h, mpr + mfin, 0, rowptr, off) || (obs_tail && fe_ingest(obs_tail, "observable", nobs, mpr + mfin, 0, rowptr, off)))
        return nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error(SWD_ERR_DEVICE, "no HIP device available: the MI355X decoder has no CPU fallback"); return nullptr; }
    if (device < 0 || device >= ndev) { set_error(SWD_ERR_DEVICE, "device %d out of range (%d devices)", device, ndev); return nullptr; }
    FrontEnd *f = new FrontEnd();
    f->device = device; f->max_shots = max_shots; f->mpr = mpr; f->mfin = mfin; f->h = h; f->nobs = nobs;
    f->state_stride = ((int64_t)2 * mpr + 15) & ~(int64_t)15;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    f->o_off = al(rowptr.size() * 4);
    f->o_state = f->o_off + al(std::max<size_t>(off.size(), 1) * 2);
    f->bytes = f->o_state + al((size_t)max_shots * f->state_stride);
    if (hipSetDevice(device) != hipSuccess || f->dev.reserve(f->bytes) ||
        hipMemcpy(f->dev.p, rowptr.data(), rowptr.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        (!off.empty() && hipMemcpy((char *)f->dev.p + f->o_off, off.data(), off.size() * 2, hipMemcpyHostToDevice) != hipSuccess) ||
        hipStreamCreateWithFlags(&f->st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&f->ev, hipEventDisableTiming) != hipSuccess) {
        set_error(SWD_ERR_DEVICE, "front end: device allocation failed on device %d", device);
        delete f;
        return nullptr;
    }
    return (swd_frontend *)f;
}

extern "C" void swd_frontend_destroy(swd_frontend *h) {
    FrontEnd *f = (FrontEnd *)h;
    if (!f) return;
    (void)hipSetDevice(f->device);
    delete f;
}

extern "C" int swd_frontend_begin(swd_frontend *h, int32_t B) {
    SWD_FRONTEND_PROLOGUE(f, h);
    if (B <= 0 || B > f->max_shots) { set_error("front end begin: %d shots, the front end was created for 1..%d", B, f->max_shots); return -1; }
    SWD_HIP(hipSetDevice(f->device));
    if (fe_enter(f, f->st)) return -1;
    SWD_HIP(hipMemsetAsync((char *)f->dev.p + f->o_state, 0, (size_t)B * f->state_stride, f->st));
    f->B = B; f->bits = 0; f->rounds = 0; f->fill = 0; f->finished = false;
    return fe_leave(f, f->st);
}

extern "C" int swd_frontend_state(swd_frontend *h, int64_t *bits_received, int64_t *rounds_done, int32_t *info, int64_t *device_bytes) {
    SWD_FRONTEND_PROLOGUE(f, h);
    if (bits_received) *bits_received = f->bits;
    if (rounds_done) *rounds_done = f->rounds;
    if (info) {
        const int v[8] = {f->mpr, f->mfin, f->h, f->nobs, f->fill, f->finished ? 1 : 0, f->B, f->max_shots};
        for (int i = 0; i < 8; ++i) info[i] = v[i];
    }
    if (device_bytes) *device_bytes = (int64_t)f->bytes;
    return 0;
}

extern "C" int swd_frontend_push_dev(swd_frontend *h, int32_t nbits, const uint8_t *meas, int64_t stride, int32_t packed, uint8_t *det_rows,
                                     int64_t det_stride, int32_t *rows_out, void *stream) {
    SWD_FRONTEND_PROLOGUE(f, h);
    return fe_push_dev(f, nbits, meas, stride, packed, det_rows, det_stride, rows_out, (hipStream_t)stream);
}

extern "C" int swd_frontend_finish_dev(swd_frontend *h, int32_t nbits, const uint8_t *final_meas, int64_t stride, int32_t packed,
                                       uint8_t *det_rows, int64_t det_stride, int32_t *rows_out, uint32_t *raw_obs, void *stream) {
    SWD_FRONTEND_PROLOGUE(f, h);
    return fe_finish_dev(f, nbits, final_meas, stride, packed, det_rows, det_stride, rows_out, raw_obs, (hipStream_t)stream);
}

extern "C" int swd_frontend_push(swd_frontend *h, int32_t nbits, const uint8_t *meas, int32_t packed, uint8_t *det_rows, int32_t *rows_out) {
    SWD_FRONTEND_PROLOGUE(f, h);
    if (fe_check_push(f, nbits, meas, det_rows)) return -1;
    const size_t in = (size_t)f->B * fe_dense(nbits, packed), rows = (size_t)((f->fill + (int64_t)nbits) / f->mpr * f->h);
    SWD_HIP(hipSetDevice(f->device));
    if (f->hin.reserve(std::max<size_t>(in, 8)) || f->hdet.reserve(std::max<size_t>((size_t)f->B * rows, 8))) return -1;
    if (in) SWD_HIP(hipMemcpyAsync(f->hin.p, meas, in, hipMemcpyHostToDevice, f->st));
    if (fe_push_dev(f, nbits, f->hin.as<uint8_t>(), 0, packed, f->hdet.as<uint8_t>(), 0, rows_out, f->st)) return -1;
    if (rows) SWD_HIP(hipMemcpyAsync(det_rows, f->hdet.p, (size_t)f->B * rows, hipMemcpyDeviceToHost, f->st));
    SWD_HIP(hipStreamSynchronize(f->st));
    return 0;
}

extern "C" int swd_frontend_finish(swd_frontend *h, int32_t nbits, const uint8_t *final_meas, int32_t packed, uint8_t *det_rows,
                                   int32_t *rows_out, uint32_t *raw_obs) {
    SWD_FRONTEND_PROLOGUE(f, h);
    if (fe_check_finish(f, nbits, final_meas, det_rows, raw_obs)) return -1;
    const size_t in = (size_t)f->B * fe_dense(nbits, packed);
    const size_t rows = (size_t)(((f->fill + (int64_t)nbits - f->mfin) / f->mpr + 1) * f->h), o_obs = ((size_t)f->B * rows + 15) & ~(size_t)15;
    SWD_HIP(hipSetDevice(f->device));
    if (f->hin.reserve(std::max<size_t>(in, 8)) || f->hdet.reserve(o_obs + (size_t)f->B * 4)) return -1;
    SWD_HIP(hipMemcpyAsync(f->hin.p, final_meas, in, hipMemcpyHostToDevice, f->st));
    if (fe_finish_dev(f, nbits, f->hin.as<uint8_t>(), 0, packed, f->hdet.as<uint8_t>(), 0, rows_out, (uint32_t *)(f->hdet.as<char>() + o_obs), f->st)) return -1;
    SWD_HIP(hipMemcpyAsync(det_rows, f->hdet.p, (size_t)f->B * rows, hipMemcpyDeviceToHost, f->st));
    SWD_HIP(hipMemcpyAsync(raw_obs, f->hdet.as<char>() + o_obs, (size_t)f->B * 4, hipMemcpyDeviceToHost, f->st));
    SWD_HIP(hipStreamSynchronize(f->st));
    return 0;
}
