// On-device DEM sampler: for every shot, faults e ~ Bernoulli(priors) over the columns of the detector
// error model, det = chk e, obs = obs e over GF(2) -- what `dem.compile_sampler().sample(shots)` hands
// to the reference's harness (/root/reference/osd.py:124-125, guessing.py:129-130).  Stim's generator
// cannot be reproduced, so the stream is the build's own: Philox4x32-10 keyed by the seed, counter =
// (shot, column / 4): the four outputs decide columns 4c..4c+3, fault iff x < round(p * 2^32).  The
// result is a pure function of (seed, shot index, column), independent of batch size and of the GPU a
// shot lands on; tests/philox_ref.py restates it in numpy.
// Further down: the Pauli sampler and the CSS accounting of the code-capacity experiments (same generator, counter word 3 = 1).
#include <string.h>

#include "swd_host.h"

using namespace swd;

namespace {

struct Sampler {
    int device = 0, num_det = 0, num_col = 0, num_obs = 0;
    DevBuf buf;                       // thr[num_col] u32 | colptr[num_col+1] u32 | rows[E] u16 | obs_mask[num_col] u32
    const uint32_t *d_thr = nullptr, *d_colptr = nullptr, *d_obs = nullptr;
    const uint16_t *d_rows = nullptr;
    DevBuf det, obs, faults;          // staging for the host-pointer entry point
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// one workgroup per shot; detector parities accumulate as bits in LDS
__global__ void __launch_bounds__(256) sample_kernel(int num_det, int num_col, const uint32_t *thr, const uint32_t *colptr,
                                                     const uint16_t *rows, const uint32_t *obs_mask, uint64_t seed,
                                                     uint64_t first_shot, uint8_t *det, int64_t det_stride, uint32_t *obs_out,
                                                     uint8_t *faults, int64_t faults_stride) {
    extern __shared__ uint32_t bits[]; // [ceil(num_det / 32)] + 1 word of observable flips
    const int tid = threadIdx.x, nw = (num_det + 31) / 32;
    const uint64_t shot = first_shot + blockIdx.x;
    for (int i = tid; i <= nw; i += 256) bits[i] = 0;
    __syncthreads();
    const int ngroups = (num_col + 3) / 4;
    for (int gidx = tid; gidx < ngroups; gidx += 256) {
        uint32_t x[4];
        philox4x32_10((uint32_t)shot, (uint32_t)(shot >> 32), (uint32_t)gidx, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = 4 * gidx + u;
            if (c >= num_col) break;
            const bool f = x[u] < thr[c];
            if (faults) faults[(int64_t)blockIdx.x * faults_stride + c] = f ? 1 : 0;
            if (f) {
                for (uint32_t e = colptr[c]; e < colptr[c + 1]; ++e) atomicXor(&bits[rows[e] >> 5], 1u << (rows[e] & 31));
                if (obs_mask && obs_mask[c]) atomicXor(&bits[nw], obs_mask[c]);
            }
        }
    }
    __syncthreads();
    for (int r = tid; r < num_det; r += 256) det[(int64_t)blockIdx.x * det_stride + r] = (uint8_t)((bits[r >> 5] >> (r & 31)) & 1u);
    if (tid == 0 && obs_out) obs_out[blockIdx.x] = bits[nw];
}

} // namespace

extern "C" swd_sampler *swd_sampler_create(const swd_graph_desc *chk, const swd_graph_desc *obs, int device) {
    if (!chk || !chk->row_ptr || !chk->col_idx || !chk->channel_probs) { set_error("null argument"); return nullptr; }
    if (chk->m <= 0 || chk->n <= 0 || chk->m > 65535) { set_error("detector matrix %d x %d out of range", chk->m, chk->n); return nullptr; }
    if (obs && (obs->m > 32 || obs->n != chk->n)) { set_error("observable matrix must be (<= 32) x %d", chk->n); return nullptr; }
    {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error(SWD_ERR_DEVICE, "no HIP device available: the MI355X decoder has no CPU fallback"); return nullptr; }
        if (device < 0 || device >= ndev) { set_error(SWD_ERR_DEVICE, "device %d out of range (%d devices)", device, ndev); return nullptr; }
    }
    Sampler *s = new Sampler();
    s->device = device; s->num_det = chk->m; s->num_col = chk->n; s->num_obs = obs ? obs->m : 0;
    const int n = chk->n, E = chk->row_ptr[chk->m];
    std::vector<uint32_t> thr(n), colptr(n + 1, 0), omask(n, 0);
    std::vector<uint16_t> rows(std::max(E, 1));
    for (int c = 0; c < n; ++c) {
        const double p = chk->channel_probs[c];
        if (!(p >= 0.0 && p <= 1.0)) { set_error("prior %d = %g is not a probability", c, p); delete s; return nullptr; }
        const double t = p * 4294967296.0 + 0.5;
        thr[c] = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
    }
    for (int e = 0; e < E; ++e) {
        if (chk->col_idx[e] < 0 || chk->col_idx[e] >= n) { set_error("detector matrix: column out of range"); delete s; return nullptr; }
        colptr[chk->col_idx[e] + 1]++;
    }
    for (int c = 0; c < n; ++c) colptr[c + 1] += colptr[c];
    {
        std::vector<uint32_t> fill(colptr.begin(), colptr.end() - 1);
        for (int r = 0; r < chk->m; ++r)
            for (int e = chk->row_ptr[r]; e < chk->row_ptr[r + 1]; ++e) rows[fill[chk->col_idx[e]]++] = (uint16_t)r;
    }
    if (obs)
        for (int k = 0; k < obs->m; ++k)
            for (int e = obs->row_ptr[k]; e < obs->row_ptr[k + 1]; ++e) {
                if (obs->col_idx[e] < 0 || obs->col_idx[e] >= n) { set_error("observable matrix: column out of range"); delete s; return nullptr; }
                omask[obs->col_idx[e]] ^= 1u << k;
            }
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_thr = 0, o_cp = al(o_thr + n * 4), o_rows = al(o_cp + (n + 1) * 4), o_obs = al(o_rows + rows.size() * 2),
                 total = al(o_obs + n * 4);
    std::vector<char> h(total, 0);
    memcpy(&h[o_thr], thr.data(), n * 4); memcpy(&h[o_cp], colptr.data(), (n + 1) * 4);
    memcpy(&h[o_rows], rows.data(), rows.size() * 2); memcpy(&h[o_obs], omask.data(), n * 4);
    if (hipSetDevice(device) != hipSuccess || s->buf.reserve(total) ||
        hipMemcpy(s->buf.p, h.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        set_error(SWD_ERR_DEVICE, "sampler: device allocation failed on device %d", device);
        delete s;
        return nullptr;
    }
    char *b = (char *)s->buf.p;
    s->d_thr = (const uint32_t *)(b + o_thr); s->d_colptr = (const uint32_t *)(b + o_cp);
    s->d_rows = (const uint16_t *)(b + o_rows); s->d_obs = obs ? (const uint32_t *)(b + o_obs) : nullptr;
    return (swd_sampler *)s;
}

extern "C" void swd_sampler_destroy(swd_sampler *h) { delete (Sampler *)h; }

extern "C" int swd_sampler_sample_dev(swd_sampler *h, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *det,
                                      int64_t det_stride, uint32_t *obs_flips, uint8_t *faults, int64_t faults_stride,
                                      void *stream) {
    Sampler *s = (Sampler *)h;
    if (!s || !det) { set_error("null argument"); return -1; }
    if (B <= 0) return 0;
    SWD_HIP(hipSetDevice(s->device));
    const size_t lds = ((size_t)(s->num_det + 31) / 32 + 1) * 4;
    hipLaunchKernelGGL(sample_kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, s->num_det, s->num_col, s->d_thr, s->d_colptr,
                       s->d_rows, s->d_obs, seed, first_shot, det, det_stride ? det_stride : s->num_det, obs_flips, faults,
                       faults_stride ? faults_stride : s->num_col);
    SWD_HIP(hipGetLastError());
    return 0;
}

extern "C" int swd_sampler_sample(swd_sampler *h, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *det,
                                  uint32_t *obs_flips, uint8_t *faults) {
    Sampler *s = (Sampler *)h;
    if (!s || !det) { set_error("null argument"); return -1; }
    if (B <= 0) return 0;
    SWD_HIP(hipSetDevice(s->device));
    if (s->det.reserve((size_t)B * s->num_det) || s->obs.reserve((size_t)B * 4)) return -1;
    if (faults && s->faults.reserve((size_t)B * s->num_col)) return -1;
    if (swd_sampler_sample_dev(h, B, seed, first_shot, s->det.as<uint8_t>(), 0, s->obs.as<uint32_t>(),
                               faults ? s->faults.as<uint8_t>() : nullptr, 0, nullptr)) return -1;
    SWD_HIP(hipDeviceSynchronize());
    SWD_HIP(hipMemcpy(det, s->det.p, (size_t)B * s->num_det, hipMemcpyDeviceToHost));
    if (obs_flips) SWD_HIP(hipMemcpy(obs_flips, s->obs.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (faults) SWD_HIP(hipMemcpy(faults, s->faults.p, (size_t)B * s->num_col, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int swd_sampler_info(const swd_sampler *h, int32_t *num_det, int32_t *num_col, int32_t *num_obs) {
    const Sampler *s = (const Sampler *)h;
    if (!s) { set_error("null sampler"); return -1; }
    if (num_det) *num_det = s->num_det;
    if (num_col) *num_col = s->num_col;
    if (num_obs) *num_obs = s->num_obs;
    return 0;
}

// ---- code-capacity experiments (include/swd.h: swd_pauli_sampler_*, swd_css_account_*) ---------------------------------------
// The data-noise Monte Carlo of the reference (/root/reference/Misc.ipynb cells 2 and 8, src/simulation.py:15-16) draws its errors and
// judges its corrections on the host; these two kernels do both on the device, so that only counters come back.  Both give a shot one
// wave (four shots share a 256-thread workgroup) while a wave covers the shot's bytes in two strides (n <= 512), else the workgroup;
// the shot's strings live in LDS and every lane computes whole checks by gathering its CSR row from them: no atomics in the
// parities, a fixed order, ordinary vector stores.
namespace {

constexpr int kWaveShotMaxN = 512;   // one wave per shot up to this many qubits (2 strides of 64 lanes x 4 qubits)
constexpr int kCapacityMaxN = 16384; // two padded strings of a shot within 32 KB of LDS

// CSR rows over a shot's LDS bytes: row r is the parity of bytes idx[ptr[r] .. ptr[r + 1])
struct LdsRows {
    std::vector<uint32_t> ptr{0};
    std::vector<uint16_t> idx;
    // rows [r0, r1) of g, column c -> byte `base + c`; -1 with the message set on a bad matrix
    int append(const swd_graph_desc *g, int r0, int r1, int n, int base, const char *what) {
        for (int r = r0; r < r1; ++r) {
            if (g->row_ptr[r] > g->row_ptr[r + 1] || g->row_ptr[r] < 0) { set_error("%s: row_ptr is not monotone", what); return -1; }
            for (int e = g->row_ptr[r]; e < g->row_ptr[r + 1]; ++e) {
                if (g->col_idx[e] < 0 || g->col_idx[e] >= n) { set_error(SWD_ERR_VALUE, "%s: column out of range", what); return -1; }
                idx.push_back((uint16_t)(base + g->col_idx[e]));
            }
            ptr.push_back((uint32_t)idx.size());
        }
        return 0;
    }
};

int capacity_device_ok(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error(SWD_ERR_DEVICE, "no HIP device available: the MI355X decoder has no CPU fallback"); return -1; }
    if (device < 0 || device >= ndev) { set_error(SWD_ERR_DEVICE, "device %d out of range (%d devices)", device, ndev); return -1; }
    return 0;
}

bool csr_desc_ok(const swd_graph_desc *g) { return g && g->row_ptr && g->col_idx && g->m >= 0 && g->n > 0; }

struct PauliSampler {
    int device = 0, n = 0, n4 = 0, mx = 0, mz = 0;
    DevBuf buf;                 // thr[3][n4] u32 (tx | txy | txyz, pad qubits 0) | ptr[mx + mz + 1] u32 | idx[E] u16
    const uint32_t *d_thr = nullptr, *d_ptr = nullptr;
    const uint16_t *d_idx = nullptr;
    DevBuf err, sx, sz;         // staging for the host-pointer entry point
};

// T threads per shot (64: a wave, 256: the workgroup), 256 / T shots per workgroup; LDS [256 / T][2][n4] bytes: X string, Z string
template <int T>
__global__ void __launch_bounds__(256) pauli_sample_kernel(int B, int n, int mx, int mz, const uint32_t *thr, const uint32_t *ptr,
                                                           const uint16_t *idx, uint64_t seed, uint64_t first_shot, uint8_t *err,
                                                           int64_t err_stride, uint8_t *sx, int64_t sx_stride, uint8_t *sz,
                                                           int64_t sz_stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t pauli_lds[];
    const int n4 = (n + 3) & ~3, slot = threadIdx.x / T, lane = threadIdx.x % T;
    const int64_t b = (int64_t)blockIdx.x * (256 / T) + slot;
    const bool live = b < B;
    uint8_t *str = pauli_lds + (size_t)slot * 2 * n4;
    if (live) {
        const uint64_t shot = first_shot + (uint64_t)b;
        for (int g = lane; g < n4 / 4; g += T) {
            uint32_t u[4], xw = 0, zw = 0;
            philox4x32_10((uint32_t)shot, (uint32_t)(shot >> 32), (uint32_t)g, 1u, (uint32_t)seed, (uint32_t)(seed >> 32), u);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = 4 * g + k; // u < tx: X, < txy: Y, < txyz: Z, else I
                xw |= (u[k] < thr[n4 + q] ? 1u : 0u) << (8 * k);
                zw |= (u[k] >= thr[q] && u[k] < thr[2 * n4 + q] ? 1u : 0u) << (8 * k);
            }
            ((uint32_t *)str)[g] = xw;
            ((uint32_t *)(str + n4))[g] = zw;
        }
    }
    __syncthreads();
    if (!live) return;
    uint8_t *e = err + b * err_stride;
    for (int i = lane; i < n; i += T) { e[i] = str[i]; e[n + i] = str[n4 + i]; }
    for (int r = lane; r < mx + mz; r += T) {
        uint32_t p = 0;
        for (uint32_t k = ptr[r]; k < ptr[r + 1]; ++k) p ^= str[idx[k]];
        if (r < mx) sx[b * sx_stride + r] = (uint8_t)p;
        else sz[b * sz_stride + (r - mx)] = (uint8_t)p;
    }
}

struct CssAccount {
    int device = 0, n = 0, len = 0, rows = 0, stab = 0; // len = bytes of a shot's estimate: 2 n, or n in the single-string form
    DevBuf buf;                                         // ptr[rows + 1] u32 | idx[E] u16; stabiliser rows first
    const uint32_t *d_ptr = nullptr;
    const uint16_t *d_idx = nullptr;
};

constexpr int kAccountGrid = 2048; // workgroups of the accounting launch at most: each walks its shots, then adds its sums once

// LDS: cnt[4] u32 | flags[256 / T] u32 | d[256 / T][len] bytes, d = est ^ err
template <int T>
__global__ void __launch_bounds__(256) css_account_kernel(int B, int len, int rows, int stab, const uint32_t *ptr, const uint16_t *idx,
                                                          const uint8_t *est, int64_t est_stride, const uint8_t *err,
                                                          int64_t err_stride, const int32_t *stats, int32_t stat_mask,
                                                          int32_t *result, unsigned long long *counters) {
    extern __shared__ __attribute__((aligned(16))) uint8_t acct_lds[];
    constexpr int SPW = 256 / T;
    uint32_t *cnt = (uint32_t *)acct_lds, *flags = cnt + 4;
    const int slot = threadIdx.x / T, lane = threadIdx.x % T;
    uint8_t *d = acct_lds + 16 + 4 * SPW + (size_t)slot * len;
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    for (int64_t base = (int64_t)blockIdx.x * SPW; base < B; base += (int64_t)gridDim.x * SPW) {
        const int64_t b = base + slot;
        const bool live = b < B;
        if (lane == 0) flags[slot] = 0;
        if (live) {
            const uint8_t *pe = est + b * est_stride, *pr = err + b * err_stride;
            for (int i = lane; i < len; i += T) d[i] = pe[i] ^ pr[i];
        }
        __syncthreads();
        uint32_t f = 0;
        if (live)
            for (int r = lane; r < rows; r += T) {
                uint32_t p = 0;
                for (uint32_t k = ptr[r]; k < ptr[r + 1]; ++k) p ^= d[idx[k]];
                if (p & 1u) f |= r < stab ? 3u : 1u;
            }
        if (f) atomicOr(&flags[slot], f);
        __syncthreads();
        if (live && lane == 0) {
            uint32_t w = flags[slot];
            if (stats && !(stats[b * SWD_STAT_WORDS] & stat_mask)) w |= 4u;
            if (result) result[b] = (int32_t)w;
            atomicAdd(&cnt[0], 1u);
            if (w & 1u) atomicAdd(&cnt[1], 1u);
            if (w & 2u) atomicAdd(&cnt[2], 1u);
            if (w & 4u) atomicAdd(&cnt[3], 1u);
        }
    }
    __syncthreads();
    if (counters && threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd(&counters[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

} // namespace

extern "C" swd_pauli_sampler *swd_pauli_sampler_create(const swd_graph_desc *hx, const swd_graph_desc *hz, const double *px,
                                                       const double *py, const double *pz, int device) {
    if (!csr_desc_ok(hx) || !csr_desc_ok(hz) || !px || !py || !pz) { set_error("null argument"); return nullptr; }
    if (hx->n != hz->n) { set_error("Hx, Hz blocklength does not match!"); return nullptr; }
    const int n = hx->n, n4 = (n + 3) & ~3;
    if (n > kCapacityMaxN || (int64_t)hx->m + hz->m > 65535) {
        set_error(SWD_ERR_VALUE, "Pauli sampler: %d qubits, %d + %d checks out of range (%d qubits, 65535 checks)", n, hx->m, hz->m, kCapacityMaxN);
        return nullptr;
    }
    if (capacity_device_ok(device)) return nullptr;
    std::vector<uint32_t> thr(3 * (size_t)n4, 0);
    auto threshold = [](double v) { const double t = v * 4294967296.0 + 0.5; return t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t; };
    for (int q = 0; q < n; ++q) {
        const double x = px[q], y = py[q], z = pz[q], xy = x + y, xyz = xy + z;
        if (!(x >= 0.0 && x <= 1.0) || !(y >= 0.0 && y <= 1.0) || !(z >= 0.0 && z <= 1.0)) {
            set_error(SWD_ERR_VALUE, "qubit %d: (%g, %g, %g) are not probabilities", q, x, y, z);
            return nullptr;
        }
        if (!(xyz <= 1.0)) { set_error(SWD_ERR_VALUE, "qubit %d: px + py + pz = %.17g exceeds 1", q, xyz); return nullptr; }
        thr[q] = threshold(x); thr[n4 + q] = threshold(xy); thr[2 * (size_t)n4 + q] = threshold(xyz);
    }
    LdsRows rows; // sx = Hx err_z reads the Z string at byte n4, sz = Hz err_x the X string at byte 0
    if (rows.append(hx, 0, hx->m, n, n4, "Hx") || rows.append(hz, 0, hz->m, n, 0, "Hz")) return nullptr;
    PauliSampler *s = new PauliSampler();
    s->device = device; s->n = n; s->n4 = n4; s->mx = hx->m; s->mz = hz->m;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_thr = 0, o_ptr = al(thr.size() * 4), o_idx = al(o_ptr + rows.ptr.size() * 4), total = al(o_idx + rows.idx.size() * 2 + 2);
    std::vector<char> h(total, 0);
    memcpy(&h[o_thr], thr.data(), thr.size() * 4); memcpy(&h[o_ptr], rows.ptr.data(), rows.ptr.size() * 4);
    if (!rows.idx.empty()) memcpy(&h[o_idx], rows.idx.data(), rows.idx.size() * 2);
    if (hipSetDevice(device) != hipSuccess || s->buf.reserve(total) || hipMemcpy(s->buf.p, h.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        set_error(SWD_ERR_DEVICE, "Pauli sampler: device allocation failed on device %d", device);
        delete s;
        return nullptr;
    }
    char *b = (char *)s->buf.p;
    s->d_thr = (const uint32_t *)(b + o_thr); s->d_ptr = (const uint32_t *)(b + o_ptr); s->d_idx = (const uint16_t *)(b + o_idx);
    return (swd_pauli_sampler *)s;
}

extern "C" void swd_pauli_sampler_destroy(swd_pauli_sampler *h) { delete (PauliSampler *)h; }

extern "C" int swd_pauli_sampler_info(const swd_pauli_sampler *h, int32_t *mx, int32_t *mz, int32_t *n) {
    const PauliSampler *s = (const PauliSampler *)h;
    if (!s) { set_error("null sampler"); return -1; }
    if (mx) *mx = s->mx;
    if (mz) *mz = s->mz;
    if (n) *n = s->n;
    return 0;
}

extern "C" int swd_pauli_sampler_sample_dev(swd_pauli_sampler *h, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *err,
                                            int64_t err_stride, uint8_t *sx, int64_t sx_stride, uint8_t *sz, int64_t sz_stride,
                                            void *stream) {
    PauliSampler *s = (PauliSampler *)h;
    if (!s || !err || !sx || !sz) { set_error("null argument"); return -1; }
    if (B <= 0) return 0;
    err_stride = err_stride ? err_stride : 2 * (int64_t)s->n; sx_stride = sx_stride ? sx_stride : s->mx; sz_stride = sz_stride ? sz_stride : s->mz;
    if (err_stride < 2 * (int64_t)s->n || sx_stride < s->mx || sz_stride < s->mz) { set_error("Pauli sampler: a stride is shorter than a shot's row"); return -1; }
    SWD_HIP(hipSetDevice(s->device));
    const bool wave = s->n <= kWaveShotMaxN;
    const int spw = wave ? 4 : 1;
    const size_t lds = (size_t)spw * 2 * s->n4;
    auto kern = wave ? pauli_sample_kernel<64> : pauli_sample_kernel<256>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((B + spw - 1) / spw)), dim3(256), lds, (hipStream_t)stream, B, s->n, s->mx, s->mz, s->d_thr,
                       s->d_ptr, s->d_idx, seed, first_shot, err, err_stride, sx, sx_stride, sz, sz_stride);
    SWD_HIP(hipGetLastError());
    return 0;
}

extern "C" int swd_pauli_sampler_sample(swd_pauli_sampler *h, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *err, uint8_t *sx,
                                        uint8_t *sz) {
    PauliSampler *s = (PauliSampler *)h;
    if (!s || !err || !sx || !sz) { set_error("null argument"); return -1; }
    if (B <= 0) return 0;
    SWD_HIP(hipSetDevice(s->device));
    // (+ 1: a code without checks of one type still gets a device pointer)
    if (s->err.reserve((size_t)B * 2 * s->n) || s->sx.reserve((size_t)B * s->mx + 1) || s->sz.reserve((size_t)B * s->mz + 1)) return -1;
    if (swd_pauli_sampler_sample_dev(h, B, seed, first_shot, s->err.as<uint8_t>(), 0, s->sx.as<uint8_t>(), 0, s->sz.as<uint8_t>(), 0, nullptr))
        return -1;
    SWD_HIP(hipDeviceSynchronize());
    SWD_HIP(hipMemcpy(err, s->err.p, (size_t)B * 2 * s->n, hipMemcpyDeviceToHost));
    if (s->mx) SWD_HIP(hipMemcpy(sx, s->sx.p, (size_t)B * s->mx, hipMemcpyDeviceToHost));
    if (s->mz) SWD_HIP(hipMemcpy(sz, s->sz.p, (size_t)B * s->mz, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" swd_css_account *swd_css_account_create(const swd_graph_desc *cx, int32_t stab_x, const swd_graph_desc *cz, int32_t stab_z,
                                                   int device) {
    if (!cx && !cz) { set_error("CSS accounting: cx and cz are both NULL"); return nullptr; }
    if ((cx && !csr_desc_ok(cx)) || (cz && !csr_desc_ok(cz))) { set_error("null argument"); return nullptr; }
    if (cx && cz && cx->n != cz->n) { set_error("cx, cz blocklength does not match!"); return nullptr; }
    const int n = cx ? cx->n : cz->n;
    const int64_t rows = (int64_t)(cx ? cx->m : 0) + (cz ? cz->m : 0);
    if (n > kCapacityMaxN || rows > 65535) {
        set_error("CSS accounting: %d qubits, %lld rows out of range (%d qubits, 65535 rows)", n, (long long)rows, kCapacityMaxN);
        return nullptr;
    }
    if ((cx && (stab_x < 0 || stab_x > cx->m)) || (cz && (stab_z < 0 || stab_z > cz->m))) {
        set_error("CSS accounting: the stabiliser row count exceeds the matrix");
        return nullptr;
    }
    if (capacity_device_ok(device)) return nullptr;
    // a shot's LDS bytes mirror its estimate: [X string | Z string] (cx reads the Z string), or the one string of the single-string form
    const int zbase = cx && cz ? n : 0;
    LdsRows lr;
    if ((cx && lr.append(cx, 0, stab_x, n, zbase, "cx")) || (cz && lr.append(cz, 0, stab_z, n, 0, "cz")) ||
        (cx && lr.append(cx, stab_x, cx->m, n, zbase, "cx")) || (cz && lr.append(cz, stab_z, cz->m, n, 0, "cz")))
        return nullptr;
    CssAccount *a = new CssAccount();
    a->device = device; a->n = n; a->len = cx && cz ? 2 * n : n; a->rows = (int)rows; a->stab = (cx ? stab_x : 0) + (cz ? stab_z : 0);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_idx = al(lr.ptr.size() * 4), total = al(o_idx + lr.idx.size() * 2 + 2);
    std::vector<char> h(total, 0);
    memcpy(&h[0], lr.ptr.data(), lr.ptr.size() * 4);
    if (!lr.idx.empty()) memcpy(&h[o_idx], lr.idx.data(), lr.idx.size() * 2);
    if (hipSetDevice(device) != hipSuccess || a->buf.reserve(total) || hipMemcpy(a->buf.p, h.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        set_error(SWD_ERR_DEVICE, "CSS accounting: device allocation failed on device %d", device);
        delete a;
        return nullptr;
    }
    a->d_ptr = (const uint32_t *)a->buf.p; a->d_idx = (const uint16_t *)((char *)a->buf.p + o_idx);
    return (swd_css_account *)a;
}

extern "C" void swd_css_account_destroy(swd_css_account *h) { delete (CssAccount *)h; }

extern "C" int swd_css_account_dev(swd_css_account *h, int32_t B, const uint8_t *est, int64_t est_stride, const uint8_t *err,
                                   int64_t err_stride, const int32_t *stats, int32_t stat_mask, int32_t *result, uint64_t *counters,
                                   void *stream) {
    CssAccount *a = (CssAccount *)h;
    if (!a || !est || !err) { set_error("null argument"); return -1; }
    if (B <= 0) return 0;
    est_stride = est_stride ? est_stride : a->len; err_stride = err_stride ? err_stride : a->len;
    if (est_stride < a->len || err_stride < a->len) { set_error("CSS accounting: a stride is shorter than a shot's %d bytes", a->len); return -1; }
    SWD_HIP(hipSetDevice(a->device));
    const bool wave = a->n <= kWaveShotMaxN && a->rows <= 4 * kWaveShotMaxN;
    const int spw = wave ? 4 : 1;
    const size_t lds = 16 + 4 * (size_t)spw + (size_t)spw * a->len;
    const int64_t groups = ((int64_t)B + spw - 1) / spw;
    auto kern = wave ? css_account_kernel<64> : css_account_kernel<256>;
    hipLaunchKernelGGL(kern, dim3((unsigned)std::min<int64_t>(groups, kAccountGrid)), dim3(256), lds, (hipStream_t)stream, B, a->len, a->rows,
                       a->stab, a->d_ptr, a->d_idx, est, est_stride, err, err_stride, stats, stat_mask, result,
                       (unsigned long long *)counters);
    SWD_HIP(hipGetLastError());
    return 0;
}

// ---- memory experiments (include/swd.h: swd_shot_account_dev) ------------------------------------------------------------------------
// The last lines of the reference's sliding_window_decoder (/root/reference/osd.py:181-191) for a batch of the window loop: the
// decisions the pipeline left in shot_result against the sampler's true observable flips, and the per-window records reduced to
// counts.  One thread per shot, the grid walks the shots like css_account_kernel; a wave counts with ballots, the workgroup sums
// in LDS and adds each non-zero sum to the global counters once.  Everything is integer: no result depends on arrival order.
namespace {

constexpr int kWindowTile = 64; // windows whose counters a workgroup keeps in LDS at a time (64 x 10 x 8 B = 5 KB)

__global__ void __launch_bounds__(256) shot_account_kernel(int B, int W, const int32_t *shot_result, const uint32_t *true_flips,
                                                           const int32_t *stats, uint64_t first_shot, int32_t *result,
                                                           unsigned long long *counters, unsigned long long *window_counters,
                                                           unsigned long long *failed, int failed_cap) {
    __shared__ unsigned long long hist[kWindowTile * SWD_WINDOW_COUNTER_WORDS];
    __shared__ unsigned long long fail_base;
    __shared__ uint32_t cnt[4], wave_fail[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool windows = stats && window_counters && W > 0;
    if (tid < 4) cnt[tid] = 0;
    // the shots are walked once per tile of windows; the per-shot part belongs to the first walk
    for (int t0 = 0; t0 == 0 || (windows && t0 < W); t0 += kWindowTile) {
        const int nt = windows ? min(kWindowTile, W - t0) : 0;
        for (int i = tid; i < nt * SWD_WINDOW_COUNTER_WORDS; i += 256) hist[i] = 0;
        __syncthreads();
        for (int64_t base = (int64_t)blockIdx.x * 256; base < B; base += (int64_t)gridDim.x * 256) {
            const int64_t b = base + tid;
            const bool live = b < B;
            if (t0 == 0) {
                uint32_t w = 0;
                if (live) {
                    if (shot_result[2 * b + 1] != 0) w |= 2u;
                    if ((uint32_t)shot_result[2 * b] != true_flips[b]) w |= 4u;
                    if (w) w |= 1u; // np.logical_or(flagged_err, logical_err), osd.py:184-188
                    if (result) result[b] = (int32_t)w;
                }
                const unsigned long long m_live = __ballot(live), m_fail = __ballot(w & 1u), m_flag = __ballot(w & 2u), m_obs = __ballot(w & 4u);
                const unsigned long long m = lane == 0 ? m_live : lane == 1 ? m_fail : lane == 2 ? m_flag : m_obs;
                if (lane < 4 && m) atomicAdd(&cnt[lane], (uint32_t)__popcll(m));
                if (failed) { // slots for the pass's failing shots: counted in LDS, reserved with one atomic
                    if (lane == 0) wave_fail[wave] = (uint32_t)__popcll(m_fail);
                    __syncthreads();
                    const uint32_t n = wave_fail[0] + wave_fail[1] + wave_fail[2] + wave_fail[3];
                    if (tid == 0 && n) fail_base = atomicAdd(&failed[0], (unsigned long long)n);
                    __syncthreads();
                    if (w & 1u) {
                        uint32_t before = (uint32_t)__popcll(m_fail & ((1ull << lane) - 1ull));
                        for (int k = 0; k < wave; ++k) before += wave_fail[k];
                        const unsigned long long slot = fail_base + before;
                        if (slot < (unsigned long long)failed_cap) failed[1 + slot] = first_shot + (uint64_t)b;
                    }
                    __syncthreads(); // (the next pass writes wave_fail and fail_base again)
                }
            }
            for (int t = 0; t < nt; ++t) {
                const int32_t *st = stats + (live ? (b * W + (t0 + t)) * SWD_STAT_WORDS : 0); // words 0 and 1 only
                const int32_t s0 = live ? st[0] : 0, s1 = live ? st[1] : 0;
                unsigned long long mine = 0, its = (unsigned long long)(long long)s1;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const unsigned long long mc = __ballot(live && (s0 & 7) == c);
                    if (lane == c) mine = (unsigned long long)__popcll(mc);
                }
                const unsigned long long mn = __ballot(live && !(s0 & SWD_STATUS_CONVERGE));
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) its += __shfl_xor(its, off);
                if (lane == 8) mine = (unsigned long long)__popcll(mn);
                if (lane == 9) mine = its;
                if (lane < SWD_WINDOW_COUNTER_WORDS && mine) atomicAdd(&hist[t * SWD_WINDOW_COUNTER_WORDS + lane], mine);
            }
        }
        __syncthreads();
        for (int i = tid; i < nt * SWD_WINDOW_COUNTER_WORDS; i += 256)
            if (hist[i]) atomicAdd(&window_counters[(size_t)t0 * SWD_WINDOW_COUNTER_WORDS + i], hist[i]);
        __syncthreads();
    }
    if (counters && tid < 4 && cnt[tid]) atomicAdd(&counters[tid], (unsigned long long)cnt[tid]);
}

} // namespace

extern "C" int swd_shot_account_dev(int device, int32_t B, int32_t W, const int32_t *shot_result, const uint32_t *true_flips,
                                    const int32_t *stats, uint64_t first_shot, int32_t *result, uint64_t *counters,
                                    uint64_t *window_counters, uint64_t *failed, int32_t failed_cap, void *stream) {
    if (B <= 0) return 0;
    if (!shot_result || !true_flips) { set_error("null argument"); return -1; }
    if (W < 0 || (failed && failed_cap < 0)) { set_error("shot accounting: W = %d, failed_cap = %d must not be negative", W, failed_cap); return -1; }
    if (capacity_device_ok(device)) return -1;
    SWD_HIP(hipSetDevice(device));
    const int64_t groups = ((int64_t)B + 255) / 256;
    hipLaunchKernelGGL(shot_account_kernel, dim3((unsigned)std::min<int64_t>(groups, kAccountGrid)), dim3(256), 0, (hipStream_t)stream, B, W,
                       shot_result, true_flips, stats, first_shot, result, (unsigned long long *)counters,
                       (unsigned long long *)window_counters, (unsigned long long *)failed, failed ? failed_cap : 0);
    SWD_HIP(hipGetLastError());
    return 0;
}

// ---- memory experiments: logical errors per group of observables (include/swd.h: swd_group_account_dev) ------------------------------
// "Any observable of a subset wrong" -- the X and the Z logical error rate of a two-basis experiment -- cannot be had from
// shot_account_kernel's counts, so it is a launch of its own, made only when groups are asked for.  The same shape: one thread per
// shot, the grid walks the shots, a ballot per mask, the workgroup sums in LDS and adds each non-zero sum to its counter once.
namespace {

struct GroupMasks { uint32_t m[SWD_MAX_OBSERVABLE_GROUPS]; };

__global__ void __launch_bounds__(256) group_account_kernel(int B, int G, const int32_t *shot_result, const uint32_t *true_flips,
                                                            GroupMasks masks, unsigned long long *counters) {
    __shared__ uint32_t cnt[SWD_MAX_OBSERVABLE_GROUPS];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < SWD_MAX_OBSERVABLE_GROUPS) cnt[tid] = 0;
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * 256; base < B; base += (int64_t)gridDim.x * 256) {
        const int64_t b = base + tid;
        const uint32_t diff = b < B ? (uint32_t)shot_result[2 * b] ^ true_flips[b] : 0u; // (a shot past B has no wrong observable)
        unsigned long long m = 0;
#pragma unroll
        for (int g = 0; g < SWD_MAX_OBSERVABLE_GROUPS; ++g) {
            const unsigned long long mg = __ballot(diff & masks.m[g]);
            if (lane == g) m = mg;
        }
        if (lane < G && m) atomicAdd(&cnt[lane], (uint32_t)__popcll(m));
    }
    __syncthreads();
    if (tid < G && cnt[tid]) atomicAdd(&counters[tid], (unsigned long long)cnt[tid]);
}

} // namespace

extern "C" int swd_group_account_dev(int device, int32_t B, const int32_t *shot_result, const uint32_t *true_flips, int32_t num_groups,
                                     const uint32_t *masks, uint64_t *counters, void *stream) {
    if (num_groups < 0 || num_groups > SWD_MAX_OBSERVABLE_GROUPS) {
        set_error("group accounting: %d groups, at most %d", num_groups, SWD_MAX_OBSERVABLE_GROUPS);
        return -1;
    }
    if (B <= 0 || num_groups == 0) return 0;
    if (!shot_result || !true_flips || !masks || !counters) { set_error("null argument"); return -1; }
    if (capacity_device_ok(device)) return -1;
    SWD_HIP(hipSetDevice(device));
    GroupMasks gm = {};
    for (int g = 0; g < num_groups; ++g) gm.m[g] = masks[g];
    const int64_t groups = ((int64_t)B + 255) / 256;
    hipLaunchKernelGGL(group_account_kernel, dim3((unsigned)std::min<int64_t>(groups, kAccountGrid)), dim3(256), 0, (hipStream_t)stream, B,
                       (int)num_groups, shot_result, true_flips, gm, (unsigned long long *)counters);
    SWD_HIP(hipGetLastError());
    return 0;
}

// ---- rolling DEM sampler (include/swd.h: swd_rolling_sampler_*)------------------------------------------------------------------------
// The detector rows of an experiment of ANY number of rounds from a periodic template of R0 rounds, a few row blocks per call: what a
// memory experiment on a rolling session feeds its windows with.  A call emits the rows of row blocks block0 .. block0 + nblocks - 1
// and for that draws the column blocks block0 - 1 .. block0 + nblocks - 1 of the R-round model -- a contiguous range of its GLOBAL
// columns, each mapped to a template column by a table of at most eight entries (one per column block) that the host fills in.  The
// stream is sample_kernel's on the global column, so the rows are those of swd_sampler_* on the R-round model.  A call covers few rows
// and one or two thousand columns, so the shape is the Pauli sampler's: a wave per shot, four shots per workgroup (the workgroup per
// shot when the columns are many); the shot's row bits and observable word live in LDS, faults scatter into them with atomicXor, rows
// outside the emitted range are dropped.  Lanes of shots past B stay predicated to the last barrier.
namespace {

constexpr int kRollEntries = 8;     // column blocks one launch draws: the one before the first emitted row block and up to 7 more
constexpr int kRollMaxRows = 65504; // rows one launch emits at most: 2047 words of row bits + the observable word, 32 KB for four shots
constexpr int kRollWaveCols = 2048; // up to this many columns a wave draws a shot, beyond it the workgroup

struct RollCall {
    uint64_t g0, g1;                // global columns drawn: [g0, g1) = the entries' columns, in order and without gaps
    uint64_t fcol0;                 // the global column that faults[..][0] stands for
    uint64_t gstart[kRollEntries];  // per entry: first global column,
    uint32_t tstart[kRollEntries];  //   first template column,
    uint32_t len[kRollEntries];     //   number of columns,
    int32_t rshift[kRollEntries];   //   the block's first row relative to the first emitted row (-h for the block before it),
    uint32_t counted;               //   bit e: its observable masks and faults belong to this call
    int32_t n, nrows;
};

struct RollingSampler {
    int device = 0, h = 0, ncol = 0, nobs = 0, R0 = 0, j0 = 0, j1 = 0, nblk = 0;
    std::vector<int64_t> anchor;    // template: first column of every block, then ncol
    DevBuf buf;                     // thr[ncol] u32 | colptr[ncol + 1] u32 | rows[E] u16, relative to the block's first row | obs_mask[ncol] u32
    const uint32_t *d_thr = nullptr, *d_colptr = nullptr, *d_obs = nullptr;
    const uint16_t *d_rows = nullptr;
    DevBuf det, obs, faults;        // staging for the host-pointer entry point

    int64_t cs() const { return anchor[j0 + 1] - anchor[j0]; }
    int least_rounds() const { return R0 - (j1 - j0); }
    // column block b of the model of `rounds` rounds: its first global column, its template block
    void block(int rounds, int b, int64_t *g, int *tb) const {
        const int64_t up = rounds - R0, nbody = (j1 - j0) + up;
        if (b < j0) { *tb = b; *g = anchor[b]; }
        else if (b < j0 + nbody) { *tb = j0; *g = anchor[j0] + (int64_t)(b - j0) * cs(); }
        else { *tb = (int)(b - up); *g = anchor[*tb] + up * cs(); }
    }
    int64_t first_col(int rounds, int b) const { // b = rounds + 1: the model's number of columns
        if (b == rounds + 1) return anchor[nblk] + (int64_t)(rounds - R0) * cs();
        int64_t g; int tb;
        block(rounds, b, &g, &tb);
        return g;
    }
};

// T threads per shot (64: a wave, 256: the workgroup), 256 / T shots per workgroup; LDS [256 / T][words of row bits + 1]
template <int T>
__global__ void __launch_bounds__(256) rolling_rows_kernel(int B, RollCall call, const uint32_t *thr, const uint32_t *colptr,
                                                           const uint16_t *rows, const uint32_t *obs_mask, uint64_t seed,
                                                           uint64_t first_shot, uint8_t *det, int64_t det_stride, uint32_t *obs_flips,
                                                           uint8_t *faults, int64_t faults_stride) {
    extern __shared__ uint32_t roll_bits[];
    __shared__ RollCall tb; // (the entries are looked up with a per-lane index)
    const int nrows = call.nrows, nw = (nrows + 31) >> 5, slot = threadIdx.x / T, lane = threadIdx.x % T;
    uint32_t *bits = roll_bits + (size_t)slot * (nw + 1);
    const int64_t b = (int64_t)blockIdx.x * (256 / T) + slot;
    const bool live = b < B;
    if (threadIdx.x == 0) tb = call;
    for (int i = lane; i <= nw; i += T) bits[i] = 0;
    __syncthreads();
    if (live) {
        const uint64_t shot = first_shot + (uint64_t)b, g0 = call.g0, g1 = call.g1;
        const uint32_t gfirst = (uint32_t)(g0 >> 2), ngroups = (uint32_t)((g1 - 1) >> 2) - gfirst + 1;
        for (uint32_t gi = lane; gi < ngroups; gi += T) {
            const uint32_t g = gfirst + gi;
            uint32_t x[4];
            philox4x32_10((uint32_t)shot, (uint32_t)(shot >> 32), g, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
            int e = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint64_t c = ((uint64_t)g << 2) + u;
                if (c < g0 || c >= g1) continue;
                while (c >= tb.gstart[e] + tb.len[e]) ++e; // (c < g1 = the end of the last entry)
                const uint32_t tc = tb.tstart[e] + (uint32_t)(c - tb.gstart[e]);
                const bool f = x[u] < thr[tc], mine = (tb.counted >> e) & 1u;
                if (faults && mine) faults[b * faults_stride + (int64_t)(c - call.fcol0)] = f ? 1 : 0;
                if (f) {
                    const int shift = tb.rshift[e];
                    for (uint32_t k = colptr[tc]; k < colptr[tc + 1]; ++k) {
                        const int r = shift + (int)rows[k];
                        if (r >= 0 && r < nrows) atomicXor(&bits[r >> 5], 1u << (r & 31));
                    }
                    if (mine && obs_mask && obs_mask[tc]) atomicXor(&bits[nw], obs_mask[tc]);
                }
            }
        }
    }
    __syncthreads();
    if (live) {
        for (int r = lane; r < nrows; r += T) det[b * det_stride + r] = (uint8_t)((bits[r >> 5] >> (r & 31)) & 1u);
        if (lane == 0 && obs_flips) obs_flips[b] ^= bits[nw];
    }
}

// one launch: the rows of row blocks b0 .. b0 + n - 1 (n <= kRollEntries - 1, n h <= kRollMaxRows)
int rolling_launch(RollingSampler *s, int B, uint64_t seed, uint64_t first_shot, int rounds, int b0, int n, uint8_t *det, int64_t stride,
                   uint32_t *obs_flips, uint8_t *faults, int64_t faults_stride, uint64_t fcol0, hipStream_t st) {
    RollCall c{};
    for (int b = std::max(b0 - 1, 0); b < b0 + n; ++b) {
        int64_t g; int tb;
        s->block(rounds, b, &g, &tb);
        const int e = c.n++;
        c.gstart[e] = (uint64_t)g; c.tstart[e] = (uint32_t)s->anchor[tb]; c.len[e] = (uint32_t)(s->anchor[tb + 1] - s->anchor[tb]);
        c.rshift[e] = (b - b0) * s->h;
        if (b >= b0) c.counted |= 1u << e;
    }
    c.g0 = c.gstart[0]; c.g1 = c.gstart[c.n - 1] + c.len[c.n - 1]; c.fcol0 = fcol0; c.nrows = n * s->h;
    const bool wave = c.g1 - c.g0 <= (uint64_t)kRollWaveCols;
    const int spw = wave ? 4 : 1;
    const size_t lds = (size_t)spw * ((size_t)(c.nrows + 31) / 32 + 1) * 4;
    auto kern = wave ? rolling_rows_kernel<64> : rolling_rows_kernel<256>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((B + spw - 1) / spw)), dim3(256), lds, st, B, c, s->d_thr, s->d_colptr, s->d_rows, s->d_obs, seed,
                       first_shot, det, stride, obs_flips, faults, faults_stride);
    SWD_HIP(hipGetLastError());
    return 0;
}

// the checks of a call; -> the first column and the number of columns of column blocks block0 .. block0 + nblocks - 1
int rolling_range(const RollingSampler *s, int rounds, int block0, int nblocks, int64_t *col0, int64_t *ncols) {
    if (rounds < s->least_rounds()) {
        set_error("rolling sampler: %d rounds; a template of %d rounds with %d body rounds serves %d rounds and more", rounds, s->R0, s->j1 - s->j0,
                  s->least_rounds());
        return -1;
    }
    if (rounds >= 1 << 30 || s->first_col(rounds, rounds + 1) >= (int64_t)1 << 34) {
        set_error("rolling sampler: the model of %d rounds has 2^34 columns or more (%lld per round): they do not fit the generator's counter", rounds,
                  (long long)s->cs());
        return -1;
    }
    if (block0 < 0 || nblocks <= 0 || (int64_t)block0 + nblocks > (int64_t)rounds + 1) {
        set_error("rolling sampler: row blocks %d .. %lld are not within the %d + 1 blocks of the experiment", block0, (long long)block0 + nblocks - 1, rounds);
        return -1;
    }
    *col0 = s->first_col(rounds, block0);
    *ncols = s->first_col(rounds, block0 + nblocks) - *col0;
    return 0;
}

} // namespace

extern "C" swd_rolling_sampler *swd_rolling_sampler_create(const swd_graph_desc *chk, const swd_graph_desc *obs, int32_t n_half, int32_t j0,
                                                           int32_t j1, const int64_t *anchor_cols, int32_t num_blocks, int device) {
    if (!chk || !chk->row_ptr || !chk->col_idx || !chk->channel_probs || !anchor_cols) { set_error("null argument"); return nullptr; }
    const int h = n_half, n = chk->n, nb = num_blocks;
    if (h <= 0 || h > 65535 / 2) { set_error(SWD_ERR_VALUE, "rolling sampler: n_half = %d out of range (1 .. 32767: a column's rows are 16-bit offsets within two blocks)", h); return nullptr; }
    if (nb <= 0 || n <= 0 || (int64_t)chk->m != (int64_t)nb * h) { set_error(SWD_ERR_VALUE, "rolling sampler: %d detector rows are not %d blocks of %d", chk->m, nb, h); return nullptr; }
    if (obs && (!obs->row_ptr || !obs->col_idx || obs->m > 32 || obs->n != n)) { set_error(SWD_ERR_VALUE, "observable matrix must be (<= 32) x %d: at most 32 observables", n); return nullptr; }
    if (j0 < 0 || j1 <= j0 || j1 > nb - 1) { set_error(SWD_ERR_VALUE, "rolling sampler: body blocks %d .. %d are not within the %d blocks (a tail block must follow)", j0, j1 - 1, nb); return nullptr; }
    if (anchor_cols[0] != 0 || anchor_cols[nb] != n) { set_error(SWD_ERR_VALUE, "rolling sampler: anchor columns must run from 0 to %d", n); return nullptr; }
    for (int b = 0; b < nb; ++b)
        if (anchor_cols[b + 1] <= anchor_cols[b]) { set_error(SWD_ERR_VALUE, "rolling sampler: anchor columns must increase (block %d)", b); return nullptr; }
    if (capacity_device_ok(device)) return nullptr;
    const int E = chk->row_ptr[chk->m];
    std::vector<uint32_t> thr(n), colptr(n + 1, 0), omask(n, 0);
    std::vector<int> block_of(n);
    std::vector<uint16_t> rows(std::max(E, 1));
    for (int b = 0; b < nb; ++b)
        for (int64_t c = anchor_cols[b]; c < anchor_cols[b + 1]; ++c) block_of[c] = b;
    for (int c = 0; c < n; ++c) {
        const double p = chk->channel_probs[c];
        if (!(p >= 0.0 && p <= 1.0)) { set_error("prior %d = %g is not a probability", c, p); return nullptr; }
        const double t = p * 4294967296.0 + 0.5;
        thr[c] = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
    }
    for (int e = 0; e < E; ++e) {
        if (chk->col_idx[e] < 0 || chk->col_idx[e] >= n) { set_error("detector matrix: column out of range"); return nullptr; }
        colptr[chk->col_idx[e] + 1]++;
    }
    for (int c = 0; c < n; ++c) colptr[c + 1] += colptr[c];
    {
        std::vector<uint32_t> fill(colptr.begin(), colptr.end() - 1);
        for (int r = 0; r < chk->m; ++r)
            for (int e = chk->row_ptr[r]; e < chk->row_ptr[r + 1]; ++e) {
                const int c = chk->col_idx[e], b = block_of[c];
                if (r < b * h || r >= (b + 2) * h) { // (r < chk->m = nb h holds: the last block keeps to its own rows)
                    set_error(SWD_ERR_VALUE, "rolling sampler: column %d of round block %d touches row %d, outside the rows [%d, %d) of blocks %d and %d", c, b, r,
                              b * h, (b + 2) * h, b, b + 1);
                    return nullptr;
                }
                rows[fill[c]++] = (uint16_t)(r - b * h);
            }
    }
    if (obs)
        for (int k = 0; k < obs->m; ++k)
            for (int e = obs->row_ptr[k]; e < obs->row_ptr[k + 1]; ++e) {
                if (obs->col_idx[e] < 0 || obs->col_idx[e] >= n) { set_error(SWD_ERR_VALUE, "observable matrix: column out of range"); return nullptr; }
                omask[obs->col_idx[e]] ^= 1u << k;
            }
    // the body blocks: translates of block j0 -- the rows are relative already
    const int64_t a0 = anchor_cols[j0], cs = anchor_cols[j0 + 1] - a0;
    for (int j = j0 + 1; j < j1; ++j) {
        const int64_t aj = anchor_cols[j];
        if (anchor_cols[j + 1] - aj != cs) {
            set_error(SWD_ERR_VALUE, "rolling sampler: the body blocks are not translates: block %d has %lld columns, block %d has %lld", j, (long long)(anchor_cols[j + 1] - aj), j0, (long long)cs);
            return nullptr;
        }
        for (int64_t i = 0; i < cs; ++i) {
            const uint32_t da = colptr[a0 + i + 1] - colptr[a0 + i], db = colptr[aj + i + 1] - colptr[aj + i];
            const char *what = thr[a0 + i] != thr[aj + i] ? "prior" : omask[a0 + i] != omask[aj + i] ? "observable mask" : da != db ? "rows" : nullptr;
            for (uint32_t e = 0; !what && e < da; ++e)
                if (rows[colptr[a0 + i] + e] != rows[colptr[aj + i] + e]) what = "rows";
            if (what) {
                set_error(SWD_ERR_VALUE, "rolling sampler: the body blocks are not translates: column %lld of block %d differs from that of block %d in its %s", (long long)i, j, j0, what);
                return nullptr;
            }
        }
    }
    RollingSampler *s = new RollingSampler();
    s->device = device; s->h = h; s->ncol = n; s->nobs = obs ? obs->m : 0; s->R0 = nb - 1; s->j0 = j0; s->j1 = j1; s->nblk = nb;
    s->anchor.assign(anchor_cols, anchor_cols + nb + 1);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_thr = 0, o_cp = al(o_thr + (size_t)n * 4), o_rows = al(o_cp + ((size_t)n + 1) * 4), o_obs = al(o_rows + rows.size() * 2),
                 total = al(o_obs + (size_t)n * 4);
    std::vector<char> hb(total, 0);
    memcpy(&hb[o_thr], thr.data(), (size_t)n * 4); memcpy(&hb[o_cp], colptr.data(), ((size_t)n + 1) * 4);
    memcpy(&hb[o_rows], rows.data(), rows.size() * 2); memcpy(&hb[o_obs], omask.data(), (size_t)n * 4);
    if (hipSetDevice(device) != hipSuccess || s->buf.reserve(total) || hipMemcpy(s->buf.p, hb.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        set_error(SWD_ERR_DEVICE, "rolling sampler: device allocation failed on device %d", device);
        delete s;
        return nullptr;
    }
    char *bp = (char *)s->buf.p;
    s->d_thr = (const uint32_t *)(bp + o_thr); s->d_colptr = (const uint32_t *)(bp + o_cp);
    s->d_rows = (const uint16_t *)(bp + o_rows); s->d_obs = obs ? (const uint32_t *)(bp + o_obs) : nullptr;
    return (swd_rolling_sampler *)s;
}

extern "C" void swd_rolling_sampler_destroy(swd_rolling_sampler *h) { delete (RollingSampler *)h; }

extern "C" int swd_rolling_sampler_info(const swd_rolling_sampler *h, int32_t *info, int32_t rounds, int32_t block0, int32_t nblocks,
                                        int64_t *first_col, int64_t *num_cols) {
    const RollingSampler *s = (const RollingSampler *)h;
    if (!s) { set_error("null sampler"); return -1; }
    if (info) {
        const int v[8] = {s->h, s->ncol, s->nobs, s->R0, s->j0, s->j1, s->least_rounds(), 0};
        for (int i = 0; i < 8; ++i) info[i] = v[i];
    }
    if (rounds >= 0 && (first_col || num_cols)) {
        int64_t c0, nc;
        if (rolling_range(s, rounds, block0, nblocks, &c0, &nc)) return -1;
        if (first_col) *first_col = c0;
        if (num_cols) *num_cols = nc;
    }
    return 0;
}

extern "C" int swd_rolling_sampler_rows_dev(swd_rolling_sampler *h, int32_t B, uint64_t seed, uint64_t first_shot, int32_t rounds,
                                            int32_t block0, int32_t nblocks, uint8_t *det_rows, int64_t stride, uint32_t *obs_flips,
                                            uint8_t *faults, int64_t faults_stride, void *stream) {
    RollingSampler *s = (RollingSampler *)h;
    if (!s || !det_rows) { set_error("null argument"); return -1; }
    int64_t col0, ncols;
    if (rolling_range(s, rounds, block0, nblocks, &col0, &ncols)) return -1;
    if (B <= 0) return 0;
    const int64_t nrows = (int64_t)nblocks * s->h;
    stride = stride ? stride : nrows; faults_stride = faults_stride ? faults_stride : ncols;
    if (stride < nrows || (faults && faults_stride < ncols)) { set_error("rolling sampler: a stride is shorter than a shot's %lld rows / %lld columns", (long long)nrows, (long long)ncols); return -1; }
    SWD_HIP(hipSetDevice(s->device));
    const int per = std::max(1, std::min(kRollEntries - 1, kRollMaxRows / s->h));
    for (int b = block0; b < block0 + nblocks; b += per) {
        const int n = std::min(per, block0 + nblocks - b);
        if (rolling_launch(s, B, seed, first_shot, rounds, b, n, det_rows + (int64_t)(b - block0) * s->h, stride, obs_flips, faults, faults_stride,
                           (uint64_t)col0, (hipStream_t)stream))
            return -1;
    }
    return 0;
}

extern "C" int swd_rolling_sampler_rows(swd_rolling_sampler *h, int32_t B, uint64_t seed, uint64_t first_shot, int32_t rounds, int32_t block0,
                                        int32_t nblocks, uint8_t *det_rows, uint32_t *obs_flips, uint8_t *faults) {
    RollingSampler *s = (RollingSampler *)h;
    if (!s || !det_rows) { set_error("null argument"); return -1; }
    int64_t col0, ncols;
    if (rolling_range(s, rounds, block0, nblocks, &col0, &ncols)) return -1;
    if (B <= 0) return 0;
    const size_t nrows = (size_t)nblocks * s->h;
    SWD_HIP(hipSetDevice(s->device));
    if (s->det.reserve((size_t)B * nrows) || s->obs.reserve((size_t)B * 4) || (faults && s->faults.reserve((size_t)B * (size_t)ncols))) return -1;
    if (obs_flips) SWD_HIP(hipMemcpy(s->obs.p, obs_flips, (size_t)B * 4, hipMemcpyHostToDevice));
    if (swd_rolling_sampler_rows_dev(h, B, seed, first_shot, rounds, block0, nblocks, s->det.as<uint8_t>(), 0, obs_flips ? s->obs.as<uint32_t>() : nullptr,
                                     faults ? s->faults.as<uint8_t>() : nullptr, 0, nullptr))
        return -1;
    SWD_HIP(hipDeviceSynchronize());
    SWD_HIP(hipMemcpy(det_rows, s->det.p, (size_t)B * nrows, hipMemcpyDeviceToHost));
    if (obs_flips) SWD_HIP(hipMemcpy(obs_flips, s->obs.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (faults) SWD_HIP(hipMemcpy(faults, s->faults.p, (size_t)B * (size_t)ncols, hipMemcpyDeviceToHost));
    return 0;
}

// ---- diagnostics: a foreign kernel that holds workgroup slots for a bounded time (include/swd.h: swd_diag_occupy) ----
namespace swd {
__global__ void __launch_bounds__(1024) occupy_kernel(long long ticks, uint32_t *sink) {
    extern __shared__ __attribute__((aligned(16))) char occ_smem[];
    const long long t0 = wall_clock64(); // constant 100 MHz counter
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
    if (sink && threadIdx.x == 0 && occ_smem[0] == 77) sink[0] = 1u; // (keeps the LDS allocation alive)
}
} // namespace swd

extern "C" int swd_diag_occupy(int device, int32_t blocks, int32_t threads, int32_t lds_bytes, int32_t microseconds, void *stream) {
    if (blocks <= 0 || threads <= 0 || threads > 1024 || lds_bytes < 0 || lds_bytes > 160 * 1024 || microseconds < 0 || microseconds > 2000000) {
        swd::set_error("swd_diag_occupy: blocks > 0, 1..1024 threads, 0..163840 bytes of LDS, at most 2 000 000 us");
        return -1;
    }
    SWD_HIP(hipSetDevice(device));
    SWD_HIP(hipFuncSetAttribute((const void *)swd::occupy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(swd::occupy_kernel, dim3((unsigned)blocks), dim3((unsigned)threads), (size_t)lds_bytes, (hipStream_t)stream,
                       (long long)microseconds * 100, (uint32_t *)nullptr);
    SWD_HIP(hipGetLastError());
    return 0;
}
