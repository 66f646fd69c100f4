// Circuit sampler (include/swd.h: swd_circuit_sampler_*): Pauli-frame simulation of a memory circuit's op list, the forward
// direction of what circuit.dem_from_ops analyses backwards.  slidingwindowdecoder_amd/frames.py states the rule and restates it in
// numpy (simulate_frames_host); this file executes that table bit for bit.
//
// frame_kernel: one wave = one workgroup = 64 shots, lane = shot.  A qubit's frame is two 64-bit shot masks (x, z) in LDS, so a
// Clifford op is an XOR of masks.  The op list is walked in order by the whole wave (the program is read with a wave-uniform index);
// every lane applies the wave-uniform frame update itself: all lanes read one address and write one value, and a lane's own program
// order is all the ordering the LDS needs, so there is no barrier after the first.  A noise op is drawn with lane = shot -- one
// Philox call serves four noise slots, 128 randomisation slots -- and __ballot turns the per-shot hits into masks; a zero ballot,
// nearly always at p ~ 1e-3, skips the frame update and the 64-bit division that picks the Pauli.  Shots past B in the last wave
// stay in the control flow (every ballot is executed by the whole wave); they never reach an output: emit_kernel writes the shots
// < B only.  A measurement's mask goes to rec[wave][i] in global memory (lane 0, an ordinary vector store).
// emit_kernel: one workgroup per wave of 64 shots; it reads the wave's masks once, forms detectors and observables over the CSR
// measurement map as XORs of whole masks, stages masks in LDS and cuts them into shots (bytes, or bit i & 7 of byte i >> 3) with
// a shot's stores contiguous.
#include <string.h>

#include <map>
#include <mutex>

#include "swd_host.h"

using namespace swd;

namespace {

// circuit.py's op codes (DETECTOR = 10 and OBSERVABLE = 11 are not executed: they are the measurement map)
enum { OP_R = 0, OP_RX = 1, OP_H = 2, OP_CX = 3, OP_M = 4, OP_MR = 5, OP_MRX = 6, OP_XERR = 7, OP_DEP1 = 8, OP_DEP2 = 9, OP_MX = 12, OP_ZERR = 13 };

constexpr int kFrameLdsBytes = 64 * 1024;          // the wave's slice of LDS: 16 bytes per qubit
constexpr int kMaxQubits = kFrameLdsBytes / 16;    // 4096
constexpr int kMaxSlotCalls = 1 << 30;             // slot / 4 is counter word 2

typedef unsigned long long u64;

struct CircuitSampler {
    int device = 0, num_ops = 0, num_qubits = 0, num_meas = 0, num_det = 0, num_obs = 0, num_noise = 0, num_rand = 0, randomize = 1;
    DevBuf buf;                       // prog[num_ops] uint4 | ptr[num_det + num_obs + 1] u32 | idx[E] u32
    const uint4 *d_prog = nullptr;    // { kind | qa << 8, qb (measurements: the record index), threshold, noise or randomisation slot }
    const uint32_t *d_ptr = nullptr, *d_idx = nullptr;
    std::mutex mu;
    std::map<void *, DevBuf> masks;   // per stream: rec[ceil(B / 64)][num_meas] u64, the record as shot masks between the two kernels
    DevBuf det, obs, meas;            // staging for the host-pointer entry points
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

__device__ __forceinline__ uint32_t word_of(const uint32_t (&w)[4], uint32_t k) {
    return k == 0 ? w[0] : k == 1 ? w[1] : k == 2 ? w[2] : w[3];
}

// x part / z part of Pauli 0..3 = I, X, Y, Z
__device__ __forceinline__ bool pauli_x(uint32_t p) { return p == 1u || p == 2u; }
__device__ __forceinline__ bool pauli_z(uint32_t p) { return p >= 2u; }

__global__ void __launch_bounds__(64) frame_kernel(int num_ops, int num_qubits, int num_meas, const uint4 *__restrict__ prog,
                                                   int randomize, uint64_t seed, uint64_t first_shot, u64 *__restrict__ rec) {
    extern __shared__ __attribute__((aligned(16))) u64 fr[]; // [num_qubits][2]: x mask, z mask
    const int lane = threadIdx.x;
    const uint64_t shot = first_shot + (uint64_t)blockIdx.x * 64u + (uint64_t)lane;
    const uint32_t s0 = (uint32_t)shot, s1 = (uint32_t)(shot >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int i = lane; i < 2 * num_qubits; i += 64) fr[i] = 0;
    __syncthreads();
    u64 *out = rec + (size_t)blockIdx.x * (size_t)num_meas;
    uint32_t nw[4] = {0, 0, 0, 0}, rw[4] = {0, 0, 0, 0};
    uint32_t ncall = 0xFFFFFFFFu, rcall = 0xFFFFFFFFu; // the Philox call the words belong to
    for (int i = 0; i < num_ops; ++i) {
        const uint4 op = prog[i];
        const uint32_t kind = op.x & 0xFFu, a = op.x >> 8, b = op.y, thr = op.z, slot = op.w;
        u64 *fa = fr + 2 * a;
        if (kind == OP_CX) {
            u64 *fb = fr + 2 * b;
            const u64 xa = fa[0], zb = fb[1];
            fb[0] ^= xa;
            fa[1] ^= zb;
        } else if (kind == OP_H) {
            const u64 x = fa[0], z = fa[1];
            fa[0] = z; fa[1] = x;
        } else if (kind == OP_XERR || kind == OP_ZERR || kind == OP_DEP1 || kind == OP_DEP2) {
            if ((slot >> 2) != ncall) {
                ncall = slot >> 2;
                philox4x32_10(s0, s1, ncall, 2u, k0, k1, nw);
            }
            const uint32_t u = word_of(nw, slot & 3u);
            const bool hit = u < thr;
            const u64 m = __ballot(hit);
            if (m != 0) {
                if (kind == OP_XERR) fa[0] ^= m;
                else if (kind == OP_ZERR) fa[1] ^= m;
                else if (kind == OP_DEP1) {
                    const uint32_t p = hit ? 1u + (uint32_t)(((uint64_t)u * 3u) / thr) : 0u;
                    const u64 mx = __ballot(pauli_x(p)), mz = __ballot(pauli_z(p));
                    fa[0] ^= mx; fa[1] ^= mz;
                } else {
                    u64 *fb = fr + 2 * b;
                    const uint32_t k = hit ? 1u + (uint32_t)(((uint64_t)u * 15u) / thr) : 0u, pa = k >> 2, pb = k & 3u;
                    const u64 ax = __ballot(pauli_x(pa)), az = __ballot(pauli_z(pa)), bx = __ballot(pauli_x(pb)), bz = __ballot(pauli_z(pb));
                    fa[0] ^= ax; fa[1] ^= az; fb[0] ^= bx; fb[1] ^= bz;
                }
            }
        } else { // R, RX, M, MR, MX, MRX: the ops that draw a randomisation bit
            u64 rnd = 0;
            if (randomize) {
                if ((slot >> 7) != rcall) {
                    rcall = slot >> 7;
                    philox4x32_10(s0, s1, rcall, 3u, k0, k1, rw);
                }
                rnd = __ballot((word_of(rw, (slot >> 5) & 3u) >> (slot & 31u)) & 1u);
            }
            if (kind == OP_R) { fa[0] = 0; fa[1] = rnd; }
            else if (kind == OP_RX) { fa[1] = 0; fa[0] = rnd; }
            else {
                const bool zb = kind == OP_MX || kind == OP_MRX; // measured in the X basis: the record takes the z bit
                const u64 v = fa[zb ? 1 : 0];
                if (lane == 0) out[b] = v;
                if (kind == OP_M) fa[1] = rnd;
                else if (kind == OP_MR) { fa[0] = 0; fa[1] = rnd; }
                else if (kind == OP_MX) fa[0] = rnd;
                else { fa[1] = 0; fa[0] = rnd; }
            }
        }
    }
}

constexpr int kEmitTile = 1024; // masks an emit workgroup stages in LDS at a time (8 KB; a multiple of 8: a tile is whole packed bytes)

// rows [0, n) of 64-shot masks -> out[s][0 .. n) for the shots s < nshots of the workgroup's wave of shots: bytes, or packed bits.
// The masks are made once (mask_of(i), any thread) and staged in LDS; each of the four waves then writes whole shots, lanes along
// the row, so the stores of a shot are contiguous.  Every bound of the loops around the barriers is uniform over the workgroup.
template <class F>
__device__ __forceinline__ void emit_rows(F mask_of, int n, uint8_t *out, int64_t stride, int nshots, int packed, u64 *tile) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int base = 0; base < n; base += kEmitTile) {
        const int cnt = min(kEmitTile, n - base);
        __syncthreads();
        for (int j = tid; j < cnt; j += 256) tile[j] = mask_of(base + j);
        __syncthreads();
        for (int s = wave; s < nshots; s += 4) {
            uint8_t *o = out + (int64_t)s * stride;
            if (!packed) {
                for (int j = lane; j < cnt; j += 64) o[base + j] = (uint8_t)((tile[j] >> s) & 1u);
            } else {
                for (int jb = lane; jb < (cnt + 7) / 8; jb += 64) {
                    uint32_t v = 0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int j = 8 * jb + k;
                        if (j < cnt) v |= (uint32_t)((tile[j] >> s) & 1u) << k;
                    }
                    o[base / 8 + jb] = (uint8_t)v;
                }
            }
        }
    }
}

// one workgroup per wave of 64 shots: the record's masks are read once, detectors and observables are formed as XORs of whole
// masks (64 shots per row of the map at a time) and only then cut into shots
__global__ void __launch_bounds__(256) emit_kernel(int B, int num_meas, int num_det, int num_obs, const u64 *__restrict__ rec,
                                                   const uint32_t *__restrict__ ptr, const uint32_t *__restrict__ idx, uint8_t *det,
                                                   int64_t det_stride, uint32_t *obs_flips, uint8_t *meas, int64_t meas_stride, int packed) {
    __shared__ u64 tile[kEmitTile];
    __shared__ u64 obsm[32];
    const int tid = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * 64;
    const int nshots = (int)min((int64_t)64, (int64_t)B - b0);
    const u64 *rm = rec + (size_t)blockIdx.x * (size_t)num_meas;
    auto row_mask = [&](int r) {
        u64 acc = 0;
        for (uint32_t e = ptr[r]; e < ptr[r + 1]; ++e) acc ^= rm[idx[e]];
        return acc;
    };
    if (meas) emit_rows([&](int i) { return rm[i]; }, num_meas, meas + b0 * meas_stride, meas_stride, nshots, packed, tile);
    if (det) emit_rows(row_mask, num_det, det + b0 * det_stride, det_stride, nshots, 0, tile);
    if (obs_flips) { // num_obs <= 32 here
        if (tid < num_obs) obsm[tid] = row_mask(num_det + tid);
        __syncthreads();
        if (tid < nshots) {
            uint32_t f = 0;
            for (int k = 0; k < num_obs; ++k) f |= (uint32_t)((obsm[k] >> tid) & 1u) << k;
            obs_flips[b0 + tid] = f;
        }
    }
}

bool map_ok(const swd_graph_desc *g, int num_meas, const char *what) {
    if (!g) return true;
    if (g->m < 0 || g->n != num_meas || !g->row_ptr || (g->nnz > 0 && !g->col_idx) || g->row_ptr[0] != 0) {
        set_error(SWD_ERR_VALUE, "circuit sampler: the %s map must be a CSR over the %d measurements", what, num_meas);
        return false;
    }
    for (int r = 0; r < g->m; ++r) {
        if (g->row_ptr[r] > g->row_ptr[r + 1]) { set_error(SWD_ERR_VALUE, "circuit sampler: %s map: row_ptr is not monotone", what); return false; }
        for (int e = g->row_ptr[r]; e < g->row_ptr[r + 1]; ++e)
            if (g->col_idx[e] < 0 || g->col_idx[e] >= num_meas) {
                set_error(SWD_ERR_VALUE, "circuit sampler: %s %d reads measurement %d, the record has %d", what, r, g->col_idx[e], num_meas);
                return false;
            }
    }
    return true;
}

// the two launches of a call; meas_row = bytes of a shot's record in the form asked for
int circuit_launch(CircuitSampler *s, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *det, int64_t det_stride, uint32_t *obs_flips,
                   uint8_t *meas, int64_t meas_stride, int packed, void *stream) {
    if (B <= 0) return 0;
    const int64_t meas_row = packed ? (s->num_meas + 7) / 8 : s->num_meas;
    det_stride = det_stride ? det_stride : s->num_det;
    meas_stride = meas_stride ? meas_stride : meas_row;
    if ((det && det_stride < s->num_det) || (meas && meas_stride < meas_row)) {
        set_error(SWD_ERR_VALUE, "circuit sampler: a stride is shorter than a shot's row");
        return -1;
    }
    if (obs_flips && s->num_obs > 32) {
        set_error(SWD_ERR_CAPACITY, "circuit sampler: observable masks carry at most 32 observables, the circuit has %d", s->num_obs);
        return -1;
    }
    SWD_HIP(hipSetDevice(s->device));
    const int64_t waves = ((int64_t)B + 63) / 64;
    u64 *rec;
    {
        std::lock_guard<std::mutex> lock(s->mu);
        DevBuf &m = s->masks[stream]; // calls on one stream are ordered; calls on two streams get a buffer each
        if (m.reserve((size_t)waves * (size_t)std::max(s->num_meas, 1) * sizeof(u64))) return -1;
        rec = m.as<u64>();
    }
    hipLaunchKernelGGL(frame_kernel, dim3((unsigned)waves), dim3(64), (size_t)std::max(s->num_qubits, 1) * 16, (hipStream_t)stream, s->num_ops,
                       s->num_qubits, s->num_meas, s->d_prog, s->randomize, seed, first_shot, rec);
    SWD_HIP(hipGetLastError());
    if (det || obs_flips || meas) {
        hipLaunchKernelGGL(emit_kernel, dim3((unsigned)waves), dim3(256), 0, (hipStream_t)stream, (int)B, s->num_meas, s->num_det, s->num_obs, rec,
                           s->d_ptr, s->d_idx, det, det_stride, obs_flips, meas, meas_stride, packed);
        SWD_HIP(hipGetLastError());
    }
    return 0;
}

} // namespace

extern "C" swd_circuit_sampler *swd_circuit_sampler_create(int32_t num_ops, const int32_t *kind, const int32_t *qa, const int32_t *qb,
                                                           const uint32_t *thr, const int32_t *meas, const int32_t *noise_slot,
                                                           const int32_t *rand_slot, int32_t num_qubits, int32_t num_meas,
                                                           const swd_graph_desc *det_map, const swd_graph_desc *obs_map, int32_t randomize,
                                                           int device) {
    if (num_ops < 0 || (num_ops > 0 && (!kind || !qa || !qb || !thr || !meas || !noise_slot || !rand_slot))) { set_error("null argument"); return nullptr; }
    if (num_qubits < 0 || num_meas < 0) { set_error(SWD_ERR_VALUE, "circuit sampler: %d qubits, %d measurements", num_qubits, num_meas); return nullptr; }
    if (num_qubits > kMaxQubits) {
        set_error(SWD_ERR_CAPACITY, "circuit sampler: %d qubits; a wave's frame of 16 bytes per qubit fits %d in its %d KB of LDS", num_qubits,
                  kMaxQubits, kFrameLdsBytes / 1024);
        return nullptr;
    }
    if (!map_ok(det_map, num_meas, "detector") || !map_ok(obs_map, num_meas, "observable")) return nullptr;
    std::vector<uint4> prog((size_t)std::max(num_ops, 1));
    std::vector<uint8_t> written((size_t)num_meas, 0);
    int nn = 0, nr = 0;
    for (int i = 0; i < num_ops; ++i) {
        const int k = kind[i];
        const bool two = k == OP_CX || k == OP_DEP2, noise = k == OP_XERR || k == OP_ZERR || k == OP_DEP1 || k == OP_DEP2;
        const bool measure = k == OP_M || k == OP_MR || k == OP_MX || k == OP_MRX, random = measure || k == OP_R || k == OP_RX;
        if (!(two || noise || random || k == OP_H)) { set_error(SWD_ERR_VALUE, "circuit sampler: op %d has the code %d, which is not executable", i, k); return nullptr; }
        if (qa[i] < 0 || qa[i] >= num_qubits || (two && (qb[i] < 0 || qb[i] >= num_qubits || qb[i] == qa[i]))) {
            set_error(SWD_ERR_VALUE, "circuit sampler: op %d: qubits out of range (%d qubits)", i, num_qubits);
            return nullptr;
        }
        if (measure && (meas[i] < 0 || meas[i] >= num_meas || written[meas[i]]++)) {
            set_error(SWD_ERR_VALUE, "circuit sampler: op %d: measurement index %d out of range or used twice (%d measurements)", i, meas[i], num_meas);
            return nullptr;
        }
        // slots are numbered in list order: the kernel keeps the words of one Philox call and looks the call up by slot
        if ((noise && noise_slot[i] != nn) || (random && rand_slot[i] != nr)) {
            set_error(SWD_ERR_VALUE, "circuit sampler: op %d: slots must be numbered 0, 1, ... in list order", i);
            return nullptr;
        }
        const uint32_t slot = noise ? (uint32_t)nn++ : random ? (uint32_t)nr++ : 0u;
        prog[i] = make_uint4((uint32_t)k | ((uint32_t)qa[i] << 8), measure ? (uint32_t)meas[i] : two ? (uint32_t)qb[i] : 0u, noise ? thr[i] : 0u, slot);
    }
    for (int m = 0; m < num_meas; ++m)
        if (!written[m]) { set_error(SWD_ERR_VALUE, "circuit sampler: measurement %d is never written", m); return nullptr; }
    if ((nn >> 2) >= kMaxSlotCalls) { set_error(SWD_ERR_CAPACITY, "circuit sampler: %d noise slots do not fit the generator's counter", nn); return nullptr; }
    {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error(SWD_ERR_DEVICE, "no HIP device available: the MI355X decoder has no CPU fallback"); return nullptr; }
        if (device < 0 || device >= ndev) { set_error(SWD_ERR_DEVICE, "device %d out of range (%d devices)", device, ndev); return nullptr; }
    }
    const int nd = det_map ? det_map->m : 0, no = obs_map ? obs_map->m : 0;
    std::vector<uint32_t> ptr{0}, idx;
    for (const swd_graph_desc *g : {det_map, obs_map})
        for (int r = 0; g && r < g->m; ++r) {
            for (int e = g->row_ptr[r]; e < g->row_ptr[r + 1]; ++e) idx.push_back((uint32_t)g->col_idx[e]);
            ptr.push_back((uint32_t)idx.size());
        }
    CircuitSampler *s = new CircuitSampler();
    s->device = device; s->num_ops = num_ops; s->num_qubits = num_qubits; s->num_meas = num_meas; s->num_det = nd; s->num_obs = no;
    s->num_noise = nn; s->num_rand = nr; s->randomize = randomize ? 1 : 0;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_ptr = al(prog.size() * sizeof(uint4)), o_idx = al(o_ptr + ptr.size() * 4), total = al(o_idx + idx.size() * 4 + 4);
    std::vector<char> h(total, 0);
    memcpy(&h[0], prog.data(), prog.size() * sizeof(uint4)); memcpy(&h[o_ptr], ptr.data(), ptr.size() * 4);
    if (!idx.empty()) memcpy(&h[o_idx], idx.data(), idx.size() * 4);
    if (hipSetDevice(device) != hipSuccess || s->buf.reserve(total) || hipMemcpy(s->buf.p, h.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        set_error(SWD_ERR_DEVICE, "circuit sampler: device allocation failed on device %d", device);
        delete s;
        return nullptr;
    }
    char *b = (char *)s->buf.p;
    s->d_prog = (const uint4 *)b; s->d_ptr = (const uint32_t *)(b + o_ptr); s->d_idx = (const uint32_t *)(b + o_idx);
    return (swd_circuit_sampler *)s;
}

extern "C" void swd_circuit_sampler_destroy(swd_circuit_sampler *h) { delete (CircuitSampler *)h; }

extern "C" int swd_circuit_sampler_info(const swd_circuit_sampler *h, int64_t *info) {
    CircuitSampler *s = (CircuitSampler *)h;
    if (!s || !info) { set_error("null argument"); return -1; }
    std::lock_guard<std::mutex> lock(s->mu);
    size_t bytes = s->buf.cap + s->det.cap + s->obs.cap + s->meas.cap;
    for (auto &kv : s->masks) bytes += kv.second.cap;
    const int64_t v[8] = {s->num_qubits, s->num_meas, s->num_det, s->num_obs, s->num_noise, s->num_rand, (int64_t)bytes, kMaxQubits};
    memcpy(info, v, sizeof(v));
    return 0;
}

extern "C" int swd_circuit_sampler_measure_dev(swd_circuit_sampler *h, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *meas,
                                               int64_t meas_stride, int32_t packed, void *stream) {
    CircuitSampler *s = (CircuitSampler *)h;
    if (!s || !meas) { set_error("null argument"); return -1; }
    return circuit_launch(s, B, seed, first_shot, nullptr, 0, nullptr, meas, meas_stride, packed ? 1 : 0, stream);
}

extern "C" int swd_circuit_sampler_sample_dev(swd_circuit_sampler *h, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *det,
                                              int64_t det_stride, uint32_t *obs_flips, uint8_t *meas, int64_t meas_stride, void *stream) {
    CircuitSampler *s = (CircuitSampler *)h;
    if (!s || !det) { set_error("null argument"); return -1; }
    return circuit_launch(s, B, seed, first_shot, det, det_stride, obs_flips, meas, meas_stride, 0, stream);
}

extern "C" int swd_circuit_sampler_measure(swd_circuit_sampler *h, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *meas, int32_t packed) {
    CircuitSampler *s = (CircuitSampler *)h;
    if (!s || !meas) { set_error("null argument"); return -1; }
    if (B <= 0) return 0;
    const size_t row = packed ? ((size_t)s->num_meas + 7) / 8 : (size_t)s->num_meas;
    SWD_HIP(hipSetDevice(s->device));
    if (s->meas.reserve((size_t)B * row + 1)) return -1;
    if (circuit_launch(s, B, seed, first_shot, nullptr, 0, nullptr, s->meas.as<uint8_t>(), 0, packed ? 1 : 0, nullptr)) return -1;
    SWD_HIP(hipDeviceSynchronize());
    if (row) SWD_HIP(hipMemcpy(meas, s->meas.p, (size_t)B * row, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int swd_circuit_sampler_sample(swd_circuit_sampler *h, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *det,
                                          uint32_t *obs_flips, uint8_t *meas) {
    CircuitSampler *s = (CircuitSampler *)h;
    if (!s || !det) { set_error("null argument"); return -1; }
    if (B <= 0) return 0;
    SWD_HIP(hipSetDevice(s->device));
    if (s->det.reserve((size_t)B * s->num_det + 1) || s->obs.reserve((size_t)B * 4)) return -1;
    if (meas && s->meas.reserve((size_t)B * s->num_meas + 1)) return -1;
    if (circuit_launch(s, B, seed, first_shot, s->det.as<uint8_t>(), 0, obs_flips ? s->obs.as<uint32_t>() : nullptr,
                       meas ? s->meas.as<uint8_t>() : nullptr, 0, 0, nullptr)) return -1;
    SWD_HIP(hipDeviceSynchronize());
    if (s->num_det) SWD_HIP(hipMemcpy(det, s->det.p, (size_t)B * s->num_det, hipMemcpyDeviceToHost));
    if (obs_flips) SWD_HIP(hipMemcpy(obs_flips, s->obs.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (meas && s->num_meas) SWD_HIP(hipMemcpy(meas, s->meas.p, (size_t)B * s->num_meas, hipMemcpyDeviceToHost));
    return 0;
}
