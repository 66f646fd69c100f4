// Host-side helpers shared by the C-ABI translation units: error reporting, device buffers,
// and the CSR -> device-graph builder.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "swd.h"
#include "swd_env.h"
#include "swd_graph.h"

namespace swd {

// The calling thread's failure: a message and, beside it, its class (include/swd.h, swd_error_class).  Without a class: SWD_ERR_FAILED.
// What reacts to a failure -- a create that falls back to a general form, the Python surface choosing an exception -- reads
// last_error_class(), never the text.
void set_error(const char *fmt, ...);
void set_error(swd_error_class cls, const char *fmt, ...);
const char *last_error();
swd_error_class last_error_class();

#define SWD_HIP(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            swd::set_error(SWD_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                           __LINE__);                                                         \
            return -1;                                                                        \
        }                                                                                     \
    } while (0)

// Device buffer that only grows.  Growing never calls hipFree on the launch path: hipFree synchronises the whole device (and the old
// allocation may still be read by a launch in flight on another stream), so the outgrown allocation is retired and released with the
// buffer.  Growth is geometric (at least 1.5x), which bounds the retired bytes by twice the final size.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    std::vector<void *> retired;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
        for (void *q : retired) (void)hipFree(q);
    }
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        const size_t want = std::max(bytes, cap + cap / 2);
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, want);
        size_t got = want;
        if (e != hipSuccess && want > bytes) { (void)hipGetLastError(); e = hipMalloc(&q, bytes); got = bytes; }
        if (e != hipSuccess) {
            swd::set_error(SWD_ERR_DEVICE, "hipMalloc(%zu bytes) failed: %s (%s:%d)", bytes, hipGetErrorString(e), __FILE__, __LINE__);
            return -1;
        }
        if (p) retired.push_back(p);
        p = q; cap = got;
        return 0;
    }
    template <class T> T *as() { return (T *)p; }
};

// Page-locked host staging area: one asynchronous copy in and one out per host-buffer call instead of a
// synchronous pageable copy per array (a one-syndrome decode() spent most of its time in those).
constexpr size_t SWD_STAGE_MAX = 4u << 20; // host-buffer calls moving more than this copy array by array instead
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        SWD_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        cap = bytes;
        return 0;
    }
};

// Host copy of the device graph arrays + the device allocation holding them.
struct Graph {
    int m = 0, n = 0, E = 0, K = 0, D = 0, rank = 0, wm = 0;
    int S = 0;                   // message slots: E + pad cells (swd_graph.h)
    std::vector<uint8_t> epos;   // [E] position of CSR edge e inside its check's row
    std::vector<uint16_t> dpad;  // [K] pad cells behind diagonal j
    long cost_natural = 0, cost = 0; // layout_cost() of the natural layout and of this one
    std::vector<uint16_t> jptr, row_col, perm, iperm, vn_row;
    std::vector<uint8_t> row_deg, col_deg;
    std::vector<uint32_t> vn_edge, vn_edge_s;
    std::vector<uint16_t> vperm;
    std::vector<double> llr;
    // depth order of the nodes (swd_graph.h): exact degree descending, stable in the column index; the tables the device gets
    std::vector<uint16_t> vdord, vdpos; // [n] i-th listed node; listed position of column v
    std::vector<uint32_t> vn_edge_d;    // [D*n]
    std::vector<double> llr_d;          // [n]
    // original CSR/CSC kept for host-side use (rank, OSD-CS setup)
    std::vector<int32_t> row_ptr, col_idx, col_ptr, row_idx;
    DevBuf dev;
    SwdGraphDev d{};
    // side list of the heavy columns build() was given (swd_graph.h, SwdHeavyDev); empty otherwise
    std::vector<int32_t> hv_id, hv_deg, hv_ptr;
    std::vector<uint32_t> hv_edge;
    SwdHeavyDev hv{};

    // validates, fills host arrays (natural layout), computes rank.  `heavy` (ascending column ids, at most SWD_MAX_HEAVY): these
    // columns may have any weight; they leave the ELL tables (col_deg 0) for the side list
    int build(const swd_graph_desc *g, const std::vector<int32_t> *heavy = nullptr);
    // bank-conflict-aware layout with up to `pads` pad cells; build() first, upload() after.  listed: thread t serves the nodes at
    // listed positions t, t + NT, ... of the depth order (profiled kernels) instead of columns t, t + NT, ...
    void optimize_layout(int pads, bool listed = false);
    long layout_cost(long *loads = nullptr, long *stores = nullptr, bool listed = false) const;
    void fill_tables();
    void fill_listed();
    void fill_depth();
    // every listed node i * nt .. (i + 1) * nt - 1 that exists has degree <= depth[i], for each of the vf cache rows
    bool fits_depth(const int *depth, int vf, int nt) const;
    // cache image of the graph for the tuned osd_window kernel <nt, vf, dm, kg> (swd_graph.h, SwdGraphDev::img_*): after the layout is
    // final, before upload().  depth (nullable): the plan's depth profile -- both node parts are then built, the uniform one alone otherwise
    std::vector<uint32_t> img_vn, img_vn_d, img_cn;
    void fill_image(int nt, int vf, int dm, int kg, const int *depth);
    int upload();                          // hipMalloc + copy, fills d
};

// SWD_NATURAL_LAYOUT in the environment (swd_env.h): plans keep the natural layout of their graphs
bool natural_layout_requested();

int gf2_rank(int m, int n, const std::vector<int32_t> &row_ptr, const std::vector<int32_t> &col_idx);

// The row check of every graph ingest, on a copied CSR whose row_ptr spans col_idx: row_ptr monotone, every row sorted in place
// (columns ascending), column indices in range and distinct.  0, or -1 with the message set.
int csr_check_rows(int m, int n, const std::vector<int32_t> &row_ptr, std::vector<int32_t> &col_idx);

// A checked CSR with its transpose: CSC (rows ascending inside a column), c2r = CSC position -> CSR edge, r2c = its inverse
// (on request), llr[v] = log((1 - p[v]) / p[v]) (osd_window.pyx:113).
struct CsrHost {
    std::vector<int32_t> row_ptr, col_idx, col_ptr, row_idx, c2r, r2c;
    std::vector<double> llr;
};
void csr_transpose(int m, int n, const double *channel_probs, bool want_r2c, CsrHost &h);

} // namespace swd
