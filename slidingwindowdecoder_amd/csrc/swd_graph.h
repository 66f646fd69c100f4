// Device-side layout of one window Tanner graph (replaces the doubly-linked mod2sparse
// nodes of /root/reference/src/include/mod2sparse.h:46-82 on the hot path).
//
// HBM (read-only, shared by every shot; ~70 KB for the [[144,12,12]] (3,1) window so it stays
// L2-resident):
//   * checks are renumbered by DEGREE-DESCENDING order: "lane" l handles original check
//     perm[l].  Edge slots use the jagged-diagonal numbering slot(j, l) = jptr[j] + l
//     (j = position inside the row), so for a fixed j consecutive lanes touch consecutive
//     8-byte LDS words (conflict-free ds_read_b64 / ds_write_b64) and the slot count is
//     nnz plus a few pad cells -- no ELL padding, which is what lets the fp64 messages of a
//     5976-edge window fit the LDS budget;
//   * which edge of a check sits at which position j, which of several checks of one degree takes
//     which lane, and pad cells between consecutive diagonals (jptr[j + 1] - jptr[j] >= checks of
//     degree > j) are free -- no result depends on them -- and a plan's graphs use them so that the
//     variable-node pass, which gathers one cell per lane, spreads over the LDS banks
//     (swd_graph.hip, Graph::optimize_layout); the natural layout is ascending columns, lanes
//     stable in the check index, no pads;
//   * row_col[slot]  = column of that edge (coalesced for a fixed j);
//   * vn_edge[k*n+v] = k-th edge of column v in row-ascending order (the order the
//     reference's variable-node update sums in, osd_window.pyx:446-471), packed
//     slot | lane << 16 | j << 26; k-major so consecutive v are coalesced;
//   * vn_row[k*n+v]  = original row index of that edge (OSD works in original row order).
#pragma once
#include <stdint.h>

#define SWD_MAX_ROW_DEG 64   // livemask is one 64-bit word per check
#define SWD_MAX_COL_DEG 16
#define SWD_MAX_M 1024       // 10-bit lane field in vn_edge
#define SWD_MAX_E 65535      // 16-bit slot field
#define SWD_PAD_EDGE 0xFFFFFFFFu

struct SwdGraphDev {
    int32_t m, n, E, K, D;   // E = message slots (edges + pad cells), K = max row degree, D = max column degree
    int32_t new_n, rank, wm; // wm = ceil(m / 64)
    int32_t nnz, pad_;       // edges
    const uint16_t *jptr;    // [K+1]
    const uint16_t *row_col; // [E] (pad slots: 0)
    const uint8_t *row_deg;  // [m] by lane
    const uint16_t *perm;    // [m] lane -> original check
    const uint16_t *iperm;   // [m] original check -> lane
    const uint32_t *vn_edge; // [D*n]
    const uint16_t *vn_row;  // [D*n]
    const uint8_t *col_deg;  // [n]
    const double *llr;       // [n]
    // The full-graph variable-node pass by DEPTH (swd_variants.h, SWD_DEPTH_PROFILES): the nodes listed by exact degree descending
    // (stable in the column index), NT per cache row, so that row i of a profiled kernel walks depth[i] positions and no more --
    // vdord[i] = the i-th listed node, vn_edge_d / llr_d = vn_edge / llr in that order (coalesced, no dependent load).
    // (The host keeps the round-5 order in tiers of two, Graph::vperm / vn_edge_s, for swd_graph_layout only.)
    const uint16_t *vdord;     // [n]
    const uint32_t *vn_edge_d; // [D*n]
    const double *llr_d;       // [n]
    // Cache image (graphs of plans that launch the tuned osd_window kernels of up to SWD_TUNED_NT threads; null otherwise): the full
    // graph's register caches as those kernels hold them after their set-up, packed once on the host (swd_graph.hip, Graph::fill_image;
    // the word order is SwdCacheImg's, swd_osdw_kernel.h).  In 16-byte chunks, chunk-major and role-minor: chunk q of thread role r
    // is words (q * nt + r) * 4 .. + 3, so a wave loads a chunk from consecutive addresses.
    const uint32_t *img_vn;    // node part by role vtid, uniform depth: columns vtid + i * nt
    const uint32_t *img_vn_d;  // ... of the plan's depth profile: listed nodes vtid + i * nt (null without a profile)
    const uint32_t *img_cn;    // check part by role ctid: the check of lane ctid
};

// Heavy columns (weight above what the ELL tables hold; asked for by swd_bp4_create only): a side list beside the tables above,
// where such a column has col_deg 0.  Its edges are ordinary message slots of their checks.
#define SWD_MAX_HEAVY 8
struct SwdHeavyDev {
    int32_t count, edges;    // columns listed, sum of their degrees
    const int32_t *id;       // [count] column
    const int32_t *deg;      // [count] its weight in this matrix (may be 0: heavy in the other matrix of a pair only)
    const int32_t *ptr;      // [count + 1] start of its edge words
    const uint32_t *edge;    // [edges] edge words (slot | lane << 16 | j << 26) in row-ascending order, the order the reference walks a column
};

__host__ __device__ inline uint32_t swd_edge_slot(uint32_t e) { return e & 0xFFFFu; }
__host__ __device__ inline uint32_t swd_edge_lane(uint32_t e) { return (e >> 16) & 0x3FFu; }
__host__ __device__ inline uint32_t swd_edge_j(uint32_t e) { return e >> 26; }
