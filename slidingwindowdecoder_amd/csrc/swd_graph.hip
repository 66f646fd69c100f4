// CSR -> device Tanner-graph layout (see swd_graph.h) and host-side GF(2) rank.
// Replaces numpy2mod2sparse / spmatrix2mod2sparse (/root/reference/src/mod2sparse.pyx:5-31) and
// mod2sparse_rank (/root/reference/src/include/mod2sparse_extra.cpp:32-76, value only).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

#include "swd_host.h"

namespace swd {

static thread_local std::string g_err;
static thread_local swd_error_class g_err_class = SWD_ERR_FAILED;

static void set_error_v(swd_error_class cls, const char *fmt, va_list ap) {
    char buf[1024];
    vsnprintf(buf, sizeof buf, fmt, ap);
    g_err = buf;
    g_err_class = cls;
}

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    set_error_v(SWD_ERR_FAILED, fmt, ap);
    va_end(ap);
}

void set_error(swd_error_class cls, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    set_error_v(cls, fmt, ap);
    va_end(ap);
}

const char *last_error() { return g_err.c_str(); }
swd_error_class last_error_class() { return g_err_class; }

int gf2_rank(int m, int n, const std::vector<int32_t> &row_ptr, const std::vector<int32_t> &col_idx) {
    const int W = (n + 63) / 64;
    std::vector<uint64_t> rows((size_t)m * W, 0);
    for (int r = 0; r < m; ++r)
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) rows[(size_t)r * W + (col_idx[e] >> 6)] ^= 1ull << (col_idx[e] & 63);
    int rank = 0;
    std::vector<char> used(m, 0);
    for (int c = 0; c < n && rank < m; ++c) {
        int pr = -1;
        for (int r = 0; r < m; ++r)
            if (!used[r] && ((rows[(size_t)r * W + (c >> 6)] >> (c & 63)) & 1)) { pr = r; break; }
        if (pr < 0) continue;
        used[pr] = 1;
        ++rank;
        for (int r = 0; r < m; ++r)
            if (!used[r] && ((rows[(size_t)r * W + (c >> 6)] >> (c & 63)) & 1))
                for (int w = c >> 6; w < W; ++w) rows[(size_t)r * W + w] ^= rows[(size_t)pr * W + w];
    }
    return rank;
}

int csr_check_rows(int m, int n, const std::vector<int32_t> &row_ptr, std::vector<int32_t> &col_idx) {
    // (all of row_ptr first: with its ends pinned by the caller, monotone means every row lies inside col_idx)
    for (int r = 0; r < m; ++r)
        if (row_ptr[r + 1] < row_ptr[r]) { set_error("row_ptr not monotone at row %d", r); return -1; }
    for (int r = 0; r < m; ++r) {
        std::sort(col_idx.begin() + row_ptr[r], col_idx.begin() + row_ptr[r + 1]);
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
            if (col_idx[e] < 0 || col_idx[e] >= n) { set_error("column index out of range in row %d", r); return -1; }
            if (e > row_ptr[r] && col_idx[e] == col_idx[e - 1]) { set_error("duplicate entry in row %d", r); return -1; }
        }
    }
    return 0;
}

void csr_transpose(int m, int n, const double *channel_probs, bool want_r2c, CsrHost &h) {
    const int E = (int)h.col_idx.size();
    h.col_ptr.assign(n + 1, 0);
    h.row_idx.resize(E);
    h.c2r.resize(E);
    std::vector<int32_t> fill(n, 0);
    for (int e = 0; e < E; ++e) h.col_ptr[h.col_idx[e] + 1]++;
    for (int v = 0; v < n; ++v) h.col_ptr[v + 1] += h.col_ptr[v];
    for (int c = 0; c < m; ++c)
        for (int e = h.row_ptr[c]; e < h.row_ptr[c + 1]; ++e) { const int v = h.col_idx[e], k = h.col_ptr[v] + fill[v]++; h.row_idx[k] = c; h.c2r[k] = e; }
    if (want_r2c) {
        h.r2c.resize(E);
        for (int k = 0; k < E; ++k) h.r2c[h.c2r[k]] = k;
    }
    h.llr.resize(n);
    for (int v = 0; v < n; ++v) h.llr[v] = log((1 - channel_probs[v]) / channel_probs[v]); // osd_window.pyx:113
}

// Every table that names a message slot, from the one assignment (epos, iperm, dpad): slot of the edge at position j of the check on
// lane l = jptr[j] + l, jptr[j + 1] = jptr[j] + (checks of degree > j) + dpad[j].  Pad slots keep column 0 in row_col and are named
// by no edge word.
void Graph::fill_tables() {
    jptr.assign(K + 1, 0);
    for (int j = 0; j < K; ++j) {
        int cnt = 0;
        for (int l = 0; l < m; ++l) cnt += (row_deg[l] > j);
        jptr[j + 1] = (uint16_t)(jptr[j] + cnt + dpad[j]);
    }
    S = jptr[K];
    row_col.assign(S, 0);
    vn_edge.assign((size_t)std::max(D, 1) * n, SWD_PAD_EDGE);
    vn_row.assign((size_t)std::max(D, 1) * n, 0xFFFF);
    std::vector<int> fill(n, 0), hidx; // hidx: column -> place in the side list of heavy columns (only when there is one)
    if (!hv_id.empty()) {
        hidx.assign(n, -1);
        for (size_t h = 0; h < hv_id.size(); ++h) hidx[hv_id[h]] = (int)h;
        hv_edge.assign(hv_ptr.back(), 0u);
    }
    for (int r = 0; r < m; ++r) {
        const int l = iperm[r];
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
            const int j = epos[e];
            const int v = col_idx[e];
            const int slot = jptr[j] + l;
            row_col[slot] = (uint16_t)v;
            const int k = fill[v]++; // rows ascending: the order the reference's variable-node update sums in
            const uint32_t word = (uint32_t)slot | ((uint32_t)l << 16) | ((uint32_t)j << 26);
            if (!hidx.empty() && hidx[v] >= 0) { hv_edge[hv_ptr[hidx[v]] + k] = word; continue; }
            vn_edge[(size_t)k * n + v] = word;
            vn_row[(size_t)k * n + v] = (uint16_t)r;
        }
    }
}

void Graph::fill_listed() {
    vn_edge_s.assign((size_t)std::max(D, 1) * n, SWD_PAD_EDGE);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < D; ++k) vn_edge_s[(size_t)k * n + i] = vn_edge[(size_t)k * n + vperm[i]];
}

// The device's tables in depth order (swd_graph.h): vn_edge / llr permuted by vdord, after every fill_tables()
void Graph::fill_depth() {
    vn_edge_d.assign((size_t)std::max(D, 1) * n, SWD_PAD_EDGE);
    llr_d.resize(n);
    for (int i = 0; i < n; ++i) {
        llr_d[i] = llr[vdord[i]];
        for (int k = 0; k < D; ++k) vn_edge_d[(size_t)k * n + i] = vn_edge[(size_t)k * n + vdord[i]];
    }
}

bool Graph::fits_depth(const int *depth, int vf, int nt) const {
    if ((long)vf * nt < n) return false;
    for (int i = 0; i < n; ++i)
        if ((int)col_deg[vdord[i]] > depth[i / nt]) return false;
    return true;
}

// The cache image (swd_graph.h): per thread role exactly the registers the tuned osd_window kernel <nt, vf, dm, kg> holds when its
// set-up built them from the tables -- VnCacheP<vf, dm, 0, false>::llr / edp / par (byte offsets of the message cells, parity-word
// byte offsets lane << 2, m << 2 for a dead position) and CnCacheP<kg>::slp with cnt / live / l in one word behind them.  A dead node
// position points at the zero slot of the role's wave, cell S + 1 + nt / 64 + (role >> 6), a dead check position at its far slot,
// cell S + 1 + (role >> 6).  Word order: SwdCacheImg (swd_osdw_kernel.h).
void Graph::fill_image(int nt, int vf, int dm, int kg, const int *depth) {
    const int waves = nt / 64;
    auto node_part = [&](const std::vector<uint32_t> &et, const std::vector<double> &lt, const int *dep, std::vector<uint32_t> &out) {
        int pw = 0; // words of edp[][] = words of par[][] per thread: row i keeps its depth in whole pairs
        for (int i = 0; i < vf; ++i) pw += (std::min(dep ? dep[i] : dm, dm) + 1) / 2;
        const int chunks = (2 * vf + 2 * pw + 3) / 4;
        out.assign((size_t)chunks * nt * 4, 0u);
        std::vector<uint32_t> w((size_t)chunks * 4);
        for (int t = 0; t < nt; ++t) {
            std::fill(w.begin(), w.end(), 0u);
            const uint32_t dead = (uint32_t)(S + 1 + waves + (t >> 6)) << 3, nopar = (uint32_t)m << 2;
            int at = 2 * vf;
            for (int i = 0; i < vf; ++i) {
                const int idx = t + i * nt, kd = std::min(dep ? dep[i] : dm, dm);
                const bool valid = idx < n;
                const double l = valid ? lt[idx] : 0.0;
                uint64_t lb;
                memcpy(&lb, &l, 8);
                w[2 * i] = (uint32_t)lb; w[2 * i + 1] = (uint32_t)(lb >> 32);
                for (int k = 0; k < ((kd + 1) & ~1); ++k) {
                    const uint32_t e = (valid && k < kd && k < D) ? et[(size_t)k * n + idx] : SWD_PAD_EDGE;
                    const uint32_t ed = (e != SWD_PAD_EDGE) ? swd_edge_slot(e) << 3 : dead, ph = (e != SWD_PAD_EDGE) ? swd_edge_lane(e) << 2 : nopar;
                    w[at + (k >> 1)] |= ed << (16 * (k & 1));
                    w[at + pw + (k >> 1)] |= ph << (16 * (k & 1));
                }
                at += (kd + 1) / 2;
            }
            for (int q = 0; q < chunks; ++q) memcpy(&out[((size_t)q * nt + t) * 4], &w[(size_t)q * 4], 16);
        }
    };
    node_part(vn_edge, llr, nullptr, img_vn);
    if (depth) node_part(vn_edge_d, llr_d, depth, img_vn_d); else img_vn_d.clear();
    const int chunks = (2 * kg + 1 + 3) / 4;
    img_cn.assign((size_t)chunks * nt * 4, 0u);
    std::vector<uint32_t> w((size_t)chunks * 4);
    for (int t = 0; t < nt; ++t) {
        std::fill(w.begin(), w.end(), 0u);
        const int cnt = (t < m) ? (int)row_deg[t] : 0;
        const uint32_t far = (uint32_t)(S + 1 + (t >> 6)) << 3;
        for (int k = 0; k < 4 * kg; ++k) w[k >> 1] |= ((k < cnt) ? (uint32_t)(jptr[k] + t) << 3 : far) << (16 * (k & 1));
        w[2 * kg] = ((t < m) ? (uint32_t)t : 0xFFFFu) | ((uint32_t)cnt << 16) | ((uint32_t)cnt << 24);
        for (int q = 0; q < chunks; ++q) memcpy(&img_cn[((size_t)q * nt + t) * 4], &w[(size_t)q * 4], 16);
    }
}

// LDS-array cycles of one variable-node pass over the full graph, from the tables: thread t serves column t (listed: the node at
// position t of the depth order -- 32 resp. 16 consecutive listed positions make a group), edge index k, one 8-byte cell per lane.  ds_read_b64 is served in aligned groups of 32 lanes, bank = cell mod 32; ds_write_b64 in aligned groups
// of 16 lanes, bank = cell mod 16.  A group costs the largest number of (distinct) cells on one bank.
long Graph::layout_cost(long *loads, long *stores, bool listed) const {
    long cl = 0, cs = 0;
    const std::vector<uint32_t> &vn_edge = listed ? this->vn_edge_d : this->vn_edge; // (v below: the listed position)
    for (int k = 0; k < D; ++k)
        for (int v0 = 0; v0 < n; v0 += 16) {
            if ((v0 & 31) == 0) {
                int h[32] = {0}, mx = 0;
                for (int v = v0; v < std::min(n, v0 + 32); ++v) {
                    const uint32_t e = vn_edge[(size_t)k * n + v];
                    if (e != SWD_PAD_EDGE) mx = std::max(mx, ++h[swd_edge_slot(e) & 31]);
                }
                cl += mx;
            }
            int h[16] = {0}, mx = 0;
            for (int v = v0; v < std::min(n, v0 + 16); ++v) {
                const uint32_t e = vn_edge[(size_t)k * n + v];
                if (e != SWD_PAD_EDGE) mx = std::max(mx, ++h[swd_edge_slot(e) & 15]);
            }
            cs += mx;
        }
    if (loads) *loads = cl;
    if (stores) *stores = cs;
    return cl + cs;
}

// Layout optimiser: lowers layout_cost() with the three freedoms no result depends on -- the order of a check's edges over its
// positions (the check pass takes two minima and a parity), which of several checks of one degree takes which lane, and up to
// `pads` pad cells between consecutive diagonals.  Deterministic (no random choice), bounded work; keeps the natural layout when it
// finds nothing better.
void Graph::optimize_layout(int pads, bool listed) {
    const long nat = listed ? layout_cost(nullptr, nullptr, true) : cost_natural; // (the layout is the natural one here)
    if (pads < 0) pads = 0;
    if (E + pads > SWD_MAX_E) pads = SWD_MAX_E - E;
    // per CSR edge: its check, and the load / store group of its (column, edge index inside the column) -- listed: of the column's
    // position in the depth order, the fourth freedom: which thread serves which node changes no result either
    std::vector<int> gl(E), gs(E), erow(E);
    {
        std::vector<int> fill(n, 0);
        for (int r = 0; r < m; ++r)
            for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
                const int v = col_idx[e];
                const int k = fill[v]++;
                const int t = listed ? (int)vdpos[v] : v;
                erow[e] = r;
                gl[e] = (t >> 5) * D + k;
                gs[e] = (t >> 4) * D + k;
            }
    }
    const int NGL = ((n + 31) >> 5) * D, NGS = ((n + 15) >> 4) * D;
    // one pad cell after each of the first diagonals: consecutive diagonals then start on different banks
    std::vector<uint16_t> pad(K, 0);
    for (int j = 0, left = pads; j + 1 < K && left > 0; ++j, --left) pad[j] = 1;
    std::vector<int> jp(K + 1, 0);
    for (int j = 0; j < K; ++j) {
        int cnt = 0;
        for (int l = 0; l < m; ++l) cnt += (row_deg[l] > j);
        jp[j + 1] = jp[j] + cnt + pad[j];
    }
    std::vector<uint8_t> pos(epos);
    std::vector<uint16_t> lane(iperm);
    std::vector<int> slot(E);
    std::vector<uint8_t> hl((size_t)NGL * 32, 0), hs((size_t)NGS * 16, 0);
    for (int e = 0; e < E; ++e) {
        slot[e] = jp[pos[e]] + lane[erow[e]];
        hl[(size_t)gl[e] * 32 + (slot[e] & 31)]++;
        hs[(size_t)gs[e] * 16 + (slot[e] & 15)]++;
    }
    // The search descends on the sum over groups and banks of (cells on the bank)^2, loads counted twice (a load conflict always
    // costs a cycle, a store's only once the array cycles exceed the instruction's six): it falls with every cell that leaves a
    // busier bank for an emptier one, where the cost itself -- the busiest bank per group -- is flat almost everywhere.
    auto mv = [&](int e, int s0, int s1) -> int { // moves edge e from cell s0 to s1, returns the change of the sum
        uint8_t *L = &hl[(size_t)gl[e] * 32], *T = &hs[(size_t)gs[e] * 16];
        int d = 0;
        if ((s0 ^ s1) & 31) { d += 2 * (2 * ((int)L[s1 & 31] - (int)L[s0 & 31]) + 2); L[s0 & 31]--; L[s1 & 31]++; }
        if ((s0 ^ s1) & 15) { d += 2 * ((int)T[s1 & 15] - (int)T[s0 & 15]) + 2; T[s0 & 15]--; T[s1 & 15]++; }
        return d;
    };
    // lanes that may trade places: runs of equal degree
    std::vector<int> run1(m), lane_row(m);
    for (int l = 0; l < m;) { int h = l; while (h < m && row_deg[h] == row_deg[l]) ++h; for (int q = l; q < h; ++q) run1[q] = h; l = h; }
    for (int r = 0; r < m; ++r) lane_row[lane[r]] = r;
    // Every other sweep also takes the moves that leave the sum as it is (they lead off plateaus); lanes trade places in every
    // fourth sweep only, a lane pair costs as much as all the position pairs of its two checks.
    const int kSweeps = 12; // bounds the time of a create: a sweep visits every pair of positions of a check and every pair of lanes of a run
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        long gained = 0;
        for (int r = 0; r < m; ++r)
            for (int a = row_ptr[r]; a < row_ptr[r + 1]; ++a)
                for (int b = a + 1; b < row_ptr[r + 1]; ++b) { // same check, same lane: the two edges trade cells
                    const int sa = slot[a], sb = slot[b];
                    const int d = mv(a, sa, sb) + mv(b, sb, sa);
                    if (d < 0 || (d == 0 && (sweep & 1))) { std::swap(pos[a], pos[b]); slot[a] = sb; slot[b] = sa; gained -= d; }
                    else { mv(b, sa, sb); mv(a, sb, sa); }
                }
        for (int la = 0; la < m && (sweep & 3) == 0; ++la)
            for (int lb = la + 1; lb < run1[la]; ++lb) {
                const int r1 = lane_row[la], r2 = lane_row[lb];
                int d = 0;
                for (int e = row_ptr[r1]; e < row_ptr[r1 + 1]; ++e) d += mv(e, slot[e], slot[e] - la + lb);
                for (int e = row_ptr[r2]; e < row_ptr[r2 + 1]; ++e) d += mv(e, slot[e], slot[e] - lb + la);
                if (d < 0) {
                    for (int e = row_ptr[r1]; e < row_ptr[r1 + 1]; ++e) slot[e] += lb - la;
                    for (int e = row_ptr[r2]; e < row_ptr[r2 + 1]; ++e) slot[e] += la - lb;
                    lane[r1] = (uint16_t)lb; lane[r2] = (uint16_t)la; lane_row[lb] = r1; lane_row[la] = r2;
                    gained -= d;
                } else {
                    for (int e = row_ptr[r2]; e < row_ptr[r2 + 1]; ++e) mv(e, slot[e] - lb + la, slot[e]);
                    for (int e = row_ptr[r1]; e < row_ptr[r1 + 1]; ++e) mv(e, slot[e] - la + lb, slot[e]);
                }
            }
        if (!gained && !(sweep & 1)) break;
    }
    long cur = 0;
    for (int g = 0; g < NGL; ++g) { int mx = 0; for (int b = 0; b < 32; ++b) mx = std::max(mx, (int)hl[(size_t)g * 32 + b]); cur += mx; }
    for (int g = 0; g < NGS; ++g) { int mx = 0; for (int b = 0; b < 16; ++b) mx = std::max(mx, (int)hs[(size_t)g * 16 + b]); cur += mx; }
    if (cur >= nat) return; // nothing better than positions in column order without pads
    epos = pos; iperm = lane; dpad = pad;
    for (int r = 0; r < m; ++r) perm[iperm[r]] = (uint16_t)r; // (equal-degree lanes traded places: row_deg by lane is unchanged)
    fill_tables();
    fill_listed();
    fill_depth();
    cost = layout_cost(nullptr, nullptr, listed);
}

int Graph::build(const swd_graph_desc *g, const std::vector<int32_t> *heavy) {
    if (!g || !g->row_ptr || !g->col_idx || !g->channel_probs) { set_error("null graph description"); return -1; }
    m = g->m; n = g->n; E = g->nnz;
    if (m <= 0 || n <= 0 || E <= 0) { set_error("empty check matrix (m=%d n=%d nnz=%d)", m, n, E); return -1; }
    if (g->row_ptr[0] != 0 || g->row_ptr[m] != E) { set_error("row_ptr does not span nnz"); return -1; }
    if (m > SWD_MAX_M) { set_error(SWD_ERR_CAPACITY, "m=%d exceeds this build's limit of %d checks", m, SWD_MAX_M); return -1; }
    if (n > 65534) { set_error(SWD_ERR_CAPACITY, "n=%d exceeds this build's limit of 65534 columns", n); return -1; }
    if (E > SWD_MAX_E) { set_error(SWD_ERR_CAPACITY, "nnz=%d exceeds this build's limit of %d edges", E, SWD_MAX_E); return -1; }
    row_ptr.assign(g->row_ptr, g->row_ptr + m + 1);
    col_idx.assign(g->col_idx, g->col_idx + E);
    if (csr_check_rows(m, n, row_ptr, col_idx)) return -1;
    // degrees
    row_deg.assign(m, 0);
    col_deg.assign(n, 0);
    K = 0; D = 0;
    std::vector<int> cdeg(n, 0);
    for (int r = 0; r < m; ++r) {
        int d = row_ptr[r + 1] - row_ptr[r];
        if (d > SWD_MAX_ROW_DEG) { set_error(SWD_ERR_CAPACITY, "row %d has weight %d > %d", r, d, SWD_MAX_ROW_DEG); return -1; }
        if (d == 0) { set_error("row %d is empty: every check needs degree > 0 (osd_window.pyx:117)", r); return -1; }
        K = std::max(K, d);
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) cdeg[col_idx[e]]++;
    }
    hv_id.clear(); hv_deg.clear(); hv_ptr.clear(); hv_edge.clear();
    std::vector<int> ldeg(cdeg); // weights the ELL tables see: 0 for a column of the side list
    if (heavy && !heavy->empty()) {
        if (heavy->size() > SWD_MAX_HEAVY) { set_error(SWD_ERR_CAPACITY, "%d heavy columns exceed this build's bound %d", (int)heavy->size(), SWD_MAX_HEAVY); return -1; }
        hv_ptr.push_back(0);
        for (size_t h = 0; h < heavy->size(); ++h) {
            const int v = (*heavy)[h];
            if (v < 0 || v >= n || (h > 0 && v <= (*heavy)[h - 1])) { set_error("heavy column list not ascending inside [0, %d)", n); return -1; }
            hv_id.push_back(v); hv_deg.push_back(cdeg[v]); hv_ptr.push_back(hv_ptr.back() + cdeg[v]);
            ldeg[v] = 0;
        }
    }
    for (int v = 0; v < n; ++v) {
        if (ldeg[v] > SWD_MAX_COL_DEG) { set_error(SWD_ERR_CAPACITY, "column %d has weight %d > %d", v, ldeg[v], SWD_MAX_COL_DEG); return -1; }
        D = std::max(D, ldeg[v]);
        col_deg[v] = (uint8_t)ldeg[v];
    }
    // lanes: checks by degree descending (stable in original index)
    perm.resize(m); iperm.resize(m);
    std::vector<int> order(m);
    for (int r = 0; r < m; ++r) order[r] = r;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return (row_ptr[a + 1] - row_ptr[a]) > (row_ptr[b + 1] - row_ptr[b]);
    });
    for (int l = 0; l < m; ++l) { perm[l] = (uint16_t)order[l]; iperm[order[l]] = (uint16_t)l; row_deg[l] = (uint8_t)(row_ptr[order[l] + 1] - row_ptr[order[l]]); }
    // natural layout: positions in ascending column order, no pad cells
    epos.resize(E);
    for (int r = 0; r < m; ++r)
        for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) epos[e] = (uint8_t)(e - row_ptr[r]);
    dpad.assign(K, 0);
    // CSC with row-ascending entries
    col_ptr.assign(n + 1, 0);
    for (int v = 0; v < n; ++v) col_ptr[v + 1] = col_ptr[v] + cdeg[v];
    row_idx.assign(E, 0);
    {
        std::vector<int> fill(n, 0);
        for (int r = 0; r < m; ++r)
            for (int e = row_ptr[r]; e < row_ptr[r + 1]; ++e) { const int v = col_idx[e]; row_idx[col_ptr[v] + fill[v]++] = r; }
    }
    fill_tables();
    cost_natural = cost = layout_cost();
    llr.resize(n);
    for (int v = 0; v < n; ++v) {
        const double p = g->channel_probs[v];
        llr[v] = log((1 - p) / p); // osd_window.pyx:113
    }
    // listed order of the nodes for the tiered full-graph pass: degree tiers of two positions, heaviest first, stable in the index
    // (a window's column types -- runs of consecutive columns of one degree -- stay runs: neighbouring lanes keep neighbouring slots)
    {
        std::vector<int> ord(n);
        for (int v = 0; v < n; ++v) ord[v] = v;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return (ldeg[a] + 1) / 2 > (ldeg[b] + 1) / 2; });
        vperm.resize(n);
        for (int i = 0; i < n; ++i) vperm[i] = (uint16_t)ord[i];
        fill_listed();
    }
    // depth order: exact degree descending, stable in the index (swd_graph.h)
    {
        std::vector<int> ord(n);
        for (int v = 0; v < n; ++v) ord[v] = v;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return ldeg[a] > ldeg[b]; });
        vdord.resize(n); vdpos.resize(n);
        for (int i = 0; i < n; ++i) { vdord[i] = (uint16_t)ord[i]; vdpos[ord[i]] = (uint16_t)i; }
        fill_depth();
    }
    rank = gf2_rank(m, n, row_ptr, col_idx);
    wm = (m + 63) / 64;
    return 0;
}

int Graph::upload() {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o_jptr = 0;
    size_t o_rowcol = al(o_jptr + jptr.size() * 2);
    size_t o_rowdeg = al(o_rowcol + row_col.size() * 2);
    size_t o_perm = al(o_rowdeg + row_deg.size());
    size_t o_iperm = al(o_perm + perm.size() * 2);
    size_t o_vnedge = al(o_iperm + iperm.size() * 2);
    size_t o_vnrow = al(o_vnedge + vn_edge.size() * 4);
    size_t o_coldeg = al(o_vnrow + vn_row.size() * 2);
    size_t o_llr = al(o_coldeg + col_deg.size());
    size_t o_vdord = al(o_llr + llr.size() * 8);
    size_t o_vnedge_d = al(o_vdord + vdord.size() * 2);
    size_t o_llr_d = al(o_vnedge_d + vn_edge_d.size() * 4);
    size_t o_imgvn = al(o_llr_d + llr_d.size() * 8);
    size_t o_imgvnd = al(o_imgvn + img_vn.size() * 4);
    size_t o_imgcn = al(o_imgvnd + img_vn_d.size() * 4);
    size_t total = al(o_imgcn + img_cn.size() * 4);
    // (the side list of heavy columns behind everything else, only when there is one: the other graphs' images are unchanged)
    const size_t nh = hv_id.size();
    const size_t o_hvid = total, o_hvdeg = al(o_hvid + nh * 4), o_hvptr = al(o_hvdeg + nh * 4), o_hvedge = al(o_hvptr + (nh + 1) * 4);
    if (nh) total = al(o_hvedge + hv_edge.size() * 4 + 4);
    std::vector<char> h(total, 0);
    if (nh) {
        memcpy(&h[o_hvid], hv_id.data(), nh * 4);
        memcpy(&h[o_hvdeg], hv_deg.data(), nh * 4);
        memcpy(&h[o_hvptr], hv_ptr.data(), (nh + 1) * 4);
        if (!hv_edge.empty()) memcpy(&h[o_hvedge], hv_edge.data(), hv_edge.size() * 4);
    }
    memcpy(&h[o_jptr], jptr.data(), jptr.size() * 2);
    memcpy(&h[o_rowcol], row_col.data(), row_col.size() * 2);
    memcpy(&h[o_rowdeg], row_deg.data(), row_deg.size());
    memcpy(&h[o_perm], perm.data(), perm.size() * 2);
    memcpy(&h[o_iperm], iperm.data(), iperm.size() * 2);
    memcpy(&h[o_vnedge], vn_edge.data(), vn_edge.size() * 4);
    memcpy(&h[o_vnrow], vn_row.data(), vn_row.size() * 2);
    memcpy(&h[o_coldeg], col_deg.data(), col_deg.size());
    memcpy(&h[o_llr], llr.data(), llr.size() * 8);
    memcpy(&h[o_vdord], vdord.data(), vdord.size() * 2);
    memcpy(&h[o_vnedge_d], vn_edge_d.data(), vn_edge_d.size() * 4);
    memcpy(&h[o_llr_d], llr_d.data(), llr_d.size() * 8);
    if (!img_vn.empty()) memcpy(&h[o_imgvn], img_vn.data(), img_vn.size() * 4);
    if (!img_vn_d.empty()) memcpy(&h[o_imgvnd], img_vn_d.data(), img_vn_d.size() * 4);
    if (!img_cn.empty()) memcpy(&h[o_imgcn], img_cn.data(), img_cn.size() * 4);
    if (dev.reserve(total)) return -1;
    SWD_HIP(hipMemcpy(dev.p, h.data(), total, hipMemcpyHostToDevice));
    char *b = (char *)dev.p;
    d.m = m; d.n = n; d.E = S; d.nnz = E; d.pad_ = 0; d.K = K; d.D = D; d.rank = rank; d.wm = wm; d.new_n = 0;
    d.jptr = (const uint16_t *)(b + o_jptr);
    d.row_col = (const uint16_t *)(b + o_rowcol);
    d.row_deg = (const uint8_t *)(b + o_rowdeg);
    d.perm = (const uint16_t *)(b + o_perm);
    d.iperm = (const uint16_t *)(b + o_iperm);
    d.vn_edge = (const uint32_t *)(b + o_vnedge);
    d.vn_row = (const uint16_t *)(b + o_vnrow);
    d.col_deg = (const uint8_t *)(b + o_coldeg);
    d.llr = (const double *)(b + o_llr);
    d.vdord = (const uint16_t *)(b + o_vdord);
    d.vn_edge_d = (const uint32_t *)(b + o_vnedge_d);
    d.llr_d = (const double *)(b + o_llr_d);
    d.img_vn = img_vn.empty() ? nullptr : (const uint32_t *)(b + o_imgvn);
    d.img_vn_d = img_vn_d.empty() ? nullptr : (const uint32_t *)(b + o_imgvnd);
    d.img_cn = img_cn.empty() ? nullptr : (const uint32_t *)(b + o_imgcn);
    hv = SwdHeavyDev{};
    if (nh) {
        hv.count = (int32_t)nh; hv.edges = (int32_t)hv_edge.size();
        hv.id = (const int32_t *)(b + o_hvid); hv.deg = (const int32_t *)(b + o_hvdeg);
        hv.ptr = (const int32_t *)(b + o_hvptr); hv.edge = (const uint32_t *)(b + o_hvedge);
    }
    return 0;
}

bool natural_layout_requested() { return env::on(env::NATURAL_LAYOUT); }

} // namespace swd

extern "C" int swd_graph_layout(const swd_graph_desc *g, int32_t pads, int32_t *info, uint16_t *jptr, uint16_t *row_col, uint16_t *perm,
                                uint16_t *iperm, uint8_t *row_deg, uint32_t *vn_edge, uint32_t *vn_edge_s, uint16_t *vperm) {
    swd::Graph G;
    if (G.build(g)) return -1;
    long nl = 0, ns = 0, cl = 0, cs = 0;
    G.layout_cost(&nl, &ns);
    if (!swd::natural_layout_requested()) G.optimize_layout(pads);
    G.layout_cost(&cl, &cs);
    if (info) {
        const int32_t v[8] = {G.S, G.K, G.D, (int32_t)cl, (int32_t)cs, (int32_t)nl, (int32_t)ns, G.S - G.E};
        memcpy(info, v, sizeof v);
    }
    if (jptr) memcpy(jptr, G.jptr.data(), G.jptr.size() * 2);
    if (row_col) memcpy(row_col, G.row_col.data(), G.row_col.size() * 2);
    if (perm) memcpy(perm, G.perm.data(), G.perm.size() * 2);
    if (iperm) memcpy(iperm, G.iperm.data(), G.iperm.size() * 2);
    if (row_deg) memcpy(row_deg, G.row_deg.data(), G.row_deg.size());
    if (vn_edge) memcpy(vn_edge, G.vn_edge.data(), G.vn_edge.size() * 4);
    if (vn_edge_s) memcpy(vn_edge_s, G.vn_edge_s.data(), G.vn_edge_s.size() * 4);
    if (vperm) memcpy(vperm, G.vperm.data(), G.vperm.size() * 2);
    return 0;
}

extern "C" int swd_graph_node_depth(const swd_graph_desc *g, int32_t pads, int32_t nt, int32_t vf, const int32_t *depth, int32_t *info,
                                    uint16_t *vdord, uint32_t *vn_edge_d, double *llr_d, uint32_t *vn_edge, double *llr) {
    swd::Graph G;
    if (G.build(g)) return -1;
    if (nt <= 0 || vf <= 0 || vf > 64 || !depth) { swd::set_error("swd_graph_node_depth: nt, vf > 0, vf <= 64 and a depth per cache row"); return -1; }
    int dep[64];
    for (int i = 0; i < vf; ++i) dep[i] = depth[i];
    const bool fits = G.fits_depth(dep, vf, nt);
    long nl = 0, ns = 0, cl = 0, cs = 0;
    G.layout_cost(&nl, &ns, true);
    if (!swd::natural_layout_requested()) G.optimize_layout(pads, true);
    G.layout_cost(&cl, &cs, true);
    if (info) {
        const int32_t v[8] = {fits ? 1 : 0, G.S, G.D, (int32_t)cl, (int32_t)cs, (int32_t)nl, (int32_t)ns, G.S - G.E};
        memcpy(info, v, sizeof v);
    }
    if (vdord) memcpy(vdord, G.vdord.data(), G.vdord.size() * 2);
    if (vn_edge_d) memcpy(vn_edge_d, G.vn_edge_d.data(), G.vn_edge_d.size() * 4);
    if (llr_d) memcpy(llr_d, G.llr_d.data(), G.llr_d.size() * 8);
    if (vn_edge) memcpy(vn_edge, G.vn_edge.data(), G.vn_edge.size() * 4);
    if (llr) memcpy(llr, G.llr.data(), G.llr.size() * 8);
    return 0;
}

extern "C" int swd_graph_cache_image(const swd_graph_desc *g, int32_t pads, int32_t nt, int32_t vf, int32_t dm, int32_t kg, const int32_t *depth,
                                     int32_t *info, uint32_t *img_vn, uint32_t *img_cn, uint16_t *jptr, uint8_t *row_deg, uint32_t *vn_edge,
                                     double *llr) {
    swd::Graph G;
    if (G.build(g)) return -1;
    if (nt < 64 || nt % 64 || vf <= 0 || vf > 64 || dm <= 0 || dm % 2 || kg <= 0) { swd::set_error("swd_graph_cache_image: nt a multiple of 64, 0 < vf <= 64, dm even, kg > 0"); return -1; }
    if (G.m > nt || G.n > (long)nt * vf || G.D > dm || G.K > 4 * kg) { swd::set_error("swd_graph_cache_image: the graph does not fit a <%d, %d, %d, %d> kernel", nt, vf, dm, kg); return -1; }
    int dep[64];
    for (int i = 0; i < vf && depth; ++i) dep[i] = depth[i];
    if (depth && !G.fits_depth(dep, vf, nt)) { swd::set_error("swd_graph_cache_image: the graph does not fit the depth profile"); return -1; }
    if (!swd::natural_layout_requested()) G.optimize_layout(pads, depth != nullptr);
    if ((G.S + 1 + 2 * (nt / 64)) * 8 > 65536) { swd::set_error("swd_graph_cache_image: %d message slots exceed 16-bit byte offsets", G.S); return -1; }
    G.fill_image(nt, vf, dm, kg, depth ? dep : nullptr);
    const std::vector<uint32_t> &vn = depth ? G.img_vn_d : G.img_vn;
    if (info) {
        const int32_t v[8] = {G.S, G.K, G.D, (int32_t)(vn.size() / ((size_t)nt * 4)), (int32_t)(G.img_cn.size() / ((size_t)nt * 4)), G.S - G.E, 0, 0};
        memcpy(info, v, sizeof v);
    }
    if (img_vn) memcpy(img_vn, vn.data(), vn.size() * 4);
    if (img_cn) memcpy(img_cn, G.img_cn.data(), G.img_cn.size() * 4);
    if (jptr) memcpy(jptr, G.jptr.data(), G.jptr.size() * 2);
    if (row_deg) memcpy(row_deg, G.row_deg.data(), G.row_deg.size());
    if (vn_edge) memcpy(vn_edge, (depth ? G.vn_edge_d : G.vn_edge).data(), G.vn_edge.size() * 4);
    if (llr) memcpy(llr, (depth ? G.llr_d : G.llr).data(), G.llr.size() * 8);
    return 0;
}

extern "C" const char *swd_last_error(void) { return swd::last_error(); }
extern "C" int swd_last_error_class(void) { return swd::last_error_class(); }
extern "C" int swd_abi_version(void) { return SWD_ABI_VERSION; }
extern "C" int swd_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}
