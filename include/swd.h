/*
 * swd.h -- C ABI of the MI355X sliding-window QLDPC decoder (libswd_hip.so).
 *
 * The reference has no FFI layer: its boundary is the Cython extension-type surface
 * re-exported by /root/reference/src/__init__.py:2-4 and called one syndrome at a time from
 * Python loops (/root/reference/osd.py:152-167, guessing.py:160-197).  Each entry point below
 * names the reference interface it replaces.  Plain pointers and sizes only; integer return
 * codes (0 = ok, <0 = error, text via swd_last_error()); no exceptions, no exit().
 *
 * Conventions
 *   - check matrices are passed as CSR over GF(2): row_ptr[m+1], col_idx[nnz] (columns need
 *     not be sorted; duplicates are not allowed);
 *   - syndromes / error vectors are one byte per bit (0/1), row-major [shot][bit];
 *   - "_dev" entry points take DEVICE pointers (e.g. torch tensors' data_ptr()) and a
 *     hipStream_t passed as void*; the others take HOST pointers and copy.
 */
#ifndef SWD_H
#define SWD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWD_ABI_VERSION 4

/* Environment variables (test hooks and diagnostics)
 *
 * The library reads these nineteen variables and nothing else from the environment (csrc/swd_env.h holds the table and the only
 * getenv).  None changes a result; each demands a kernel form or a scheduling that the library would otherwise choose by itself, so a
 * production process sets none of them.
 * Read: P = at its first use, then cached for the process; C = by every handle creation; L = by every launch.
 * Kind: set = on when set to anything, "0" included; nonzero = on when set to anything but "0"; int; text.
 *
 *   variable                   read  kind     effect
 *   SWD_FORCE_HUGE             C     set      swd_osdw_create, swd_gdg_create: the general form (every array in HBM) on any graph
 *   SWD_NATURAL_LAYOUT         C     set      graphs keep the natural message-slot layout (also read by swd_graph_layout and the other
 *                                             host-only layout calls)
 *   SWD_UNIFORM_DEPTH          C     nonzero  osd_window handles keep the uniform node pass where a depth profile would fit
 *   SWD_OWIDE_RING             C     int      large graphs: ring entries of the wide column-form elimination (at least 4; default 64 or 32)
 *   SWD_GRID_PCT               P     int      persistent grid of that percentage of the resident workgroup slots (at least 1; default 100)
 *   SWD_GDG_SERIAL             C     set      guessing decoders: the serial tree walk, never work items
 *   SWD_GDG_STREAM_SERIAL_MIN  L     int      guessing decoders: shots from which a batch with another one in flight walks serially (3072)
 *   SWD_GDG_PAR_MAX_SHOTS      P     int      guessing decoders: shots up to which a launch takes the work-item form (5120)
 *   SWD_GDG_INFLIGHT           P     int      work-item form: side branches of a tree queued or running at a time (at least 1; default 4)
 *   SWD_GDG_SHOTS_PCT          P     int      work-item form: shots admitted up front in percent of the grid (at least 1; default 100 / 400)
 *   SWD_ENS_TICKETS            L     set      threaded ensemble: ticket scheduling instead of the work-item ring
 *   SWD_ENS_NO_TASKS           L     set      threaded ensemble on the ring: every thread body on the unit's workgroup
 *   SWD_BP4_NT                 C     int      bp4_osd: threads of the BP kernel (a multiple of 64 in 64..1024; anything else is ignored)
 *   SWD_BP4_SKEW               P     text     bp4_osd: even | odd -- waves of that index parity sleep before every message-storing node
 *                                             pass of a split launch; anything else is off
 *   SWD_BP4_OVERLAPPED         P     set      bp4_osd: every launch is taken as one with another launch in flight
 *   SWD_BP4_NOSPLIT            C     set      bp4_osd: one thread per qubit also for small codes
 *   SWD_BP4_NO_LAZY            P     set      bp4_osd: the fused node update only
 *   SWD_BP4_GENERIC            L     set      bp4_osd: the generic instantiation instead of the specialised one
 *   SWD_BP4_SPLIT_MAX          C     int      bp4_osd: two threads per qubit up to this value of 2 n (default 256, at most 512)
 */

/* exit class of one window decode, low byte of status[]; bit 8 = converge flag */
enum {
    SWD_EXIT_PRE = 0,       /* pre-processing BP converged    osd_window.pyx:166-170 */
    SWD_EXIT_POST = 1,      /* post-processing BP converged   osd_window.pyx:188-192 */
    SWD_EXIT_OSD = 2,       /* OSD produced the answer        osd_window.pyx:193-195 */
    SWD_EXIT_FAIL_SET = 3,  /* "setting vn failed"            osd_window.pyx:179-181 */
    SWD_EXIT_FAIL_PEEL = 4, /* "peeling failed"               osd_window.pyx:184-186 */
    SWD_EXIT_NO_OSD = 5,    /* BP failed and osd_order == -1  osd_window.pyx:199     */
    SWD_EXIT_SCHED_FAULT = 6 /* pipeline only: the window's predecessor never finished (see swd_pipeline_status);
                                nothing was decoded or committed for this window */
};
#define SWD_STATUS_CONVERGE 0x100

typedef struct swd_graph_desc {
    int32_t m, n, nnz;
    const int32_t *row_ptr;      /* m+1 */
    const int32_t *col_idx;      /* nnz */
    const double *channel_probs; /* n; llr = log((1-p)/p) as osd_window.pyx:113 */
} swd_graph_desc;

/* kwargs of osd_window.__cinit__ (osd_window.pyx:10-16) */
typedef struct swd_osdw_params {
    int32_t pre_max_iter;  /* default 8   */
    int32_t post_max_iter; /* default 100 */
    double ms_scaling_factor;
    int32_t new_n;      /* <=0: min(n, 2m) (osd_window.pyx:60-63) */
    int32_t osd_method; /* 0 osd_0, 1 osd_e, 2 osd_cs (osd_window.pyx:69-79) */
    int32_t osd_order;  /* -1 disables OSD */
} swd_osdw_params;

typedef struct swd_osdw swd_osdw;

/* Why the calling thread's most recent failure happened.  Every failing entry point leaves a message (swd_last_error) and, beside it,
 * one of these classes (swd_last_error_class); both belong to the thread and stand until its next failure -- a call that succeeds
 * leaves them alone.  Code that reacts to a failure reads the class, never the text.
 *   SWD_ERR_FAILED    the default: misuse (a null handle, calls out of order), state, anything unclassified
 *   SWD_ERR_VALUE     the caller's arguments are wrong in a way no form of the library would accept (an OSD order beyond the code's
 *                     range, an unknown OSD method, probabilities that are none); the Python surface raises ValueError, as the
 *                     reference does
 *   SWD_ERR_CAPACITY  the input is valid but beyond a bound of the form that was asked: this build's graph tables, the kernel
 *                     variants, a workgroup's LDS, a general form's own limit.  The only class a fallback follows:
 *                       - swd_osdw_create / swd_gdg_create build the general form when the tuned set-up is refused with this class
 *                         (or SWD_FORCE_HUGE is set); if the general form refuses too, its message and class stand;
 *                       - swd_window_forms reports general = 1 for it and returns -1 for every other class;
 *                       - swd_bp4_create_ex appends the general_form hint to a graph refusal of this class;
 *                       - the Python SlidingWindowDecoder runs its window loop over single-window decoders when
 *                         swd_pipeline_create / swd_pipeline_create_gdg refuse a plan with it.
 *                     A malformed matrix or a failed device call never reaches another form.
 *   SWD_ERR_DEVICE    a HIP call or a device / pinned allocation failed, or no usable device is there */
enum swd_error_class { SWD_ERR_FAILED = 0, SWD_ERR_VALUE = 1, SWD_ERR_CAPACITY = 2, SWD_ERR_DEVICE = 3 };

const char *swd_last_error(void);
int swd_last_error_class(void); /* an enum swd_error_class */
int swd_abi_version(void);
int swd_device_count(void);

/* replaces osd_window(pcm, **kwargs)  (osd_window.pyx:8-126).  device = HIP ordinal. */
swd_osdw *swd_osdw_create(const swd_graph_desc *g, const swd_osdw_params *p, int device);
void swd_osdw_destroy(swd_osdw *d);
/* properties fixed at construction: rank (osd_window.pyx:87), new_n, m, n */
int swd_osdw_info(const swd_osdw *d, int32_t *m, int32_t *n, int32_t *new_n, int32_t *rank);

/* per-decode record, SWD_STAT_WORDS int32 words:
 *   [0] exit class | SWD_STATUS_CONVERGE   (property `converge`)
 *   [1] property `bp_iteration` (pre + post iterations executed)
 *   [2] pre-processing iterations   [3] post-processing iterations
 *   [4] live variable nodes, [5] live checks, [6] live edges of the shortened graph (post phase)
 *   [7] GF(2) row additions applied by the OSD elimination
 * words 2..7 feed the algorithmic-bytes accounting of bench.py. */
#define SWD_STAT_WORDS 8

/* replaces the per-shot loop around osd_window.decode (osd.py:166-167): B independent
 * syndromes in one launch.  Host pointers.
 *   synd   [B*m]   in
 *   out    [B*n]   returned vector of decode() (bp_decoding or osdw_decoding)
 *   stats  [B*SWD_STAT_WORDS]
 *   min_pm [B]     property `min_pm`
 *   hist   [B*4*n] nullable; LLR history, layout [shot][slot][vn]  (property log_prob_ratios is
 *                  its transpose).  If hist_is_state != 0 the buffer is read as the initial
 *                  history too (the reference object keeps it between decodes); otherwise
 *                  every shot starts from a zero history like a freshly built object.
 *   osd0   [B*n]   nullable; property osd0_decoding (only written for SWD_EXIT_OSD shots)
 *   bp_dec [B*n]   nullable; for SWD_EXIT_OSD shots the BP hard decisions the OSD started from (property
 *                  bp_decoding after such a decode, osd_window.pyx:499-501); for every other exit class
 *                  bp_decoding is `out` itself and bp_dec is left untouched                               */
int swd_osdw_decode_batch(swd_osdw *d, int32_t B, const uint8_t *synd, uint8_t *out,
                          int32_t *stats, double *min_pm, double *hist, int32_t hist_is_state,
                          uint8_t *osd0, uint8_t *bp_dec);

/* same, device-resident buffers, asynchronous on `stream` (hipStream_t).  stats / min_pm / hist /
 * osd0 / bp_dec may be NULL; strides are in bytes between consecutive shots (0 = dense). */
int swd_osdw_decode_batch_dev(swd_osdw *d, int32_t B, const uint8_t *synd, int64_t synd_stride,
                              uint8_t *out, int64_t out_stride, int32_t *stats, double *min_pm,
                              double *hist, int32_t hist_is_state, uint8_t *osd0, uint8_t *bp_dec, void *stream);

/* average duration (ms) of the decode kernel launches since the last call, measured with HIP
 * events on the launch stream when timing was enabled with swd_osdw_set_timing(d, 1) */
int swd_osdw_set_timing(swd_osdw *d, int32_t on);
int swd_osdw_get_timing(swd_osdw *d, double *total_ms, int64_t *launches);

/* ---- guessing decoders --------------------------------------------------------------------
 * Replace bpgdg_decoder (single-thread gdg(), the deterministic path), bpgd_decoder and
 * bp_history_decoder of /root/reference/src/bp_guessing_decoder.pyx.  kwargs as in
 * bp_guessing_decoder.pyx:7-9, 162-171, 475-478.  stats words for these decoders:
 *   [0] exit class | SWD_STATUS_CONVERGE (property `converge`), [1] BP iterations in total,
 *   [2] pre-processing iterations, [3] iterations inside decimation steps, [4] snapshots pushed,
 *   [5] BP blocks run, [6] min_converge_depth, [7] scheduling diagnostic, not part of the result:
 *   snapshots of the main branch that ran as work items (0 whenever the launch took the serial
 *   tree walk: large batches, batches of a stream object, posterior history requested).          */
typedef struct swd_gdg_params {
    int32_t max_iter;            /* pre-processing BP iterations (default 50; 8 in the notebooks) */
    double ms_scaling_factor;
    int32_t max_iter_per_step;   /* 6  */
    int32_t max_step;            /* 25 */
    int32_t max_tree_depth;      /* 3  */
    int32_t max_side_depth;      /* 10 */
    int32_t max_tree_branch_step;/* 10 (multi-thread ensemble only; unused by gdg()) */
    int32_t max_side_branch_step;/* 10 */
    double gdg_factor;           /* gdg_factor / gd_factor */
    int32_t new_n;               /* <=0: min(n, 2m) */
    int32_t low_error_mode;
    int32_t mode;                /* 0 bpgdg_decoder, 1 bpgd_decoder, 2 bp_history_decoder */
    int32_t multi_thread;        /* 0: the single-thread gdg() (bit-exact; side branches of one shot run concurrently on different
                                    workgroups).  1: bpgdg_decoder(multi_thread=True), the threaded ensemble of bpgd.cpp:419-688
                                    (main thread, 2^D - 1 tree threads, S - D side threads; kernel kind 7) with the thread
                                    bodies in a fixed order -- identical to the reference on every syndrome whose winning path
                                    metric is not shared by a second, different vector (statistics word 7 counts those; the
                                    reference's own answer depends on thread timing there).  stats for this mode: [4]
                                    hypotheses run, [5] BP blocks, [6] winner (0 main, 1.. tree ids, then side threads; -1 none),
                                    [7] tied hypotheses with a different vector.  Every decode has the state of a NEWLY BUILT
                                    reference object: min_pm_error starts as zeros (when BPGD::reset fails the zero vector comes back; a
                                    reference object that is re-used returns its PREVIOUS decode's vector there, bpgd.cpp:583, 619-625)
                                    and each thread's 4-slot posterior history starts as zeros (a re-used reference thread keeps its
                                    own stale slots when max_iter_per_step < 4).  The oracle and oracle/ref_shim.cpp build a fresh
                                    object per decode too.  2: NOT a reference mode -- every leaf of gdg()'s
                                    decimation tree counts (no min_converge_depth pruning, no snapshot cap), smallest path metric
                                    wins, ties to the earliest in stack order. */
} swd_gdg_params;

typedef struct swd_gdg swd_gdg;
/* Graphs beyond every kernel variant (more than 1024 checks, 9216 columns, row weight 64, column weight 10, or new_n > 2048) take
 * the general form (csrc/swd_huge_gdg.hip, one workgroup per shot, every array in HBM), as swd_osdw_create does; same results and
 * statistics words.  Its bounds, each an error at construction: 4096 checks, 4194304 columns, 4096 snapshots per shot
 * (max_guess, or S - D + 2 for the threaded ensemble); multi_thread = 2 is refused there; modes 0 and 1 refuse a check of weight
 * >= 128 (the reference keeps check degrees in char, bpgd.hpp:23: they wrap, no answer is pinned), mode 2 takes it.
 * Test hook of both constructors: SWD_FORCE_HUGE ("Environment variables" above) makes swd_osdw_create and swd_gdg_create build
 * the general form on any graph.  swd_pipeline_create_gdg refuses windows beyond every pipeline kernel. */
swd_gdg *swd_gdg_create(const swd_graph_desc *g, const swd_gdg_params *p, int device);
void swd_gdg_destroy(swd_gdg *d);
/* host pointers; hist [B*4*n] nullable as in swd_osdw_decode_batch (pre-processing BP history) */
int swd_gdg_decode_batch(swd_gdg *d, int32_t B, const uint8_t *synd, uint8_t *out, int32_t *stats,
                         double *min_pm, double *hist, int32_t hist_is_state);
int swd_gdg_decode_batch_dev(swd_gdg *d, int32_t B, const uint8_t *synd, int64_t synd_stride,
                             uint8_t *out, int64_t out_stride, int32_t *stats, double *min_pm,
                             void *stream);

/* ---- quaternary BP + OSD -------------------------------------------------------------------
 * Replaces bp4_osd(Hx, Hz, channel_probs_x/y/z, max_iter, ms_scaling_factor, osd_method, osd_order)
 * (/root/reference/src/bp4_osd.pyx:8-140) and its decode(sx, sz) (bp4_osd.pyx:197-221).  The
 * variable-node update uses exp/log1p; the device evaluates them with the algorithms of the C library the
 * reference links (glibc >= 2.28: table-driven exp in its FMA build, fdlibm log1p -- csrc/swd_libm.h), so
 * posterior LLRs, decisions and OSD orderings are bit-identical to a reference run on an FMA-capable x86-64.
 * Restrictions (swd_bp4_create fails with a message): column weight of Hx / Hz <= 10, except for up to 8 HEAVY columns
 * (weight above 10 in Hx or Hz, any position, any weight up to m <= 1024: the last qubit of the cycle-assembled and EG codes of
 * Misc.ipynb cells 6-8, H = (H1 | 1), touches every check), which are accepted with osd_order = -1 only unless the handle is
 * created with SWD_BP4_GENERAL_OSD (below) (decode returns the BP
 * decisions of a shot that did not converge; camel_decode never runs OSD) -- with osd_method 0 the caller's -1 stands on such a
 * graph, where the reference resets it to 0 (bp4_osd.pyx:74-76); osd_order > 0 needs
 * rank(Hx) >= rank(Hz) -- the reference sizes BOTH sweeps with kx = n - rank_x (bp4_osd.pyx:103-104, :284): with
 * rank(Hx) > rank(Hz) its z-basis sweep walks fewer candidate columns than exist, which is reproduced (pinned by
 * tests/golden/bp4_unequal_ranks.npz); with rank(Hx) < rank(Hz) it reads past its column array, which is not.
 * Further restrictions of the tuned kernels: at most 1024 checks per matrix, row weights within the graph tables, and the messages
 * of Hx and Hz together within 160 KB of LDS.
 * GENERAL FORM (swd_bp4_create_ex with SWD_BP4_GENERAL_FORM; csrc/swd_huge_bp4.hip): none of the restrictions on the graph -- any
 * row and column weight, up to 1 048 576 qubits, 1 048 576 checks per matrix and 67 108 864 edges in Hx and Hz together (the EG
 * codes [[273,111,17]] and [[1057,571,33]] of Misc.ipynb cell 8, whose every column is above the weight bound; large light codes).
 * One 1024-thread workgroup per shot (per run of a camel shot), every array in HBM.  It is opt-in and takes ANY graph, one the tuned
 * kernels would take included; on its own it runs BP only, so like a graph with heavy columns it is created with osd_order = -1
 * only (with osd_method 0 the caller's -1 stands; SWD_BP4_GENERAL_OSD below lifts both), the same results bit for bit.  Every entry point below dispatches on the handle;
 * swd_bp4_info reports the host GF(2) ranks (-1 only without the elimination on a graph whose dense rows would pass 1 GiB, where
 * they are not computed), swd_bp4_heavy_info (0, 0) (no column is special), swd_bp4_last_form threads = 1024 with the other fields 0.
 * GENERAL OSD (swd_bp4_create_ex with SWD_BP4_GENERAL_OSD; huge_bp4_osd_kernel, csrc/swd_huge_bp4.hip): the elimination and the
 * osd_e / osd_cs sweep in HBM, one 1024-thread workgroup per unconverged decode, no bound on a column's weight.  Opt-in.  With the
 * bit set osd_order >= 0 is taken on a graph with heavy columns (the tuned BP kernel queues for it), with SWD_BP4_GENERAL_FORM
 * beside it on any graph (the general BP kernel queues for it), and on any other graph too (BP in whatever tuned form the graph
 * takes, the elimination in this kernel instead of the tuned one); osd_method 0 resets the order to 0 as the reference does, so
 * Misc.ipynb cell 8's (osd0, -1) runs OSD-0 inside decode like the reference; -1 with methods 1 and 2 stays "no OSD".  The rules
 * above carry over (osd_order <= min(n - rank_x, n - rank_z); osd_order > 0 needs rank(Hx) >= rank(Hz) and walks kx candidates
 * in the z basis; osd_e order <= 15).  Its own bounds, refused at create with a message that names them: at most 4096 checks per
 * matrix (64 words per column of the transform matrix), and one workgroup's elimination arrays within the 8 GiB of a launch
 * slot's area (the grid shrinks to fit first).  Results are those of the reference bit for bit; statistics word 0 is SWD_EXIT_OSD,
 * word 7 the row additions of both bases as the general form of osd_window counts them (not comparable with the tuned kernels'). */
typedef struct swd_bp4_params {
    int32_t max_iter;          /* default 32 */
    double ms_scaling_factor;
    int32_t osd_method;        /* 0 osd_0, 1 osd_e, 2 osd_cs */
    int32_t osd_order;         /* -1 disables OSD */
} swd_bp4_params;
typedef struct swd_bp4 swd_bp4;
swd_bp4 *swd_bp4_create(const swd_graph_desc *hx, const swd_graph_desc *hz, const double *px, const double *py,
                        const double *pz, const swd_bp4_params *p, int device); /* channel_probs of hx/hz ignored */
/* swd_bp4_create with flags: bit 0 (SWD_BP4_GENERAL_FORM) = the general form, bit 1 (SWD_BP4_GENERAL_OSD) = the general
 * elimination.  swd_bp4_create(...) is swd_bp4_create_ex(..., 0). */
#define SWD_BP4_GENERAL_FORM 1
#define SWD_BP4_GENERAL_OSD 2
swd_bp4 *swd_bp4_create_ex(const swd_graph_desc *hx, const swd_graph_desc *hz, const double *px, const double *py,
                           const double *pz, const swd_bp4_params *p, int device, int32_t flags);
int swd_bp4_is_general(const swd_bp4 *d); /* 1: the handle runs the general form, 0: a tuned kernel, -1: null */
int swd_bp4_is_general_osd(const swd_bp4 *d); /* 1: created with SWD_BP4_GENERAL_OSD, 0: not, -1: null */
void swd_bp4_destroy(swd_bp4 *d);
int swd_bp4_info(const swd_bp4 *d, int32_t *mx, int32_t *mz, int32_t *n, int32_t *rank_x, int32_t *rank_z);
/* Heavy columns of the handle's graphs (both pointers nullable): how many columns the decoder treats as heavy (0: none -- the
 * kernel forms of graphs within the column-weight bound) and the largest of their weights in Hx or Hz (0 when there is none). */
int swd_bp4_heavy_info(const swd_bp4 *d, int32_t *count, int32_t *max_degree);
/* The form of the BP kernel the handle's most recent launch took (diagnostics and tests; every pointer nullable):
 * split 1 = two threads per qubit, lazy 1 = the two-half node update, fast 1 = the specialised instantiation (0: generic),
 * wmax / dm = the instantiation's most waves per workgroup and column-weight bound, threads = the workgroup size, skew = the
 * SWD_BP4_SKEW wave stagger (0 off, 1 even, 2 odd; "Environment variables" above), overlapped 1 = taken as a launch with another one in flight.
 * Returns -1 before the first launch. */
int swd_bp4_last_form(const swd_bp4 *d, int32_t *split, int32_t *lazy, int32_t *fast, int32_t *wmax, int32_t *dm,
                      int32_t *threads, int32_t *skew, int32_t *overlapped);
/* sx [B*mx], sz [B*mz] -> out [B*2*n] (row 0: X string, row 1: Z string, like the (2, n) array decode()
 * returns); stats [B*SWD_STAT_WORDS] ([0] exit|converge, [1] bp_iteration); lpr [B*3*n] nullable posterior
 * LLRs laid out [shot][x|y|z][vn] (property log_prob_ratios transposed); osd0 [B*2*n] nullable;
 * bp_dec [B*2*n] nullable: BP hard decisions at exit (properties bp_decoding_x / bp_decoding_z). */
int swd_bp4_decode_batch(swd_bp4 *d, int32_t B, const uint8_t *sx, const uint8_t *sz, uint8_t *out,
                         int32_t *stats, double *lpr, uint8_t *osd0, uint8_t *bp_dec);
int swd_bp4_decode_batch_dev(swd_bp4 *d, int32_t B, const uint8_t *sx, const uint8_t *sz, uint8_t *out,
                             int32_t *stats, double *lpr, uint8_t *osd0, uint8_t *bp_dec, void *stream);
/* bp4_osd.camel_decode (/root/reference/src/bp4_osd.pyx:223-247, called by Misc.ipynb): the last qubit is fixed to
 * I, X, Z, Y in turn, plain BP4 decodes the rest, the converged run of smallest path metric wins (ties: the
 * earliest).  out [B*2*n]; stats [B*SWD_STAT_WORDS] ([0] converge flag, [1] bp_iteration of the last run,
 * [5] winning Pauli or -1); min_pm [B] nullable (10000.0 when no run converged).  Every shot has the state of a
 * newly constructed reference object: without a converged run the zero vectors are returned. */
int swd_bp4_camel_decode_batch(swd_bp4 *d, int32_t B, const uint8_t *sx, const uint8_t *sz, uint8_t *out,
                               int32_t *stats, double *min_pm);
int swd_bp4_camel_decode_batch_dev(swd_bp4 *d, int32_t B, const uint8_t *sx, const uint8_t *sz, uint8_t *out,
                                   int32_t *stats, double *min_pm, void *stream);

/* ---- DEM sampler -----------------------------------------------------------------------------
 * Replaces `dem.compile_sampler().sample(shots)` of the reference harness (/root/reference/osd.py:124-125,
 * guessing.py:129-130; Stim is not available here): per shot, faults e ~ Bernoulli(priors) over the
 * columns of the detector error model, det = chk e, observable flips = obs e over GF(2).
 * chk: num_det x num_col CSR with channel_probs = priors; obs: (<= 32) x num_col CSR or NULL.
 * Stream: Philox4x32-10 keyed by `seed`, counter (shot, column / 4); fault iff x < round(p 2^32); shot b of
 * a call is shot number first_shot + b, so a result does not depend on batching or on the rank. */
typedef struct swd_sampler swd_sampler;
swd_sampler *swd_sampler_create(const swd_graph_desc *chk, const swd_graph_desc *obs, int device);
void swd_sampler_destroy(swd_sampler *s);
int swd_sampler_info(const swd_sampler *s, int32_t *num_det, int32_t *num_col, int32_t *num_obs);
/* det [B*num_det] u8; obs_flips [B] bit masks, nullable; faults [B*num_col] u8, nullable.  Host pointers. */
int swd_sampler_sample(swd_sampler *s, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *det,
                       uint32_t *obs_flips, uint8_t *faults);
/* device pointers (strides in bytes per shot, 0 = dense), asynchronous on `stream` */
int swd_sampler_sample_dev(swd_sampler *s, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *det,
                           int64_t det_stride, uint32_t *obs_flips, uint8_t *faults, int64_t faults_stride,
                           void *stream);

/* ---- code-capacity experiments: Pauli sampler and CSS accounting -------------------------------
 * The data-noise Monte Carlo of the reference on the device: sample, decode (swd_bp4_* or a binary decoder), account, count.
 *
 * Pauli sampler.  Replaces /root/reference/Misc.ipynb cell 2 lines 10-14 (the same lines in cell 8 and in `Data noise.ipynb`):
 *     noise = np.random.uniform(0, 1, (num_shots, code.N))
 *     err_z = np.logical_and(noise > px, noise < (px+py+pz));  syndrome_x = (err_z @ code.hx.T) % 2
 *     err_x = noise < (px+py);                                 syndrome_z = (err_x @ code.hz.T) % 2
 * Per shot and qubit q one 32-bit word u: u < tx -> X, tx <= u < txy -> Y, txy <= u < txyz -> Z, else I, with
 * tx, txy, txyz = round(px 2^32), round((px + py) 2^32), round(((px + py) + pz) 2^32) (floor(v 2^32 + 0.5) clamped to 2^32 - 1, the
 * DEM sampler's rule).  A probability outside [0, 1] or a sum above 1 is refused.  Stream: Philox4x32-10 keyed by `seed`, counter
 * (shot lo, shot hi, q / 4, 1) -- the last word keeps it disjoint from the DEM sampler's stream, which has 0 there -- and output word
 * q % 4 decides qubit q; shot b of a call is shot number first_shot + b, so a result does not depend on batching, lanes or the rank.
 * hx [mx x n], hz [mz x n] CSR (channel_probs ignored); at most 16384 qubits and 65535 checks in total.
 *   err [B][2][n]  row 0 the X string, row 1 the Z string: the layout swd_bp4_decode_batch returns
 *   sx  [B][mx]    Hx err_z          sz [B][mz]  Hz err_x                                  (all uint8) */
typedef struct swd_pauli_sampler swd_pauli_sampler;
swd_pauli_sampler *swd_pauli_sampler_create(const swd_graph_desc *hx, const swd_graph_desc *hz, const double *px, const double *py,
                                            const double *pz, int device);
void swd_pauli_sampler_destroy(swd_pauli_sampler *s);
int swd_pauli_sampler_info(const swd_pauli_sampler *s, int32_t *mx, int32_t *mz, int32_t *n);
/* host pointers */
int swd_pauli_sampler_sample(swd_pauli_sampler *s, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *err, uint8_t *sx,
                             uint8_t *sz);
/* device pointers (strides in bytes per shot, 0 = dense), asynchronous on `stream` */
int swd_pauli_sampler_sample_dev(swd_pauli_sampler *s, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *err,
                                 int64_t err_stride, uint8_t *sx, int64_t sx_stride, uint8_t *sz, int64_t sz_stride, void *stream);

/* CSS accounting: did the correction leave a logical error?  Replaces Misc.ipynb cell 2 lines 32-36, 39-43 and 45 (cell 8: 26-32)
 *     e_diff_z = (e_hat_z + err_z[i]) % 2;  logical_z_err = ((e_diff_z @ code.hz_perp.T) % 2).any()
 *     e_diff_x = (e_hat_x + err_x[i]) % 2;  logical_x_err = ((e_diff_x @ code.hx_perp.T) % 2).any()
 *     num_log_err += (logical_z_err or logical_x_err);  num_flag_err += 1 - bpd.converge
 * and /root/reference/src/simulation.py:25-28, 51-56, 90-93 (one basis).  hz_perp = ker(hz) has the row space of [Hx; Lx], so "some row of
 * hz_perp has odd overlap" is "some row of [Hx; Lx] has"; the rows are passed split, which also tells a residual syndrome from
 * a logical flip.
 *   cx  CSR applied to the Z string: its first stab_x rows are stabilisers (Hx), the rest logical operators (Lx)
 *   cz  CSR applied to the X string: Hz, then Lz
 * Either may be NULL: estimate and error are then single strings of n bytes per shot (the binary decoders, simulation.py); with
 * both, [2][n] bytes per shot as the Pauli sampler and swd_bp4_decode_batch lay them out.  Any number of logical rows; at most
 * 65535 rows in total, 16384 qubits.
 * account: with d = est ^ err, result[b] (nullable) =
 *   bit 0  some row has odd overlap with its string of d                       (the reference's criterion)
 *   bit 1  some stabiliser row has: the residual syndrome is not zero          (implies bit 0)
 *   bit 2  stats is given and stats[b * SWD_STAT_WORDS] & stat_mask is zero: with SWD_STATUS_CONVERGE, the mask of every
 *          decode call above, the decoder did not converge                      (1 - converge)
 * counters: nullable device uint64[4] = shots, bit-0, bit-1, bit-2 counts, ADDED to (one integer atomic per counter and
 * workgroup); the caller zeroes them.  Device pointers, strides in bytes per shot (0 = dense), asynchronous on `stream`. */
typedef struct swd_css_account swd_css_account;
swd_css_account *swd_css_account_create(const swd_graph_desc *cx, int32_t stab_x, const swd_graph_desc *cz, int32_t stab_z, int device);
void swd_css_account_destroy(swd_css_account *a);
int swd_css_account_dev(swd_css_account *a, int32_t B, const uint8_t *est, int64_t est_stride, const uint8_t *err, int64_t err_stride,
                        const int32_t *stats, int32_t stat_mask, int32_t *result, uint64_t *counters, void *stream);

/* ---- sliding-window pipeline ---------------------------------------------------------------
 * Replaces the window loop of the reference harness (/root/reference/osd.py:130-179, identical in
 * guessing.py:135-214 and the notebooks): for every shot, decode window t on the residual
 * syndrome, commit the first `commit` columns of the estimate into total_e_hat, update the
 * residual syndrome det ^ chk * total_e_hat, go to window t+1.  One launch for B shots. */
typedef struct swd_window_desc {
    swd_graph_desc graph; /* window matrix incl. the merged noisy-syndrome identity (osd.py:103-113) */
    int32_t row0;         /* first detector row of the window            (anchors[top_left][0]) */
    int32_t col0;         /* first global column of the window           (anchors[top_left][1]) */
    int32_t commit;       /* committed leading columns (osd.py:140,170-173) */
    int32_t reserved;
} swd_window_desc;

typedef struct swd_pipeline swd_pipeline;

/* chk = region-permuted global check matrix [num_det x num_col] (CSR), used for the residual
 * update (osd.py:178).  All windows share the decoder parameters p (osd.py:152-161). */
swd_pipeline *swd_pipeline_create(int32_t num_windows, const swd_window_desc *wins,
                                  const swd_graph_desc *chk, const swd_osdw_params *p, int device);
/* same window loop with a guessing decoder in every window (guessing.py:135-214) */
swd_pipeline *swd_pipeline_create_gdg(int32_t num_windows, const swd_window_desc *wins,
                                      const swd_graph_desc *chk, const swd_gdg_params *p, int device);
void swd_pipeline_destroy(swd_pipeline *pl);
int swd_pipeline_info(const swd_pipeline *pl, int32_t *num_windows, int32_t *num_det,
                      int32_t *num_col, int32_t *lds_bytes, int32_t *threads);
/* optional: observables matrix obs [num_obs x num_col] (CSR, num_obs <= 32) for the on-device
 * logical accounting of osd.py:184-187 */
int swd_pipeline_set_observables(swd_pipeline *pl, const swd_graph_desc *obs);
/* det [B*num_det] in; total [B*num_col] out (total_e_hat); stats [B*W*SWD_STAT_WORDS], min_pm
 * [B*W] and shot_result [B*2] nullable.  shot_result[2b] = bit mask of the observables the
 * committed faults flip (obs @ total_e_hat, needs swd_pipeline_set_observables), shot_result[2b+1]
 * = 1 if the residual syndrome det ^ chk @ total_e_hat is non-zero ("flagged").  Host pointers. */
int swd_pipeline_decode(swd_pipeline *pl, int32_t B, const uint8_t *det, uint8_t *total,
                        int32_t *stats, double *min_pm, int32_t *shot_result);
/* device pointers, asynchronous on `stream` */
int swd_pipeline_decode_dev(swd_pipeline *pl, int32_t B, const uint8_t *det, int64_t det_stride,
                            uint8_t *total, int64_t total_stride, int32_t *stats, double *min_pm,
                            int32_t *shot_result, void *stream);
/* Scheduling-fault flags accumulated by every launch of this pipeline since the last call, read and cleared
 * (0 = none; bit 0: a window waited more than 10 s for its predecessor window of the same shot, which cannot
 * happen by construction -- its statistics record SWD_EXIT_SCHED_FAULT; bit 1: a workgroup of the guessing decoders'
 * work-item loop found nothing to do for 20 s while units were still outstanding and left -- results incomplete).  Synchronises the device, so call it
 * after the asynchronous swd_pipeline_decode_dev launches it should cover; swd_pipeline_decode checks it itself. */
int swd_pipeline_status(swd_pipeline *pl, uint32_t *flags);

/* total_e_hat bit-packed: total_bits [B * ((num_col + 7) / 8)], bit (c & 7) of byte (c >> 3) of a shot's row = column c
 * (numpy: np.unpackbits(bits, axis=1, count=num_col, bitorder="little")).  1098 B per shot instead of 8784 for the [[144,12,12]]
 * experiment -- the per-shot output SURVEY section 8(e) counts.  Host pointers; otherwise as swd_pipeline_decode. */
int swd_pipeline_decode_packed(swd_pipeline *pl, int32_t B, const uint8_t *det, uint8_t *total_bits,
                               int32_t *stats, double *min_pm, int32_t *shot_result);

/* ---- streaming form of the window loop -------------------------------------------------------
 * Consecutive batches through ONE pipeline, two in flight (what a deployment, or the shots loop of the reference harness
 * /root/reference/osd.py:130-191 cut into batches, does): a stream object owns two lanes, each with its own HIP stream, launch
 * slot, device buffers and page-locked staging.  Batch k + 1 is copied in and launched while batch k still runs: its persistent
 * grid takes the workgroup slots that the tail of batch k leaves empty, and the copy-out / unpacking of batch k overlaps the
 * launch of k + 1.  Results are those of swd_pipeline_decode, batch by batch, in push order.  (Guessing decoders: a stream batch of
 * 3072 shots or more walks each decimation tree serially instead of spreading its side branches over the grid as work items --
 * the next batch fills the tail the serial walk leaves; same results, statistics word 7 aside.  A caller that alternates streams of
 * its own with swd_pipeline_decode_dev gets the same choice: a launch that finds the handle's previous launch still running on
 * another stream is treated as a stream batch.)
 *   flags  SWD_STREAM_PACKED    total_e_hat is returned bit-packed (layout of swd_pipeline_decode_packed)
 *          SWD_STREAM_NO_STATS  per-window stats / min_pm are not copied back (pop takes NULL for them)
 * Host form: push(det [B*num_det]) enqueues copy-in + launch + copy-out on the next lane and returns at once; pop() waits for
 * the OLDEST batch in flight and fills the caller's arrays (total [B*num_col] bytes, or [B*((num_col+7)/8)] with
 * SWD_STREAM_PACKED; stats / min_pm / shot_result nullable), returns its B.  At most two batches in flight: a third push without a
 * pop fails.  A scheduling fault of the batch (see swd_pipeline_status) makes its pop fail.
 * Device form: push_dev launches on the next lane with the caller's device buffers (the caller keeps one set of output buffers
 * per lane, i.e. alternates between two); `after` (hipStream_t) = a stream whose work so far must precede the launch: the
 * producer of det and whoever still reads the lane's output buffers.  NULL means the legacy default stream, as everywhere in HIP
 * (the lanes are non-blocking streams and do not synchronise with it by themselves); SWD_STREAM_NO_DEPENDENCY skips the wait
 * (inputs and output buffers already synchronised by the caller).  wait(stream): `stream` waits for both lanes (device-side), or
 * with NULL the host does.
 * Lifetime: destroy the stream objects of a pipeline before the pipeline.  The other order is tolerated -- swd_pipeline_destroy
 * drains and detaches the live stream objects, every later call on them fails with a message, swd_pipeline_stream_destroy still
 * frees them -- but must not race with calls on those stream objects from other threads.
 * A scheduling fault (see swd_pipeline_status) is reported by the pop of the batch it happened in: every launch has a fault word
 * of its own next to the decoder's sticky one. */
typedef struct swd_stream swd_stream;
#define SWD_STREAM_PACKED 1
#define SWD_STREAM_NO_STATS 2
#define SWD_STREAM_NO_DEPENDENCY ((void *)(intptr_t)-1)
swd_stream *swd_pipeline_stream_create(swd_pipeline *pl, int32_t max_shots, int32_t flags);
void swd_pipeline_stream_destroy(swd_stream *s);
int swd_pipeline_stream_push(swd_stream *s, int32_t B, const uint8_t *det);
int swd_pipeline_stream_pop(swd_stream *s, uint8_t *total, int32_t *stats, double *min_pm, int32_t *shot_result);
int swd_pipeline_stream_pending(swd_stream *s); /* host batches pushed and not yet popped (0..2) */
int swd_pipeline_stream_push_dev(swd_stream *s, int32_t B, const uint8_t *det, int64_t det_stride, uint8_t *total,
                                 int64_t total_stride, int32_t *stats, double *min_pm, int32_t *shot_result, void *after);
int swd_pipeline_stream_wait(swd_stream *s, void *stream);
/* `stream` waits (device-side) for the lane of the most recent push or push_dev alone -- what the consumer of batch k needs, so that
 * batch k + 1 on the other lane stays in flight.  Fails if nothing has been pushed on this stream object. */
int swd_pipeline_stream_wait_last(swd_stream *s, void *stream);

/* ---- device window loop: plans beyond the one-launch pipeline kernels ---------------------------
 * The same window loop (/root/reference/osd.py:130-179) for plans whose windows swd_pipeline_create refuses with SWD_ERR_CAPACITY --
 * more than 1024 checks, 9216 columns, row weight 64 or column weight 10 in a window: [[756,16,<=34]] at (W, F) = (3, 1),
 * [[288,12,18]] at W = 8 -- and, on request, for any other plan.  Opt-in (csrc/swd_loop.hip); additive, SWD_ABI_VERSION stays 4.
 * The handle owns ONE single-window decoder per DISTINCT window, built through swd_osdw_create (decoder = 0, params = swd_osdw_params*)
 * or swd_gdg_create (decoder = 1, params = swd_gdg_params*): each takes a tuned kernel, a large-graph kernel or the general form by
 * itself, and SWD_FORCE_HUGE keeps its meaning.  Two windows are the same when matrix and priors agree (new_n is one parameter of the
 * loop): the BB plans have 4 windows and 3 distinct ones, which matters because every general-form handle holds CUs x slice of scratch.
 * It keeps the CSC of chk with int32 rows, the observable masks (obs nullable, <= 32 rows), and buffers that grow with B: the residual
 * syndrome [B][num_det rounded up to 4], the estimate [B][largest window n], one window's statistics and path metrics.
 *   create     NULL with a message and class.  A refusal of a window's own create stands with its class, "window <t>: " in front.
 *              SWD_ERR_CAPACITY of the loop itself: the committed columns of a window reach a span of more than 65 536 rows of chk
 *              (one commit stages the span in LDS; on the BB plans the span lies inside the window).
 *   info       all nullable; device_bytes = the handle's own arrays as they are now (the window decoders' graphs and scratch not counted)
 *   decode_dev arguments and results exactly those of swd_pipeline_decode_dev: det is not modified, total is zeroed first, stats
 *              [B][W][SWD_STAT_WORDS] (every word of the window decode), min_pm [B][W] and shot_result [B][2] nullable.  Everything is
 *              queued on `stream`: begin (resid = det), then per window its *_decode_batch_dev on resid + row0 with the residual's
 *              stride and one commit launch (loop_commit_kernel: committed faults into total, their columns of chk into the residual
 *              rows they reach, their observable masks into the accumulator, the window's record to [shot][window]; the last window's
 *              launch also reduces "residual != 0" into shot_result).  No host synchronisation of its own -- a general-form window
 *              decoder still synchronises with its previous stream when the stream changes.  Decodes of one handle on different
 *              streams are ordered by an event (the buffers are shared), so results do not depend on how streams alternate.
 *   decode     the same with host pointers (det [B*num_det], total [B*num_col], ...); synchronous.
 * Not served: stream objects, sessions of every kind, rolling experiments -- they need the one-launch pipeline. */
typedef struct swd_window_loop swd_window_loop;
swd_window_loop *swd_window_loop_create(int32_t num_windows, const swd_window_desc *wins, const swd_graph_desc *chk,
                                        const swd_graph_desc *obs, int32_t decoder, const void *params, int device);
void swd_window_loop_destroy(swd_window_loop *l);
int swd_window_loop_info(const swd_window_loop *l, int32_t *num_windows, int32_t *num_det, int32_t *num_col,
                         int32_t *distinct_decoders, int64_t *device_bytes);
int swd_window_loop_decode_dev(swd_window_loop *l, int32_t B, const uint8_t *det, int64_t det_stride, uint8_t *total,
                               int64_t total_stride, int32_t *stats, double *min_pm, int32_t *shot_result, void *stream);
int swd_window_loop_decode(swd_window_loop *l, int32_t B, const uint8_t *det, uint8_t *total, int32_t *stats,
                           double *min_pm, int32_t *shot_result);

/* ---- memory experiments: per-shot accounting of a window-loop batch ------------------------------
 * The last lines of the reference's sliding_window_decoder (/root/reference/osd.py:181-191) on the device, so that sample -> window
 * loop -> count needs no per-shot array on the host.
 *   shot_result [B][2]  as swd_pipeline_decode_dev writes it     true_flips [B]  as swd_sampler_sample_dev writes obs_flips
 *   stats [B][W][SWD_STAT_WORDS], nullable: only words 0 and 1 are read
 * result[b] (nullable) =
 *   bit 1  flagged: shot_result[2b+1] != 0
 *   bit 2  observable mismatch: shot_result[2b] != true_flips[b]
 *   bit 0  bit 1 or bit 2                                         (np.logical_or(flagged_err, logical_err), osd.py:184-188)
 * counters (nullable) uint64[4] = shots, bit-0, bit-1, bit-2 counts: the layout of swd_css_account_dev.
 * window_counters (nullable, used with stats) uint64[W][SWD_WINDOW_COUNTER_WORDS]: words 0-7 the histogram of the exit class
 * stats[b][t][0] & 7, word 8 the shots with stats[b][t][0] & SWD_STATUS_CONVERGE zero, word 9 the sum of stats[b][t][1].
 * failed (nullable) uint64[1 + failed_cap]: word 0 is ADDED to with the number of shots that have bit 0; the global number
 * first_shot + b of such a shot is stored at 1 + slot while slot < failed_cap, slot = what word 0 held before the add of its
 * workgroup plus its rank among the workgroup's failing shots; later ones are counted only.  Which shots are stored when they do
 * not all fit, and the order of those stored, depend on arrival; the counts and the sorted complete list do not.
 * All three are ADDED to with integer atomics (one per non-zero sum and workgroup); the caller zeroes them.  Device pointers,
 * asynchronous on `stream`; B = 0 does nothing. */
#define SWD_WINDOW_COUNTER_WORDS 10
int swd_shot_account_dev(int device, int32_t B, int32_t W, const int32_t *shot_result, const uint32_t *true_flips,
                         const int32_t *stats, uint64_t first_shot, int32_t *result, uint64_t *counters,
                         uint64_t *window_counters, uint64_t *failed, int32_t failed_cap, void *stream);

/* Logical errors per GROUP of observables (the X and the Z logicals of a two-basis experiment, say): counters[g] is ADDED to with
 * the number of shots b that have (shot_result[2b] ^ true_flips[b]) & masks[g] != 0, for g < num_groups <= SWD_MAX_OBSERVABLE_GROUPS.
 * Flagged shots count only through their observables; a zero mask counts nothing; masks may overlap.  `masks` is a HOST array
 * [num_groups], read before the call returns; shot_result, true_flips and counters (uint64[num_groups], zeroed by the caller) are
 * device pointers.  One integer atomic per non-zero sum and workgroup, asynchronous on `stream`; B = 0 or no group does nothing. */
#define SWD_MAX_OBSERVABLE_GROUPS 4
int swd_group_account_dev(int device, int32_t B, const int32_t *shot_result, const uint32_t *true_flips, int32_t num_groups,
                          const uint32_t *masks, uint64_t *counters, void *stream);

/* ---- rolling DEM sampler: the detector rows of an experiment of any length, round block by round block ----------
 * A detector error model of R0 rounds whose columns are region-permuted (windows.plan_windows) falls into R0 + 1 column blocks,
 * one per row block of h = n_half detector rows: block b = columns [anchor_cols[b], anchor_cols[b + 1]) holds the faults that first
 * show in row block b, and they reach into row block b + 1 at most.  When the blocks j0 .. j1 - 1 (the BODY) are translates of one
 * another, the model of R rounds of the same circuit is, for every R >= R0 - (j1 - j0):
 *     the head blocks 0 .. j0 - 1 as they are | block j0 repeated (j1 - j0) + (R - R0) times, copy k with its rows moved down by k h
 *     (observable masks and priors as they are) | the tail blocks j1 .. R0 with their rows moved down by (R - R0) h
 * (windows.extend_template is the executable statement; tests/test_rolling_experiment_host.py holds it against plan_windows(R)).
 * The rolling sampler draws that model's detector rows a few row blocks at a time, bit-identical to swd_sampler_* on the R-round
 * model, in device memory that does not depend on R: what a memory experiment on a rolling session needs.
 *   create   chk: (R0 + 1) h x num_col CSR with channel_probs = priors; obs: (<= 32) x num_col CSR or NULL; anchor_cols [num_blocks + 1]
 *            = first column of every block, then num_col (strictly increasing from 0; num_blocks = R0 + 1); 0 <= j0 < j1 <=
 *            num_blocks - 1.  Refused with a message: a column of block b with a row outside [b h, (b + 2) h); body blocks that
 *            differ in length, rows (moved), observable masks or thresholds; more than 32 observables; h > 32767.  Per template
 *            column the device keeps the threshold (round(p 2^32), the rule of swd_sampler_create), the observable mask and the
 *            rows as u16 relative to the block's first row (0 .. 2 h - 1).
 *   rows_dev ONE STATELESS call: det_rows[b][0 .. nblocks h) = rows [block0 h, (block0 + nblocks) h) of shot first_shot + b of
 *            the `rounds`-round experiment (stride = bytes between shots, 0 = nblocks h); obs_flips [B] (nullable) is XORed INTO
 *            with the observable masks of the faults in column blocks block0 .. block0 + nblocks - 1, so a sweep of calls over all
 *            R + 1 blocks counts every column once (the caller zeroes it first); faults (nullable) [b][0 .. columns of those blocks)
 *            = the faults of these same column blocks (faults_stride = bytes between shots, 0 = their number of columns).  The
 *            call draws column blocks block0 - 1 .. block0 + nblocks - 1: a block between two calls is drawn by both, each keeping
 *            its own half of the rows.  Stream: that of swd_sampler_* on the GLOBAL column number c of the R-round model --
 *            Philox4x32-10 keyed by `seed`, counter (shot lo, shot hi, c >> 2, 0), output word c & 3, fault iff x < threshold of
 *            the template column c maps to.  The result is a pure function of (seed, shot number, rounds, block range): nothing
 *            depends on the order of calls.  Refused: rounds < R0 - (j1 - j0); a block range outside 0 .. rounds; rounds whose
 *            model has 2^34 columns or more (c >> 2 is counter word 2).  Asynchronous on `stream`; long calls are split into
 *            several launches.  B = 0 does nothing.
 *   rows     the same with host pointers, dense ([B][nblocks h], [B], [B][columns]); obs_flips is read, XORed into and written back
 *   info     info[8] = { h, num_col, num_obs, R0, j0, j1, least rounds served, 0 }; with rounds >= 0 also (all nullable) the
 *            R-round model's first column of block `block0` and the number of columns of blocks block0 .. block0 + nblocks - 1 */
typedef struct swd_rolling_sampler swd_rolling_sampler;
swd_rolling_sampler *swd_rolling_sampler_create(const swd_graph_desc *chk, const swd_graph_desc *obs, int32_t n_half, int32_t j0,
                                                int32_t j1, const int64_t *anchor_cols, int32_t num_blocks, int device);
void swd_rolling_sampler_destroy(swd_rolling_sampler *s);
int swd_rolling_sampler_info(const swd_rolling_sampler *s, int32_t *info, int32_t rounds, int32_t block0, int32_t nblocks,
                             int64_t *first_col, int64_t *num_cols);
int swd_rolling_sampler_rows_dev(swd_rolling_sampler *s, int32_t B, uint64_t seed, uint64_t first_shot, int32_t rounds,
                                 int32_t block0, int32_t nblocks, uint8_t *det_rows, int64_t stride, uint32_t *obs_flips,
                                 uint8_t *faults, int64_t faults_stride, void *stream);
int swd_rolling_sampler_rows(swd_rolling_sampler *s, int32_t B, uint64_t seed, uint64_t first_shot, int32_t rounds, int32_t block0,
                             int32_t nblocks, uint8_t *det_rows, uint32_t *obs_flips, uint8_t *faults);

/* ---- circuit sampler: Pauli-frame simulation of a memory circuit's op list ----------------------------------------
 * The forward execution of the gate / noise / measurement lists that circuit.dem_from_ops analyses backwards (the reference leaves
 * this to Stim): per shot the raw MEASUREMENT RECORD of the noisy circuit -- what swd_frontend_* and the measurement sessions
 * take -- and, as parities of it, detectors and true observable flips in the form swd_sampler_sample_dev writes them.  Additive;
 * SWD_ABI_VERSION stays 4 (csrc/swd_circuit.hip).
 * State per shot and qubit: two bits x, z (the Pauli frame against a noiseless run).  Ops in list order, op codes of circuit.py
 * (R 0, RX 1, H 2, CX 3, M 4, MR 5, MRX 6, XERR 7, DEP1 8, DEP2 9, MX 12, ZERR 13; DETECTOR 10 and OBSERVABLE 11 are not ops of the
 * program: they are the two maps); rnd = the op's randomisation bit, 0 when `randomize` is 0:
 *     R q: x = 0, z = rnd            RX q: z = 0, x = rnd           H q: swap x, z          CX c,t: x[t] ^= x[c], z[c] ^= z[t]
 *     M q,i: rec[i] = x, z = rnd     MR q,i: rec[i] = x, x = 0, z = rnd     MX q,i: rec[i] = z, x = rnd     MRX q,i: rec[i] = z, z = 0, x = rnd
 *     XERR / ZERR q: flip x / z iff u < thr          DEP1 q: iff u < thr, Pauli 1 + (u 3) / thr on q (1 X, 2 Y, 3 Z; Y flips both)
 *     DEP2 a,b: iff u < thr, k = 1 + (u 15) / thr, Pauli k >> 2 on a and k & 3 on b (0 = I); the products are 64-bit integers
 * thr = min(floor(p 2^32 + 0.5), 2^32 - 1), the DEM sampler's rule, computed by the caller.  Streams: Philox4x32-10 keyed by `seed`;
 * noise ops are numbered j = 0, 1, ... in list order and u is output word j % 4 of counter (shot lo, shot hi, j / 4, 2); the ops
 * that take rnd (R, RX, M, MR, MX, MRX) are numbered r = 0, 1, ... in list order and rnd is bit r % 32 of output word (r / 32) % 4 of
 * counter (shot lo, shot hi, r / 128, 3) -- counter words 3 = 0 and 1 are the DEM and the Pauli sampler's.  Shot b of a call is shot
 * number first_shot + b: a result is a pure function of (program, seed, shot number), whatever the batch, the lanes or the rank.
 *   create   one entry per op: kind, qa, qb (two-qubit ops), thr (noise ops), meas (record index of a measurement), noise_slot and
 *            rand_slot (the op's number j or r; they must count up in list order); entries an op does not use are ignored.
 *            det_map [num_det x num_meas], obs_map [num_obs x num_meas] (either nullable): CSR, row = the measurements a detector /
 *            an observable is the parity of (channel_probs ignored).  SWD_ERR_VALUE: a code that is not executable, a qubit or a
 *            measurement index out of range, a measurement written twice or never, slots out of order, a map that reads outside
 *            the record.  SWD_ERR_CAPACITY: more than 4096 qubits (a wave keeps 16 bytes per qubit in 64 KB of LDS).
 *   info     info[8] = { qubits, measurements, detectors, observables, noise slots, randomisation slots, device bytes, qubit bound }
 *   measure_dev  meas [B][num_meas] bytes, or with packed != 0 [B][ceil(num_meas / 8)] with measurement i in bit i & 7 of byte
 *            i >> 3 (the front end's packed layout); meas_stride = bytes between shots, 0 = dense; bytes past a row are not touched
 *   sample_dev   det [B][num_det] bytes (det_stride as above), obs_flips [B] bit masks (nullable; SWD_ERR_CAPACITY when asked for
 *            with more than 32 observables), meas (nullable) the unpacked record of the same shots
 * Both are asynchronous on `stream` (two launches) and keep, per stream HANDLE they have been called on, ceil(B / 64) num_meas 8
 * bytes of device memory between the launches (the largest B so far; released with the sampler, not before: a caller that keeps
 * creating streams should call the sampler on a fixed set of them, or destroy it with them).  Calls on different streams may
 * overlap.  Calls on ONE stream share that buffer and rely on the stream's order: two host threads must not call one sampler on the
 * same stream at the same time (the handle is otherwise safe to share between threads).  measure / sample: the same with host
 * pointers, dense, synchronous, on the null stream.  B = 0 does nothing. */
typedef struct swd_circuit_sampler swd_circuit_sampler;
swd_circuit_sampler *swd_circuit_sampler_create(int32_t num_ops, const int32_t *kind, const int32_t *qa, const int32_t *qb,
                                                const uint32_t *thr, const int32_t *meas, const int32_t *noise_slot,
                                                const int32_t *rand_slot, int32_t num_qubits, int32_t num_meas,
                                                const swd_graph_desc *det_map, const swd_graph_desc *obs_map, int32_t randomize, int device);
void swd_circuit_sampler_destroy(swd_circuit_sampler *s);
int swd_circuit_sampler_info(const swd_circuit_sampler *s, int64_t *info);
int swd_circuit_sampler_measure_dev(swd_circuit_sampler *s, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *meas,
                                    int64_t meas_stride, int32_t packed, void *stream);
int swd_circuit_sampler_sample_dev(swd_circuit_sampler *s, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *det,
                                   int64_t det_stride, uint32_t *obs_flips, uint8_t *meas, int64_t meas_stride, void *stream);
int swd_circuit_sampler_measure(swd_circuit_sampler *s, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *meas, int32_t packed);
int swd_circuit_sampler_sample(swd_circuit_sampler *s, int32_t B, uint64_t seed, uint64_t first_shot, uint8_t *det,
                               uint32_t *obs_flips, uint8_t *meas);

/* ---- online sessions: the window loop driven by the arrival of detector rows --------------------
 * The (W, F) scheme exists so that corrections are committed while the experiment still runs; the loop of the reference harness
 * (/root/reference/osd.py:130-179) is causal -- window t reads only rows < row1 of det ^ chk @ total_e_hat.  A session owns the state
 * of ONE batch of shots on the device: the residual syndrome (zero at the start), total_e_hat, the observable accumulators and the
 * per-window records.  push hands over the next nrows detector rows of every shot, in row order, in pieces of any size (0 included):
 * they are XORed into the residual syndrome, and every window whose last row has now arrived (the last window: every row of the
 * experiment) is decoded at once -- the pipeline's own kernel, launched for that window alone -- and committed: its first `commit`
 * columns go into total_e_hat, their columns of chk are XORed into the residual syndrome, rows that have NOT arrived yet included
 * (osd.py:170-178).  Every result is bit-identical to swd_pipeline_decode of the whole experiment, whatever the chunking (guessing
 * decoders: statistics word 7 aside, as ever).
 *   begin       zeroes the state for a batch of B <= max_shots shots; also restarts a used session (osd.py:130-131)
 *   push        det_rows [B*nrows] host bytes, row-major per shot; returns after the windows it made ready have been committed:
 *               *first / *count = those windows (both nullable).  Errors: before begin, after the last window has been committed,
 *               more rows than the experiment has.                                                        (osd.py:165-178)
 *   push_dev    the same with a device pointer (stride = bytes between consecutive shots, 0 = nrows), asynchronous on `stream`:
 *               merge, decode and commit are queued there in that order.  Calls on different streams are ordered by the session.
 *   window      committed part of window t (t < windows committed): faults [B*commit] = total_e_hat[:, col0 : col0 + commit],
 *               stats [B*SWD_STAT_WORDS], min_pm [B]; host pointers, all nullable; waits for the work queued so far   (osd.py:166-173)
 *   finish      after the last window: total [B*num_col], stats [B*W*SWD_STAT_WORDS], min_pm [B*W], shot_result [B*2] as
 *               swd_pipeline_decode returns them (host pointers, all nullable); before the last window it fails, and the message
 *               names the detector rows still missing.  The state stays readable until the next begin.     (osd.py:184-187)
 *   buffers     device view for the push_dev caller: total_e_hat (columns committed so far, the others zero), its stride, progress
 * Lifetime and threading as for the stream objects: several sessions of one pipeline may be alive and interleaved, each owns its
 * state; their launches are serialised on the host like all launches of the pipeline handle.  Destroy the sessions before the
 * pipeline; the other order is tolerated in the same way (every later call fails with a message, destroy still frees). */
typedef struct swd_session swd_session;
swd_session *swd_pipeline_session_create(swd_pipeline *pl, int32_t max_shots);
void swd_pipeline_session_destroy(swd_session *s);
int swd_pipeline_session_begin(swd_session *s, int32_t B);
int swd_pipeline_session_push(swd_session *s, int32_t nrows, const uint8_t *det_rows, int32_t *first, int32_t *count);
int swd_pipeline_session_push_dev(swd_session *s, int32_t nrows, const uint8_t *det_rows, int64_t stride, int32_t *first,
                                  int32_t *count, void *stream);
int swd_pipeline_session_window(swd_session *s, int32_t t, uint8_t *faults, int32_t *stats, double *min_pm);
int swd_pipeline_session_finish(swd_session *s, uint8_t *total, int32_t *stats, double *min_pm, int32_t *shot_result);
int swd_pipeline_session_buffers(swd_session *s, uint8_t **total, int64_t *total_stride, int32_t *rows_received,
                                 int32_t *windows_done);

/* ---- rolling sessions: experiments of any length on a frame of residual rows ------------------------
 * An online session is tied to the number of rounds its plan was built for.  For a memory experiment every window between the first
 * and the last is a translate of ONE window, so a pipeline built for R0 rounds serves as a TEMPLATE: head = window 0, body = window 1,
 * tail = last window, F * h = row stride between windows.  A rolling session decodes experiments of every length R = R0 (mod F),
 * known only when they end, bit-identical to swd_pipeline_decode of a pipeline built for R rounds; its device memory does not depend
 * on R.  Per shot it keeps a FRAME of residual rows whose row 0 is the first row of the window decoded next, the observable
 * accumulator and a sticky flagged bit.  Arriving rows are XORed into the frame; as soon as the frame holds the next window's rows it
 * is decoded (the pipeline's own kernel, launched for that window alone) and committed: the first `commit` columns are written to the
 * step's output, their columns of chk are XORed into the frame, their observable masks into the accumulator, the F * h rows that
 * scroll out are ORed into the flagged bit and the frame moves down by F * h rows.
 *   create      checks the template: at least a first, one body and a last window; body windows share one matrix, commit and stride;
 *               their committed columns of chk and observable masks are translates; no committed column touches a row before its
 *               window.  NOT checked here: the priors (a body window with other priors than window 1 is caught only as a
 *               different window graph, a template with ONE body window not at all), and the periodicity of chk / obs when there
 *               is one body window only.  windows.rolling_template is the full check -- priors, chk and obs per body ROUND -- and
 *               the Python layer runs it before create; a caller of the C ABI answers for the periodicity of its own template.
 *   begin       zero state for a batch of B <= max_shots shots; also restarts a used session
 *   push        the next nrows detector rows of every shot (host bytes [B*nrows], any number, 0 included).  EVERY row handed to push
 *               counts as a row of a syndrome round: the final data-measurement block must go to finish, push cannot tell the
 *               difference and a whole final block would complete a body window.  Windows completed by the call: *count of them,
 *               numbered *first .. (from 0, without bound); window k of the call writes faults [k][B][commit_max] (its first
 *               `commit` columns of each row; commit_max = max of the head's and the body's commit, info[7]), stats
 *               [k][B][SWD_STAT_WORDS], min_pm [k][B]; all nullable.  The call fails before it does anything if it would complete
 *               more than max_windows windows (the capacity of those arrays).  Nothing of a window is kept after the call.
 *   push_dev    the same with device pointers (stride = bytes between consecutive shots, 0 = nrows), asynchronous on `stream`
 *   finish      the remaining nrows >= 1 rows, the final block among them, then the tail window, committed whole: faults
 *               [B][tail commit], stats [B][SWD_STAT_WORDS], min_pm [B], shot_result [B][2] = observable flips of every fault
 *               committed since begin, flagged (the sticky bit OR the rows left in the frame) as swd_pipeline_decode returns them.
 *               Fails, leaving the state as it was, if the rows do not make an experiment the template serves (R = R0 (mod F) rounds
 *               with a head and a tail window); the message names the lengths served.  After finish: begin.
 *   finish_dev  the same with device pointers, asynchronous on `stream`
 *   state       rows received and windows committed since begin, rows in the frame, info[8] = { frame rows, rows the next window
 *               waits for in the frame, row stride, tail rows, head commit, body commit, tail commit, commit_max }, bytes of
 *               device memory the session owns (a function of max_shots and the template alone); all nullable
 * Stream ordering, lifetime and threading as for the online sessions. */
typedef struct swd_rolling swd_rolling;
swd_rolling *swd_pipeline_rolling_create(swd_pipeline *pl, int32_t max_shots);
void swd_pipeline_rolling_destroy(swd_rolling *s);
int swd_pipeline_rolling_begin(swd_rolling *s, int32_t B);
int swd_pipeline_rolling_push(swd_rolling *s, int32_t nrows, const uint8_t *det_rows, int32_t max_windows, uint8_t *faults,
                              int32_t *stats, double *min_pm, int64_t *first, int32_t *count);
int swd_pipeline_rolling_push_dev(swd_rolling *s, int32_t nrows, const uint8_t *det_rows, int64_t stride, int32_t max_windows,
                                  uint8_t *faults, int32_t *stats, double *min_pm, int64_t *first, int32_t *count, void *stream);
int swd_pipeline_rolling_finish(swd_rolling *s, int32_t nrows, const uint8_t *final_rows, uint8_t *faults, int32_t *stats,
                                double *min_pm, int32_t *shot_result);
int swd_pipeline_rolling_finish_dev(swd_rolling *s, int32_t nrows, const uint8_t *final_rows, int64_t stride, uint8_t *faults,
                                    int32_t *stats, double *min_pm, int32_t *shot_result, void *stream);
int swd_pipeline_rolling_state(swd_rolling *s, int64_t *rows_received, int64_t *windows_done, int32_t *frame_fill, int32_t *info,
                               int64_t *device_bytes);

/* ---- detector front end: raw measurement records in, detector rows out ------------------------------
 * A running experiment produces measurement outcomes; the sessions above take detector rows.  Every detector of a memory
 * experiment is the parity of measurements of its own round and of the round before it, and the rounds after the first are
 * translates of one another, so three templates state the whole map (measurements.py, MeasurementMap.blocks, builds and checks them):
 *     head, body  [n_half x 2 meas_per_round]             CSR over [previous round's measurements | this round's measurements]: round 0
 *                                                         (no entry in the first half) and every later syndrome round
 *     tail        [n_half x (meas_per_round + meas_final)] CSR over [last syndrome round | final block]: the detectors of the final block
 *     obs_tail    [(<= 32) x the same]                     the observables (nullable: none)
 * (channel_probs of the descriptors is ignored.)  A front end owns, for one batch of shots, the last complete round's outcomes and
 * the bits of the round under way: 2 meas_per_round bytes per shot, whatever the length of the experiment, so it serves fixed and
 * rolling sessions alike.  Refused at create: 2 meas_per_round + meas_final > 32768 (what one launch stages), a template of another
 * shape, an entry outside its columns.
 *   begin       zero state for a batch of B <= max_shots shots; also restarts a used front end
 *   push_dev    the next nbits measurement bits of every shot, any number, 0 included; a chunk may end inside a round and inside a
 *               byte.  packed = 0: one byte per bit (non-zero = 1); packed = 1: bit (i & 7) of byte (i >> 3) of the chunk -- every
 *               chunk starts at bit 0 of its own buffer.  stride = bytes between the shots' buffers (0 = dense: nbits, or
 *               (nbits + 7) / 8 packed); buffers that are 8-byte aligned (pointer and stride) are read with 8-byte loads.  Writes
 *               the detector rows of every round the bits completed, det_rows [B][*rows_out] (det_stride = bytes between shots, 0 =
 *               *rows_out), the layout swd_pipeline_session_push_dev and swd_pipeline_rolling_push_dev read.  *rows_out (nullable) =
 *               ((bits of the round under way + nbits) / meas_per_round) n_half is computed on the host: the caller sizes det_rows by
 *               the same rule from `state`; nothing is read back from the device.  One launch (more when a push is longer than a
 *               launch stages), asynchronous on `stream`; calls on different streams are ordered by the front end.
 *               EVERY bit handed to push counts as a bit of a syndrome round: the final block goes to finish.
 *   finish_dev  the rest of the syndrome round under way, if any (whole further rounds are taken too), then the final block: writes
 *               the remaining detector rows, the final block's n_half among them, and raw_obs [B]: bit k = the parity of observable
 *               k's measurements.  Fails, with the state unchanged, unless the bits complete the last syndrome round exactly, bring
 *               the whole final block and at least one syndrome round has been seen.  After finish: begin.
 *   push/finish the same with host pointers, dense, synchronous
 *   state       bits received and syndrome rounds completed since begin; info[8] = { meas_per_round, meas_final, n_half, observables,
 *               bits of the round under way, final block taken, B, max_shots }; bytes of device memory owned; all nullable */
typedef struct swd_frontend swd_frontend;
swd_frontend *swd_frontend_create(const swd_graph_desc *head, const swd_graph_desc *body, const swd_graph_desc *tail,
                                  const swd_graph_desc *obs_tail, int32_t meas_per_round, int32_t meas_final, int32_t n_half,
                                  int32_t max_shots, int device);
void swd_frontend_destroy(swd_frontend *fe);
int swd_frontend_begin(swd_frontend *fe, int32_t B);
int swd_frontend_state(swd_frontend *fe, int64_t *bits_received, int64_t *rounds_done, int32_t *info, int64_t *device_bytes);
int swd_frontend_push_dev(swd_frontend *fe, int32_t nbits, const uint8_t *meas, int64_t stride, int32_t packed, uint8_t *det_rows,
                          int64_t det_stride, int32_t *rows_out, void *stream);
int swd_frontend_finish_dev(swd_frontend *fe, int32_t nbits, const uint8_t *final_meas, int64_t stride, int32_t packed,
                            uint8_t *det_rows, int64_t det_stride, int32_t *rows_out, uint32_t *raw_obs, void *stream);
int swd_frontend_push(swd_frontend *fe, int32_t nbits, const uint8_t *meas, int32_t packed, uint8_t *det_rows, int32_t *rows_out);
int swd_frontend_finish(swd_frontend *fe, int32_t nbits, const uint8_t *final_meas, int32_t packed, uint8_t *det_rows,
                        int32_t *rows_out, uint32_t *raw_obs);

/* Threading and streams: every entry point may be called from any host thread.  Launches of ONE decoder /
 * pipeline handle are serialised on the host while they are prepared; on the device, launches on different streams
 * run concurrently -- each launch takes its scheduling scratch from a ring of four launch slots, and a fifth launch
 * in flight makes its stream wait for the first (hipStreamWaitEvent).  The same holds for swd_bp4 handles (the queue
 * of unconverged decodes between the BP and the OSD kernel, the internal posterior buffer and the camel_decode
 * scratch belong to the launch slot).  Host-buffer entry points of one handle are mutually exclusive for their
 * whole duration (they share staging buffers). */

/* diagnostics: device-side phase timers (100 MHz ticks) of the last launch, out [B*W*8]:
 * init, pre BP, sort, shorten+peel, post BP, OSD sort, OSD elimination, OSD sweep + epilogue */
int swd_pipeline_set_profiling(swd_pipeline *pl, int32_t on);
int swd_pipeline_get_profile(swd_pipeline *pl, int32_t B, int64_t *out);
int swd_pipeline_set_timing(swd_pipeline *pl, int32_t on);
int swd_pipeline_get_timing(swd_pipeline *pl, double *total_ms, int64_t *launches);

/* diagnostics: occupies `blocks` workgroups of `threads` threads with `lds_bytes` of LDS each for `microseconds` (bounded: at most
 * 2 s) on `stream` -- a foreign, long-running kernel for tests of the persistent grids' forward progress under reduced
 * residency (tests/test_gpu_forward_progress.py: blocks that each take more than half a CU's LDS hold one CU apiece). */
int swd_diag_occupy(int device, int32_t blocks, int32_t threads, int32_t lds_bytes, int32_t microseconds, void *stream);

/* diagnostics: evaluates one routine of the quaternary decoder's arithmetic element by element, out[i] = f(x[i]) (ops 4 and 6:
 * f(x[i], y[i]); y may be NULL otherwise), on n fp64 DEVICE arrays with an ordinary grid-stride kernel on `stream` -- the device
 * build of csrc/swd_libm.h and of the composites on top of it, which tests/test_gpu_libm.py holds to a host build of the same header
 * bit for bit.  op: 0 swd_exp (constant table); 1 swd_exp_from with the table copied to LDS as bp4_kernel copies it; 2 swd_log1p;
 * 3 bp4_log1pexp and 4 bp4_logaddexp (csrc/swd_bp4_kernel.h, LDS table, the forms of the BP loops); 5 / 6 the general form's
 * called copies hb_log1pexp / hb_logaddexp, launched from the translation unit that owns them (csrc/swd_huge_bp4.hip). */
int swd_diag_libm(int device, int32_t op, int64_t n, const double *x, const double *y, double *out, void *stream);

/* diagnostics, host only (needs no device): the message-slot layout of graph g as a pipeline built now would lay it out with up to
 * `pads` pad cells -- the bank-conflict-aware layout, or under SWD_NATURAL_LAYOUT ("Environment variables" above) the natural one
 * (positions in column order, no pads).  info[8] = { slots, K, D, model cost of the loads, of the stores, the natural layout's two costs,
 * pad cells used }; the arrays (any of them may be NULL) are sized jptr [K + 1], row_col [slots], perm / iperm / row_deg [m],
 * vn_edge / vn_edge_s [D * n], vperm [n]: call once with NULL arrays for the sizes.  The cost is in LDS-array cycles of one
 * variable-node pass over the full graph (csrc/swd_graph.hip, Graph::layout_cost). */
int swd_graph_layout(const swd_graph_desc *g, int32_t pads, int32_t *info, uint16_t *jptr, uint16_t *row_col, uint16_t *perm,
                     uint16_t *iperm, uint8_t *row_deg, uint32_t *vn_edge, uint32_t *vn_edge_s, uint16_t *vperm);

/* Depth-profiled node pass (csrc/swd_variants.h, SWD_DEPTH_PROFILES): an osd_window handle or pipeline whose kernel variant declares
 * a depth profile and whose window graphs all fit it serves the full graph's nodes in descending-degree order, a fixed number of
 * edge positions per row of the register cache; every other handle keeps the uniform pass over the variant's column-weight bound.
 * Both compute the same results.  1: profiled, 0: uniform (the launches of such a handle that write a posterior history keep the
 * uniform kernel).  Test hook: SWD_UNIFORM_DEPTH ("Environment variables" above) keeps the uniform form, as SWD_NATURAL_LAYOUT
 * keeps the natural message-slot layout. */
int swd_osdw_node_depth(const swd_osdw *h);
int swd_pipeline_node_depth(const swd_pipeline *pl);

/* diagnostics, host only: the depth order of graph g and the layout a pipeline that launches a depth-profiled kernel of `nt` threads
 * and `vf` cache rows of depths depth[vf] would build with up to `pads` pad cells (thread t serves the nodes at listed positions
 * t, t + nt, ...; SWD_NATURAL_LAYOUT as above).  info[8] = { graph fits the profile, slots, D, listed-order model cost of the loads,
 * of the stores, the natural layout's two costs in that model, pad cells used }; vdord [n] = the listed nodes (exact degree
 * descending, stable in the column), vn_edge_d [D * n] / llr_d [n] = the tables in that order, vn_edge [D * n] / llr [n] = the final
 * tables in column order; any array may be NULL. */
int swd_graph_node_depth(const swd_graph_desc *g, int32_t pads, int32_t nt, int32_t vf, const int32_t *depth, int32_t *info,
                         uint16_t *vdord, uint32_t *vn_edge_d, double *llr_d, uint32_t *vn_edge, double *llr);

/* Cache image (csrc/swd_graph.h, SwdGraphDev::img_*): the osd_window kernels of up to 256 threads load the full graph's register
 * caches ready-made, packed once per graph when a handle is created.  diagnostics, host only: the image of graph g as a pipeline that
 * launches the kernel variant <nt, vf, dm, kg> would build it with up to `pads` pad cells -- depth NULL: the uniform node part (row i of
 * thread role t serves column t + i * nt over dm positions), else depth[vf]: the node part of that depth profile (listed node
 * t + i * nt of the depth order over depth[i] positions; the graph must fit) and the layout of such a plan.  In 16-byte chunks,
 * chunk-major and role-minor: word w of role t is at ((w / 4) * nt + t) * 4 + w % 4.
 *   node part, words of a role in order: the prior of each row (low word, high word; +0.0 for a row without a node); then for each row
 *   its edge positions two per word (low half first) as byte offsets of their message cells, slot << 3; then for each row the
 *   positions' checks as lane << 2.  A row takes its depth rounded up to whole pairs; a position without an edge holds the byte
 *   offset of cell slots + 1 + nt / 64 + t / 64 and the check m << 2.
 *   check part, role t = lane t: positions 0 .. 4 kg - 1 two per word as byte offsets (jptr[k] + t) << 3, beyond the check's
 *   degree (and for t >= m) the offset of cell slots + 1 + t / 64; then one word (t, or 0xFFFF for t >= m) | degree << 16 | degree << 24.
 * info[8] = { slots, K, D, chunks of the node part, chunks of the check part, pad cells used, 0, 0 }; img_vn [chunks * nt * 4], img_cn
 * likewise, and the tables the image was packed from: jptr [K + 1], row_deg [m] by lane, vn_edge [D * n] / llr [n] in the order the
 * node part serves (columns, or the depth order).  Any array may be NULL: call once with NULL arrays for the sizes. */
int swd_graph_cache_image(const swd_graph_desc *g, int32_t pads, int32_t nt, int32_t vf, int32_t dm, int32_t kg, const int32_t *depth,
                          int32_t *info, uint32_t *img_vn, uint32_t *img_cn, uint16_t *jptr, uint8_t *row_deg, uint32_t *vn_edge,
                          double *llr);

/* diagnostics: which forms of the window kernels (csrc/swd_osdw_kernel.h, pipeline_kernel) a plan takes.  The kernel variant, the
 * LDS-resident or large-graph form and each window's LDS layout decide which code a launch runs; these calls report the decision,
 * taken by the code that builds a handle (csrc/swd_plan.h, Plan::select_forms) and by the conditions the kernels themselves test
 * (swd_osd0_routine, swd_post_form).
 * plan [SWD_FORM_PLAN_WORDS]:
 *   [0..3] threads, variable nodes per thread, column-weight bound, groups of four row positions of the variant; [4] the full-graph
 *   phase splits heavy checks; [5] large-graph form; [6] every window graph fits the variant's depth profile; [7] LDS bytes per
 *   workgroup; [8] guessing decoders: work-item form available; [9] guessing decoders: depth-2 cache of the shortened graph;
 *   [10] general form (no window kernel takes the plan: words 0..9 are 0); [11] kernel kind of the most recent launch -- 0 / 3
 *   osd_window (3: history sum in registers), 5 / 6 the same on large graphs, 1 / 2 / 7 guessing decoders (serial walk, work items,
 *   threaded ensemble), 8 / 9 serial walk and ensemble on large graphs -- [12] that launch was scheduled as a stream batch, [13] it
 *   ran the depth-profiled kernel; [11..13] are -1 before the first launch, from swd_window_forms and in the general form.
 * window [num_windows][SWD_FORM_WINDOW_WORDS] (all -1 in the general form):
 *   [0] live-slot lists of the post phase: 0 staged in the scratch region, 1 a region of their own, 2 none; [1] post_lds; [2] osd_lds;
 *   [3] ring entries of the wide column-form elimination (0: none); [4] the higher-order sweep has arrays of its own (1) or lies over
 *   the sort keys (0); [5] candidates it evaluates at a time; [6] bytes of live mask per check (6 or 8); [7] OSD-0 elimination:
 *   0 osd0_quad, 1 osd0_wave_reg, 2 osd0_cols, 3 osd0_colsw, 4 osd0_block; [8] post phase: 0 sorted, 1 live-slot lists, 2 no lists,
 *   3 renumbered (large graphs) -- [7], [8] are -1 under a guessing decoder; [9] T of the heavy-check split and [10..12] checks served
 *   by one / two / four threads, [13] threads they take together (0 where [4] of the plan is 0); [14] 64-bit words per column of
 *   the check matrix; [15] pad cells of the graph's slot layout.
 * Any output may be NULL. */
#define SWD_FORM_PLAN_WORDS 16
#define SWD_FORM_WINDOW_WORDS 16
/* host only (needs no device): the forms a handle built now from these windows would take.  Exactly one of p (osd_window) and gp
 * (guessing decoders) is given; num_det = rows of the global check matrix of a pipeline, <= 0 for a single-window handle (its
 * `reserved`, row0, col0 and commit are then 0).  A plan no window kernel takes (a refusal of class
 * SWD_ERR_CAPACITY) is reported (plan[10]), not refused; input that no form takes -- a malformed matrix, an OSD order out of range --
 * returns -1 with its message. */
int swd_window_forms(int32_t num_windows, const swd_window_desc *wins, int32_t num_det, const swd_osdw_params *p,
                     const swd_gdg_params *gp, int32_t *plan, int32_t *window);
/* the handle's forms and its most recent launch */
int swd_osdw_last_form(const swd_osdw *h, int32_t *plan, int32_t *window);
int swd_gdg_last_form(const swd_gdg *h, int32_t *plan, int32_t *window);
int swd_pipeline_last_form(const swd_pipeline *pl, int32_t *plan, int32_t *window);

#ifdef __cplusplus
}
#endif
#endif
