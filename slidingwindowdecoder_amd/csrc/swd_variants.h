// Kernel variants: threads per shot, variable nodes per thread, column-degree bound, groups of four row positions,
// sf (the full-graph phase shares heavy checks among threads: needs the host-built map, 4 * kg may be < K),
// then which further kernels exist for the variant: guessing decoders in serial form (kind 1) and parallel form
// (kind 2), osd_window with the posterior history accumulated in registers (kind 3).
// A plan uses the first variant with NT >= m, NT * VF >= n, DM >= D, 4 * KG >= K over all its windows.
// X(nt, vf, dm, kg, sf, has_k1, has_k2, has_k3)
#pragma once
#if defined(SWD_HEADLINE_ONLY) // development builds: only the [[144,12,12]] kernels
#define SWD_VARIANTS(X) X(256, 7, 6, 9, 0, 1, 1, 1)
#elif defined(SWD_V7816_ONLY) // development builds: the <256, 7, 8, 16> kernels
#define SWD_VARIANTS(X) X(256, 7, 8, 16, 0, 1, 1, 0)
#elif defined(SWD_BB288_ONLY) // development builds: only the [[288,12,18]] kernels
#define SWD_VARIANTS(X) X(1024, 5, 6, 6, 1, 0, 0, 1) X(1024, 5, 6, 9, 0, 1, 0, 1)
#else
#define SWD_VARIANTS(X)                                                                                              \
    X(64, 4, 4, 2, 0, 1, 1, 0)      /* small codes, e.g. [[72,12,6]] hx (n=72, D=3, K=6) */                             \
    X(64, 4, 8, 16, 0, 1, 1, 0)                                                                                         \
    X(256, 2, 8, 16, 0, 1, 1, 0)                                                                                        \
    X(256, 4, 8, 16, 0, 1, 1, 0)                                                                                        \
    X(256, 2, 10, 12, 0, 1, 1, 1)   /* SHYPS r=3 circuit-level windows (63 x 476, column weight <= 9) */                \
    X(256, 7, 6, 9, 0, 1, 1, 1)     /* [[144,12,12]] circuit-level windows */                                           \
    X(256, 7, 8, 16, 0, 1, 1, 0)                                                                                        \
    X(1024, 5, 6, 6, 1, 0, 0, 1)    /* [[288,12,18]] circuit-level windows, osd_window */                               \
    X(1024, 5, 6, 9, 0, 1, 0, 1)    /* [[288,12,18]] circuit-level windows */                                           \
    X(1024, 3, 10, 12, 0, 1, 0, 0)  /* SHYPS r=3 twelve-round windows (252 x 2240, column weight 9, row weight 44) */   \
    X(1024, 8, 8, 16, 0, 1, 0, 0)
#endif

// Depth profiles (optional, per variant; osd_window kind 3): the full-graph node pass serves the nodes in descending-degree order,
// NT per cache row, and row i of the register cache walks depth[i] edge positions -- a compile-time constant -- instead of DM.
// A plan whose graphs all fit (every node listed in row i has degree <= depth[i]) launches the profiled instantiation, any other
// plan the uniform one.  {6,6,3,3,3,3,2}: the three [[144,12,12]] window graphs (at most 504 nodes of degree > 3, 1512 of degree > 2).
// X(nt, vf, dm, kg, depth[0], ..., depth[vf - 1])
#if defined(SWD_V7816_ONLY) || defined(SWD_BB288_ONLY)
#define SWD_DEPTH_PROFILES(X)
#else
#define SWD_DEPTH_PROFILES(X) X(256, 7, 6, 9, 6, 6, 3, 3, 3, 3, 2)
#endif

// Large graphs (row J of the scope table: osd_window on matrices whose fp64 messages do not fit a CU's LDS, e.g. the un-windowed
// 936 x 8784 detector error model of /root/reference/IBM.ipynb:119): one 1024-thread workgroup per shot, the scratch region of
// the layout in HBM (pipeline_kernel<..., BIG>).  Chosen when no variant above fits.  X(nt, vf, dm, kg)
#define SWD_BIG_VARIANTS(X)                                                                                           \
    X(1024, 9, 6, 9)     /* [[144,12,12]] global DEM: 936 x 8784, column weight 6, row weight 35 */                      \
    X(1024, 9, 10, 16)   /* up to 1024 checks, 9216 columns, column weight 10, row weight 64 */
