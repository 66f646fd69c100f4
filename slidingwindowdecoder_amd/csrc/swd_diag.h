// Diagnostic build switches of the kernel headers, and the only place that tests one.  SWD_IF_<NAME>(...) is its arguments in a build
// with -DSWD_<NAME> (scripts/devbuild.sh -DSWD_<NAME>, or make SWD_DEV_DEFS=-DSWD_<NAME>) and nothing in the product, so a
// diagnostic statement is one line at the indentation of the code around it.  Two rules of the preprocessor: a // comment goes in front
// of an invocation or behind its closing parenthesis, never behind its last statement, and a block with a directive of its own (#pragma)
// cannot be an argument.  tests/test_build_switches.py holds the kernel headers to this; DESIGN.md section 4 lists all build switches.
#pragma once

#ifdef SWD_BPPROF // cycles of the parts of a post-phase BP iteration and of the steps of osd0_wave_reg / osd0_quad, in s.scal[20..28] -> profile words (scripts/bp_profile.py)
#define SWD_IF_BPPROF(...) __VA_ARGS__
#else
#define SWD_IF_BPPROF(...)
#endif
#ifdef SWD_OSDPROF // cycles per elimination of osd0_block / osd0_cols / osd0_colsw (resolver, column waves, barriers), printed by the kernel; no script of its own
#define SWD_IF_OSDPROF(...) __VA_ARGS__
#else
#define SWD_IF_OSDPROF(...)
#endif
#ifdef SWD_INITPROF // where the set-up of a window goes: reset loops | cache loads | barrier | bp_init | check caches | ordered_pm (scripts/init_profile.py, subphase_profile.py)
#define SWD_IF_INITPROF(...) __VA_ARGS__
#else
#define SWD_IF_INITPROF(...)
#endif
#ifdef SWD_SHPROF // sub-phase split of the shortening step, profile words 1..5 (scripts/sh_profile.py, subphase_profile.py)
#define SWD_IF_SHPROF(...) __VA_ARGS__
#else
#define SWD_IF_SHPROF(...)
#endif
#ifdef SWD_TSPROF // absolute ticks of a unit: its start, the start of the iteration that committed it, the commit (scripts/ts_profile.py, gdg_timeline.py, ens_timeline.py)
#define SWD_IF_TSPROF(...) __VA_ARGS__
#else
#define SWD_IF_TSPROF(...)
#endif
#ifdef SWD_SELPROF // 100 MHz ticks inside select_vn / the cache rebuild, summed per unit in s.scal[20..27] (scripts/gdg_select_profile.py)
#define SWD_IF_SELPROF(...) __VA_ARGS__
#else
#define SWD_IF_SELPROF(...)
#endif
#ifdef SWD_GDGPROF // 100 MHz ticks per kind of work inside a tree walk: cache rebuilds, BP blocks, select_vn, branch starts, path metrics (scripts/gdg_phase_profile.py, ens_phase_profile.py)
#define SWD_IF_GDGPROF(...) __VA_ARGS__
#else
#define SWD_IF_GDGPROF(...)
#endif
#ifdef SWD_GDG_DEBUG // counters in the decoder's status array (words 1..), checksums of a unit's syndrome and result, commits per unit in statistics word 7 (scripts/gdg_debug.py)
#define SWD_IF_GDG_DEBUG(...) __VA_ARGS__
#define SWD_IF_NOT_GDG_DEBUG(...)
#else
#define SWD_IF_GDG_DEBUG(...)
#define SWD_IF_NOT_GDG_DEBUG(...) __VA_ARGS__
#endif
#ifdef SWD_GDG_CHECKS // invariant violations of the guessing decoders are reported in the status word (bits 8..) instead of followed; no script of its own
#define SWD_IF_GDG_CHECKS(...) __VA_ARGS__
#else
#define SWD_IF_GDG_CHECKS(...)
#endif
#ifdef SWD_RESIDENCY // workgroups of a launch resident at the same time, status words 4: now, 5: most, 6: with >= 1 unit (scripts/residency_check.py)
#define SWD_IF_RESIDENCY(...) __VA_ARGS__
#else
#define SWD_IF_RESIDENCY(...)
#endif
#ifdef SWD_BP4PROF // bp4_kernel: cycles (s_memtime) per region of a decode, summed over the units of a workgroup and printed by it; no script of its own
#define SWD_IF_BP4PROF(...) __VA_ARGS__
#else
#define SWD_IF_BP4PROF(...)
#endif

// the helpers of the sites that bracket many regions: each reads the local names of the function it is used in
#define GDG_COUNT(word, v) do { SWD_IF_GDG_DEBUG(atomicAdd(&dbg_status[word], (uint32_t)(v));) } while (0)
#define GDG_CHECK(cond, code) do { SWD_IF_GDG_CHECKS(if (!(cond)) atomicOr(chk_status, 1u << (8 + (code)));) } while (0)
#define SEL_T0() SWD_IF_SELPROF(long long sel_t_ = wall_clock64())
#define SEL_T(k) do { SWD_IF_SELPROF(const long long sel_n_ = wall_clock64(); if (threadIdx.x == 0) s.scal[20 + (k)] += (int)(sel_n_ - sel_t_); sel_t_ = sel_n_;) } while (0)
#define GPT0() SWD_IF_GDGPROF(long long gp_t_ = wall_clock64())
#define GPT(k) do { SWD_IF_GDGPROF(const long long gp_n_ = wall_clock64(); R.gp[k] += gp_n_ - gp_t_; gp_t_ = gp_n_;) } while (0)
#define BPT(x) SWD_IF_BPPROF(x = clock64())
#define BP4T(i) SWD_IF_BP4PROF({ const long long t_ = clock64(); q_[i] += t_ - q0_; q0_ = t_; })
