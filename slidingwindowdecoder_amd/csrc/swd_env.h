// Every environment variable libswd_hip.so reads (test hooks and diagnostics; documented in include/swd.h and INTEGRATION.md), and the
// only getenv of csrc/.  A variable stays here only while a file under tests/ or scripts/ sets it (tests/test_env_hooks.py).
//   when   PROCESS: read at its first use, then cached for the process;  CREATE: read by every handle creation;  LAUNCH: by every launch
//   kind   PRESENT: on when set to anything (also "0");  NONZERO: on when set to anything but "0";  INT: atoi, the call site passes its
//          default and lower clamp;  STR: the text
#pragma once
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>

namespace swd { namespace env {
enum When { PROCESS, CREATE, LAUNCH };
enum Kind { PRESENT, NONZERO, INT, STR };
#define SWD_ENV_TABLE(X)                                                                                                                   \
    X(FORCE_HUGE, "SWD_FORCE_HUGE", CREATE, PRESENT, "osd_window, guessing decoders: the general form also where a variant fits (tests/test_gpu_huge*.py, sessions, rolling)") \
    X(NATURAL_LAYOUT, "SWD_NATURAL_LAYOUT", CREATE, PRESENT, "graphs keep the natural message-slot layout (tests/test_graph_layout.py, test_gpu_graph_layout.py)") \
    X(UNIFORM_DEPTH, "SWD_UNIFORM_DEPTH", CREATE, NONZERO, "plans keep the uniform node pass (tests/test_node_depth_host.py, test_gpu_node_depth.py, test_gpu_cache_image.py)") \
    X(OWIDE_RING, "SWD_OWIDE_RING", CREATE, INT, "ring entries of osd0_colsw, at least 4, so that batches close early (tests/test_gpu_big.py)") \
    X(GRID_PCT, "SWD_GRID_PCT", PROCESS, INT, "persistent grid in percent of the workgroup slots, at least 1 (tests/test_gpu_unit_reuse.py)") \
    X(GDG_SERIAL, "SWD_GDG_SERIAL", CREATE, PRESENT, "guessing decoders: serial tree walk, no work items (tests/test_gpu_gdg.py, tests/window_forms.py)") \
    X(GDG_STREAM_SERIAL_MIN, "SWD_GDG_STREAM_SERIAL_MIN", LAUNCH, INT, "shots from which overlapped batches take the serial walk, default 3072 (tests/test_gpu_gdg.py)") \
    X(GDG_PAR_MAX_SHOTS, "SWD_GDG_PAR_MAX_SHOTS", PROCESS, INT, "shots up to which a launch takes the work-item form, default 5120 (scripts/gdg_crossover.sh)") \
    X(GDG_INFLIGHT, "SWD_GDG_INFLIGHT", PROCESS, INT, "side branches of a tree in flight, default 4, at least 1 (scripts/gdg_sweep.sh)") \
    X(GDG_SHOTS_PCT, "SWD_GDG_SHOTS_PCT", PROCESS, INT, "shots admitted up front in percent of the grid, default 100 / 400, at least 1 (scripts/gdg_sweep.sh)") \
    X(ENS_TICKETS, "SWD_ENS_TICKETS", LAUNCH, PRESENT, "threaded ensemble: tickets instead of the work-item ring (tests/test_gpu_gdg.py)") \
    X(ENS_NO_TASKS, "SWD_ENS_NO_TASKS", LAUNCH, PRESENT, "threaded ensemble on the ring: no task items (tests/test_gpu_gdg.py)") \
    X(BP4_NT, "SWD_BP4_NT", CREATE, INT, "bp4_osd: threads of the BP kernel, a multiple of 64 in 64..1024 or ignored (tests/test_gpu_bp4_heavy.py)") \
    X(BP4_SKEW, "SWD_BP4_SKEW", PROCESS, STR, "bp4_osd: even | odd, waves of that parity sleep before the storing node passes of a split launch (tests/test_gpu_bp4.py)") \
    X(BP4_OVERLAPPED, "SWD_BP4_OVERLAPPED", PROCESS, PRESENT, "bp4_osd: every launch taken as one with another in flight (tests/fuzz_bp4.py)") \
    X(BP4_NOSPLIT, "SWD_BP4_NOSPLIT", CREATE, PRESENT, "bp4_osd: one thread per qubit also for small codes (tests/fuzz_bp4.py)") \
    X(BP4_NO_LAZY, "SWD_BP4_NO_LAZY", PROCESS, PRESENT, "bp4_osd: the fused node update only (tests/fuzz_bp4.py)") \
    X(BP4_GENERIC, "SWD_BP4_GENERIC", LAUNCH, PRESENT, "bp4_osd: the generic instantiation (tests/fuzz_bp4.py, scripts/bp4_heavy_rate.py)") \
    X(BP4_SPLIT_MAX, "SWD_BP4_SPLIT_MAX", CREATE, INT, "bp4_osd: two threads per qubit up to this 2 n, default 256, at most 512 (tests/fuzz_bp4.py)")
#define X(id, name, when, kind, doc) id,
enum Id { SWD_ENV_TABLE(X) COUNT };
#undef X
struct Entry { const char *name; When when; Kind kind; const char *doc; };
#define X(id, name, when, kind, doc) {name, when, kind, doc},
constexpr Entry kTable[COUNT] = {SWD_ENV_TABLE(X)};
#undef X

inline const char *str(Id id) { // NULL: not set
    if (kTable[id].when != PROCESS) return getenv(kTable[id].name);
    static std::once_flag once[COUNT];
    static std::string text[COUNT];
    static bool set[COUNT];
    std::call_once(once[id], [id] { if (const char *e = getenv(kTable[id].name)) { text[id] = e; set[id] = true; } });
    return set[id] ? text[id].c_str() : nullptr;
}
inline bool on(Id id) { const char *e = str(id); return e && (kTable[id].kind != NONZERO || strcmp(e, "0") != 0); }
inline int num(Id id, int dflt, int lo = INT_MIN) { const char *e = str(id); return e ? std::max(lo, atoi(e)) : dflt; }
}} // namespace swd::env
