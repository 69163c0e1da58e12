// knobs.h -- every environment variable the engine honours, written down ONCE: the record the values land in (Knobs), the accessors of the few
// variables that are read where they are used, and the table (one row per variable) that drives the parse at psgsdf_create and the "env",
// "ignored_dev_only" and "effective" objects of psgsdf_get_tuning.  include/psgsdf.h lists the variables with their meaning for the caller; a *
// there means at_use here.  Plain C++, no HIP header: tests/knobs_check.cpp compiles it on its own.
//
// Two kinds of variable:
//   at_create  parsed once by knobs_parse when a context is created; the value lives in psgsdf_ctx::knob and never changes behind the context's
//              back (psgsdf_set_frame_solver is the one call that writes a member afterwards)
//   at_use     read through its accessor below every time the code path runs (tests change PSGSDF_FM_ROWS between launches on a live context,
//              tools/first_contact.py PSGSDF_XR_MEM between contexts of one process); "env" still reports what was set at creation
// Adding a knob: one row in kKnobTable, one member of Knobs (or one accessor), one line in the comment block of include/psgsdf.h
// (tests/test_host_tools.py holds the three against each other).
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace psge {
typedef const char* (*KnobEnv)(const char*);      // the environment as the knobs see it: the engine passes process_env (getenv), a test its own table
inline const char* process_env(const char* name) { return getenv(name); }

// what the at_create variables resolved to, defaults included (state they PRODUCE -- xr_mem_kind, persist_off, img_compacted, num_cu as cut by the
// CU mask -- stays in the context)
struct Knobs {
    bool pcg_poll = true;                // PSGSDF_PCG_POLL=0: the PCG stop test drains the stream instead of watching the mapped mailbox
    bool speculate = true;               // PSGSDF_SPECULATE=0: always wait for the stop decision before the next iteration starts (round 2)
    bool speculate_mr = true;            // PSGSDF_SPECULATE_MR=0: no speculative start of the next iteration on multi-rank contexts (round 3's loop)
    bool fold_in_next = true;            // PSGSDF_FOLD_IN_NEXT=0: always a k_sum_parts launch
    bool fuse_albedo = true;             // PSGSDF_FUSE_ALBEDO=0: separate k_apply_albedo launch
    bool fuse_pcg_init = true;           // PSGSDF_FUSE_PCG_INIT=0: separate k_cgf_init launch
    bool pcg_persist = true;             // PSGSDF_PCG_PERSIST=0: always the per-pass kernels
    bool pcg_fuse_apply = true;          // PSGSDF_PCG_FUSE_APPLY=0: k_apply_dist behind it
    bool pcg_window = true;              // PSGSDF_PCG_WINDOW=0: the single-rank pipelined solve gathers per thread instead of reading an LDS window (pcg_solve.h k_cgp_solve<.., WIN>)
    int pcg_solve_rows = 0;              // PSGSDF_PCG_SOLVE_ROWS: rows per workgroup of the persistent solve on one rank (0: as many workgroups as CUs); tests shape the partition with it
    bool areg_device = true;             // PSGSDF_AREG_DEVICE=0: the regularised albedo solve driven by the host (two read-backs per CG iteration: what multi-rank contexts run)
    bool fm_solve = true;                // PSGSDF_FM_SOLVE=0: k_solve_light / k_solve_pose as kernels of their own behind the frame-major sweeps
    bool fm_solve_led = true;            // ... also the LED light vector (by the sweep's very last workgroup); PSGSDF_FM_SOLVE=2 keeps k_solve_light for it
    int frame_solve = 0;                 // PSGSDF_FRAME_SOLVE / psgsdf_set_frame_solver: 0 = LDL^T per frame in double (default), 1 = the reference's solver: ONE Eigen-style float Jacobi-PCG over the block-diagonal system of all frames (frame_solve.hip)
    bool xr_enable = true;               // PSGSDF_XR=0: multi-rank contexts always use the per-pass kernels + RCCL all-reduce (round 2)
    bool xf_enable = true;               // PSGSDF_XF=0: multi-rank frame rows through an RCCL all-reduce + solve kernels (round 3)
    bool xs_enable = true;               // PSGSDF_XS=0: multi-rank scalar read-backs staged in the mailbox shadow and all-reduced over RCCL (round 3)
    bool xh_enable = true;               // PSGSDF_XH=0: halo rows through RCCL send / recv (round 3)
    int xwait_spins = 1 << 24;           // polls of a wait inside a kernel for a peer's flag (PSGSDF_XWAIT_LOG2)
    bool img_compact = true;             // PSGSDF_IMG_COMPACT=0: float keyframes stay float even when every value is (float)byte / 255
    int xcd_map = 163;                   // PSGSDF_XCD_MAP: logical workgroup ids -- bit 0 frame-major sweeps XCD-contiguous, bit 1 k_sweep_albedo / k_energy / k_derive XCD-contiguous, bit 2 k_sweep_dist XCD-contiguous (off: 68 -> 76 us), bit 5 (32) k_sweep_dist heaviest block first (70 -> 62 us), bit 6 (64) albedo / energy heaviest first (no gain), bit 7 (128) the per-pass distance solve k_cgf_pass XCD-contiguous (round 6); PSGSDF_XCD_STRIPE=T: stripes of T ids instead of eighths
    bool ao_cut = true;                  // PSGSDF_AO_CUT=0: the rays of include/psgsdf_occlusion.h walk on past their radius (what the cut buys: tools/time_mesh.py; the same bits)
    long long compare_chunk = 1ll << 24; // PSGSDF_COMPARE_CHUNK: queries per launch of include/psgsdf_compare.h's search (1 .. 2^24; the same bits)
    long long query_chunk = 1ll << 30;   // PSGSDF_QUERY_CHUNK: queries per launch of include/psgsdf_query.h's kernels (a multiple of 64 up to 2^30; the same bits)
    int cu_mask_lo = -1, cu_mask_hi = -1;      // PSGSDF_CU_MASK=lo:hi: the context's stream only uses CUs [lo, hi) (two ranks sharing one GPU)
    // development build only (libpsgsdf_dev.so): fault injection, ablation, the round-2 race.  The product library leaves them at these defaults
    int pcg_ablate = 0;                  // PSGSDF_PCG_ABLATE: timing ablations of the persistent solve, bits 1 and 4 (wrong results; tools only)
    bool mbox_check = true;              // PSGSDF_MBOX_CHECK=0: take read-backs on the marker's / status word's say-so (round-2 behaviour; reproduces its flake)
    int fault_solve = 0;                 // PSGSDF_FAULT_SOLVE=n: fault injection into the n-th persistent solve of this context
    long long fault_halo = 0;            // PSGSDF_FAULT_HALO
};

// ---- the at_use variables: one accessor each, which holds the variable's range rule
inline int knob_fm_rows(KnobEnv env = process_env) {         // observations per thread of the frame-major sweeps, or 0: unset (>= 4: the partial-row buffer is sized for that; <= 64: fm_for_each_obs keeps one bit per observation of a thread)
    const char* e = env("PSGSDF_FM_ROWS"); const int v = e ? atoi(e) : 0; return v >= 4 && v <= 64 ? v : 0;
}
inline int knob_pcg_rows(KnobEnv env = process_env) {        // rows per thread of the per-pass distance solve: 1 (default) or 2
    const char* e = env("PSGSDF_PCG_ROWS"); const int v = e ? atoi(e) : 0; return v >= 1 && v <= 2 ? v : 1;
}
inline int knob_pcg_blocks(int max_blocks, KnobEnv env = process_env) {     // cap on the workgroups of a per-pass launch: 1 .. max_blocks (default)
    const char* e = env("PSGSDF_PCG_BLOCKS"); const int v = e ? atoi(e) : 0; return v > 0 && v <= max_blocks ? v : max_blocks;
}
inline bool knob_pcg_col16(KnobEnv env = process_env) {      // false: the 32-bit column table even where 16-bit deltas would reach
    const char* e = env("PSGSDF_PCG_COL16"); return !(e && atoi(e) == 0);
}
inline int knob_xr_mem(KnobEnv env = process_env) {          // memory kind pinned for the cross-rank hand-offs: 1 fine, 2 uncached, 3 coarse; 0: the probe chooses
    const char* e = env("PSGSDF_XR_MEM"); return !e ? 0 : !strcmp(e, "fine") ? 1 : !strcmp(e, "uncached") ? 2 : !strcmp(e, "coarse") ? 3 : 0;
}
inline double knob_wait_timeout_s(KnobEnv env = process_env) {      // bound of a host wait for something a kernel publishes (the engine evaluates it once per process)
    const char* e = env("PSGSDF_WAIT_TIMEOUT_S"); const double v = e ? atof(e) : 0.0; return v > 0.0 ? v : 120.0;
}
inline double knob_destroy_timeout_s(KnobEnv env = process_env) { const char* e = env("PSGSDF_DESTROY_TIMEOUT_S"); return e ? atof(e) : 15.0; }    // psgsdf_destroy's wait for the peers' mappings
inline double knob_socket_timeout_s(KnobEnv env = process_env) { const char* e = env("PSGSDF_SOCKET_TIMEOUT_S"); return e ? atof(e) : 120.0; }    // send / receive timeout of psgsdf_comm_init_sockets
inline const char* knob_solve_dump(KnobEnv env = process_env) { return env("PSGSDF_SOLVE_DUMP"); }      // file psgsdf_debug_time_pcg_solve dumps its per-workgroup times to, or null

// ---- the table.  Exactly ONE translation unit defines PSGSDF_KNOB_TABLE before including this header (api.hip; the stand-alone check): it is the
// one the Makefile compiles with and without -DPSGSDF_DEV, which is what decides below whether a dev_only row is honoured or reported as ignored, and
// the product library must hold the dev_only names once only (tests/test_abi.py).  Everyone else asks that unit (engine_internal.h knobs_effective_json).
#ifdef PSGSDF_KNOB_TABLE
enum KnobWhen { at_create, at_use };
enum KnobBuild { product, dev_only };
struct KnobIo {
    bool (*parse)(const char* e, Knobs& k);                                // the variable's text -> its member(s); false: refused (psgsdf_create returns PSGSDF_ERR_ARG)
    void (*report)(const Knobs& k, const char* key, std::string& o);       // its member(s) -> "effective"
};
struct KnobRow { const char* name; KnobWhen when; KnobBuild build; KnobIo io; const char* key; };      // key: under which "effective" reports it; null: not at all

inline void knob_put(std::string& o, const std::string& key, const std::string& json) { if (!o.empty()) o += ", "; o += "\"" + key + "\": " + json; }
template <auto M> void knob_put_int(const Knobs& k, const char* key, std::string& o) { knob_put(o, key, std::to_string((long long)(k.*M))); }
template <auto M> bool knob_flag(const char* e, Knobs& k) { k.*M = atoi(e) != 0; return true; }      // ("" and "abc" mean off)
template <auto M> bool knob_int(const char* e, Knobs& k) { k.*M = atoi(e); return true; }
template <auto M> bool knob_positive(const char* e, Knobs& k) { const int v = atoi(e); if (v > 0) k.*M = v; return true; }
template <auto M> bool knob_long(const char* e, Knobs& k) { k.*M = atoll(e); return true; }
template <auto M> constexpr KnobIo flag{knob_flag<M>, knob_put_int<M>};
template <auto M> constexpr KnobIo integer{knob_int<M>, knob_put_int<M>};
template <auto M> constexpr KnobIo positive{knob_positive<M>, knob_put_int<M>};
template <auto M> constexpr KnobIo long_integer{knob_long<M>, knob_put_int<M>};
constexpr KnobIo by_accessor{nullptr, nullptr};      // at_use: never parsed here
constexpr KnobIo fm_solve{                            // 0 off; 1 on, the LED light vector too; anything else on, k_solve_light kept for the LED vector
    [](const char* e, Knobs& k) { k.fm_solve = atoi(e) != 0; k.fm_solve_led = atoi(e) == 1; return true; },
    [](const Knobs& k, const char* key, std::string& o) { knob_put(o, key, std::to_string((int)k.fm_solve)); knob_put(o, std::string(key) + "_led", std::to_string((int)k.fm_solve_led)); }};
constexpr KnobIo frame_solve{
    [](const char* e, Knobs& k) { k.frame_solve = (!strcmp(e, "eigen") || !strcmp(e, "1")) ? 1 : 0; return true; },
    [](const Knobs& k, const char* key, std::string& o) { knob_put(o, key, k.frame_solve == 1 ? "\"eigen\"" : "\"ldlt\""); }};
constexpr KnobIo xcd_stripe{                          // on top of PSGSDF_XCD_MAP (its row comes first): bits 8 and up of xcd_map, which reports both
    [](const char* e, Knobs& k) { k.xcd_map = (k.xcd_map & 255) | (atoi(e) << 8); return true; }, nullptr};
constexpr KnobIo xwait_log2{
    [](const char* e, Knobs& k) { const int l = atoi(e); if (l >= 8 && l <= 30) k.xwait_spins = 1 << l; return true; },
    [](const Knobs& k, const char* key, std::string& o) { knob_put(o, key, std::to_string((int)lround(log2((double)k.xwait_spins)))); }};
constexpr KnobIo cu_mask{                             // "lo:hi", 0 <= lo < hi (hi <= the device's CUs: psgsdf_create, which knows the device)
    [](const char* e, Knobs& k) { int lo = 0, hi = 0; if (sscanf(e, "%d:%d", &lo, &hi) != 2 || lo < 0 || hi <= lo) return false; k.cu_mask_lo = lo; k.cu_mask_hi = hi; return true; },
    [](const Knobs& k, const char* key, std::string& o) { knob_put(o, key, "[" + std::to_string(k.cu_mask_lo) + ", " + std::to_string(k.cu_mask_hi) + "]"); }};
constexpr KnobIo compare_chunk{
    [](const char* e, Knobs& k) { k.compare_chunk = std::min(std::max(atoll(e), 1ll), 1ll << 24); return true; }, knob_put_int<&Knobs::compare_chunk>};
constexpr KnobIo query_chunk{                         // a whole decimal number, a multiple of 64 up to 2^30 (no wavefront may straddle two launches); anything else is refused, never rounded
    [](const char* e, Knobs& k) { char* end = nullptr; const long long v = strtoll(e, &end, 10); if (end == e || *end || v < 64 || v > (1ll << 30) || v % 64) return false; k.query_chunk = v; return true; },
    knob_put_int<&Knobs::query_chunk>};
constexpr KnobIo pcg_ablate{[](const char* e, Knobs& k) { k.pcg_ablate = atoi(e) & 5; return true; }, knob_put_int<&Knobs::pcg_ablate>};

static constexpr KnobRow kKnobTable[] = {
    // name                        read        build     parse and report                        key in "effective"
    {"PSGSDF_PCG_POLL",            at_create,  product,  flag<&Knobs::pcg_poll>,                 "pcg_poll"},
    {"PSGSDF_SPECULATE",           at_create,  product,  flag<&Knobs::speculate>,                "speculate"},
    {"PSGSDF_SPECULATE_MR",        at_create,  product,  flag<&Knobs::speculate_mr>,             "speculate_mr"},
    {"PSGSDF_FOLD_IN_NEXT",        at_create,  product,  flag<&Knobs::fold_in_next>,             "fold_in_next"},
    {"PSGSDF_FUSE_ALBEDO",         at_create,  product,  flag<&Knobs::fuse_albedo>,              "fuse_albedo"},
    {"PSGSDF_FUSE_PCG_INIT",       at_create,  product,  flag<&Knobs::fuse_pcg_init>,            "fuse_pcg_init"},
    {"PSGSDF_PCG_PERSIST",         at_create,  product,  flag<&Knobs::pcg_persist>,              "pcg_persist"},
    {"PSGSDF_PCG_FUSE_APPLY",      at_create,  product,  flag<&Knobs::pcg_fuse_apply>,           "pcg_fuse_apply"},
    {"PSGSDF_PCG_WINDOW",          at_create,  product,  flag<&Knobs::pcg_window>,               "pcg_window"},
    {"PSGSDF_PCG_SOLVE_ROWS",      at_create,  product,  positive<&Knobs::pcg_solve_rows>,       "pcg_solve_rows"},
    {"PSGSDF_PCG_COL16",           at_use,     product,  by_accessor,                            nullptr},
    {"PSGSDF_PCG_ROWS",            at_use,     product,  by_accessor,                            nullptr},
    {"PSGSDF_PCG_BLOCKS",          at_use,     product,  by_accessor,                            nullptr},
    {"PSGSDF_FM_SOLVE",            at_create,  product,  fm_solve,                               "fm_solve"},
    {"PSGSDF_FRAME_SOLVE",         at_create,  product,  frame_solve,                            "frame_solve"},
    {"PSGSDF_FM_ROWS",             at_use,     product,  by_accessor,                            nullptr},
    {"PSGSDF_IMG_COMPACT",         at_create,  product,  flag<&Knobs::img_compact>,              "img_compact"},
    {"PSGSDF_XCD_MAP",             at_create,  product,  integer<&Knobs::xcd_map>,               "xcd_map"},
    {"PSGSDF_XCD_STRIPE",          at_create,  product,  xcd_stripe,                             nullptr},
    {"PSGSDF_AREG_DEVICE",         at_create,  product,  flag<&Knobs::areg_device>,              "areg_device"},
    {"PSGSDF_XR",                  at_create,  product,  flag<&Knobs::xr_enable>,                "xr"},
    {"PSGSDF_XF",                  at_create,  product,  flag<&Knobs::xf_enable>,                "xf"},
    {"PSGSDF_XS",                  at_create,  product,  flag<&Knobs::xs_enable>,                "xs"},
    {"PSGSDF_XH",                  at_create,  product,  flag<&Knobs::xh_enable>,                "xh"},
    {"PSGSDF_XR_MEM",              at_use,     product,  by_accessor,                            nullptr},
    {"PSGSDF_XWAIT_LOG2",          at_create,  product,  xwait_log2,                             "xwait_log2"},
    {"PSGSDF_CU_MASK",             at_create,  product,  cu_mask,                                "cu_mask"},
    {"PSGSDF_WAIT_TIMEOUT_S",      at_use,     product,  by_accessor,                            nullptr},
    {"PSGSDF_DESTROY_TIMEOUT_S",   at_use,     product,  by_accessor,                            nullptr},
    {"PSGSDF_SOCKET_TIMEOUT_S",    at_use,     product,  by_accessor,                            nullptr},
    {"PSGSDF_SOLVE_DUMP",          at_use,     product,  by_accessor,                            nullptr},
    {"PSGSDF_AO_CUT",              at_create,  product,  flag<&Knobs::ao_cut>,                   "ao_cut"},
    {"PSGSDF_COMPARE_CHUNK",       at_create,  product,  compare_chunk,                          "compare_chunk"},
    {"PSGSDF_QUERY_CHUNK",         at_create,  product,  query_chunk,                            "query_chunk"},
    // fault injection / ablation / the round-2 race: they make results WRONG on purpose and exist in the development build only
    {"PSGSDF_PCG_ABLATE",          at_create,  dev_only, pcg_ablate,                             "pcg_ablate"},
    {"PSGSDF_FAULT_SOLVE",         at_create,  dev_only, integer<&Knobs::fault_solve>,           "fault_solve"},
    {"PSGSDF_FAULT_HALO",          at_create,  dev_only, long_integer<&Knobs::fault_halo>,       "fault_halo"},
    {"PSGSDF_MBOX_CHECK",          at_create,  dev_only, flag<&Knobs::mbox_check>,               "mbox_check"},
};

// The environment -> k, in table order.  `set` gets every variable of the table that is set (verbatim: "env"); a dev_only one lands there and takes
// effect only in a -DPSGSDF_DEV build, otherwise in `ignored` ("ignored_dev_only": set, but this build does not know it -- reported, never silently
// honoured).  false: a variable holds what its rule refuses.
#ifdef PSGSDF_DEV
constexpr bool kKnobsDevBuild = true;
#else
constexpr bool kKnobsDevBuild = false;
#endif
typedef std::vector<std::pair<std::string, std::string>> KnobList;
inline bool knobs_parse(KnobEnv env, Knobs& k, KnobList& set, KnobList& ignored) {
    for (const KnobRow& r : kKnobTable) {
        const char* e = env(r.name);
        if (!e) continue;
        if (r.build == dev_only && !kKnobsDevBuild) { ignored.emplace_back(r.name, e); continue; }
        if (r.when == at_create && !r.io.parse(e, k)) return false;
        set.emplace_back(r.name, e);
    }
    return true;
}
// the knobs' members of "effective": `"key": value, ...` without braces
inline std::string knobs_effective(const Knobs& k) {
    std::string o;
    for (const KnobRow& r : kKnobTable) if (r.key) r.io.report(k, r.key, o);
    return o;
}
#endif  // PSGSDF_KNOB_TABLE
}  // namespace psge
