// Debug / A-B switches (include/nrs.h "Debug switches"): ONE table, a typed read behind every use, and the option handling of nrs_create.
// Plain C++17, no HIP and no context: host/ctx_check.cpp runs all of it under sanitizers (`make ctx_check`), and
// tests/test_switch_table_cpu.py holds the table, the header's comment block and the names the tests pass to nrs_debug_set together.
//
// A context takes the NRS_* variables of the environment ONCE, when it is created (plus NRS_DEBUG="NAME=VALUE,NAME2=VALUE2", names without
// the prefix), and is changed afterwards through nrs_debug_set only: the library never looks at the environment again -- a host application
// may call setenv at any time -- and a read on a launch path is an array index.  Entry points without a context (the host edge builders)
// read a process-wide snapshot taken on first use.  Nothing is cached across nrs_debug_set: a switch is read where it is used, so what is
// read per call changes per call and what is read when an engine is created changes with the next engine.
//
// Kinds (what the readers do, no more):
//   PRESENCE  on when set to anything, "0" included (NRS_NO_LDS=0 turns the LDS path OFF)
//   INTEGER   atoi / atol of the value: garbage reads as 0
//   REAL      atof of the value
// An INTEGER or REAL row has an is_set too: where the library has no fixed default the reader asks is_set first and computes its own.
// To add a switch: one row here, its name in the comment block of include/nrs.h and (optionally) in README.md; `make ctx_check` and
// tests/test_switch_table_cpu.py say what is missing.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>
#include "../../include/nrs.h"

namespace nrs {

enum SwitchKind { SW_PRESENCE, SW_INTEGER, SW_REAL };
constexpr bool HOST_PACK = true;     // (the row's mark "forces the host packer": nrs_engine_devpack.hpp builds a window on the device only when none is set)

// X(identifier, kind, default (0: none), group, forces the host packer, description); the name is "NRS_" + identifier
#define NRS_SWITCH_TABLE(X) \
    X(TIMING,               SW_PRESENCE, 0,       "measurement",   false,     "stage marks of engine_create, the a2 driver and the direct solver's set-up on stderr") \
    X(ND_DBG,               SW_PRESENCE, 0,       "measurement",   false,     "phase clocks of one direct solve through nrs_debug_nd_solve, per level") \
    X(ND_DBG2,              SW_PRESENCE, 0,       "measurement",   false,     "... per front") \
    X(PEEK_DEBUG,           SW_PRESENCE, 0,       "measurement",   false,     "gain ratios at the early-rejection looks") \
    X(POISON,               SW_PRESENCE, 0,       "checks",        false,     "fresh device allocations filled with NaN patterns") \
    X(CHECK_EVAL,           SW_PRESENCE, 0,       "checks",        false,     "every LM trial state evaluated twice and compared") \
    X(CHECK_FUSED,          SW_PRESENCE, 0,       "checks",        false,     "every single-launch PCG iteration run twice from a snapshot and compared") \
    X(CHECK_CHI,            SW_PRESENCE, 0,       "checks",        false,     "the carried chi2 against the one the next linearisation computes") \
    X(ND,                   SW_INTEGER,  0,       "direct solver", false,     "0: never, otherwise: whenever possible (overrides nrs_options.direct_solve)") \
    X(ND_MAX_ROWS,          SW_INTEGER,  8000,    "direct solver", false,     "free nodes up to which direct_solve = 0 takes the direct solver") \
    X(ND_NO_CACHE,          SW_PRESENCE, 0,       "direct solver", false,     "never reuse a symbolic plan") \
    X(ND_NO_COVER,          SW_PRESENCE, 0,       "direct solver", false,     "separators from the thinner side's boundary nodes, not the minimum vertex cover") \
    X(ND_CHAIN,             SW_PRESENCE, 0,       "direct solver", false,     "the top levels of the factorisation in one launch") \
    X(ND_LEVELS,            SW_PRESENCE, 0,       "direct solver", false,     "one launch per level whatever the slot was built for (read per call)") \
    X(ND_THREADS,           SW_INTEGER,  0,       "direct solver", false,     "256: factorisation levels on 256-thread workgroups") \
    X(ND_STEP32,            SW_INTEGER,  0,       "direct solver", false,     "0: the panel by 16-column steps") \
    X(ND_BACK_FLAGS,        SW_PRESENCE, 0,       "direct solver", false,     "back pass hand-over by flags, not by the polled values") \
    X(ND_LEAF,              SW_INTEGER,  0,       "direct solver", false,     "leaf size of the dissection (4 .. the built-in one)") \
    X(ND_NO_SPLIT,          SW_PRESENCE, 0,       "direct solver", false,     "crowded levels in one launch") \
    X(ND_PLAN_PAR,          SW_INTEGER,  0,       "direct solver", false,     "nodes from which the halves of a dissection go to threads of their own (0: never)") \
    X(SPEC_TRIALS,          SW_INTEGER,  2,       "LM trials",     false,     "shadow sets for the speculative trials of a run of rejections, 0..3 (read when an engine is created)") \
    X(SPEC_MAX_ROWS,        SW_INTEGER,  1 << 18, "LM trials",     false,     "rows up to which a BA window on the two-kernel PCG carves shadow sets") \
    X(SPEC_FIXED,           SW_INTEGER,  0,       "LM trials",     false,     "batches of n trials, not sized by the last run") \
    X(SPEC_FIRST,           SW_INTEGER,  0,       "LM trials",     false,     "n further trials behind every first trial of an iteration (a stress form)") \
    X(SPEC_NO_ABORT,        SW_PRESENCE, 0,       "LM trials",     false,     "discarded trials run to their end") \
    X(SPEC_DBG,             SW_PRESENCE, 0,       "LM trials",     false,     "host clocks of every batch on stderr") \
    X(NO_REARM,             SW_PRESENCE, 0,       "LM trials",     false,     "plain windows: the PCG's status words cleared by a fill per trial, not re-armed by k_finalize") \
    X(NO_LDS,               SW_PRESENCE, 0,       "PCG / packing", HOST_PACK, "operator and lineariser gather from global memory") \
    X(NO_FUSED,             SW_PRESENCE, 0,       "PCG / packing", HOST_PACK, "two-kernel PCG at any size") \
    X(FUSED_MAX_ROWS,       SW_INTEGER,  32768,   "PCG / packing", HOST_PACK, "rows from which the single-launch iteration hands over to the two-kernel PCG") \
    X(NO_COARSE,            SW_PRESENCE, 0,       "PCG / packing", false,     "no coarse level in the preconditioner") \
    X(COARSE_MIN_TILES,     SW_INTEGER,  48,      "PCG / packing", false,     "tiles from which the fused iteration takes the coarse level") \
    X(NO_ONE_XCD,           SW_PRESENCE, 0,       "PCG / packing", false,     "the fused iteration's grid not folded onto one XCD") \
    X(NO_ECD,               SW_PRESENCE, 0,       "PCG / packing", HOST_PACK, "no edge-chi2 carry on the two-kernel path") \
    X(HIER,                 SW_PRESENCE, 0,       "PCG / packing", HOST_PACK, "hierarchical reductions at any tile count") \
    X(NO_PLAIN,             SW_PRESENCE, 0,       "PCG / packing", HOST_PACK, "generic kernels on windows that qualify for the plain ones") \
    X(NO_H4,                SW_PRESENCE, 0,       "PCG / packing", false,     "8-byte damper headers where the compact ones would do") \
    X(RC,                   SW_INTEGER,  0,       "PCG / packing", false,     "0..3: record-cache form of the compact-header operator") \
    X(NT,                   SW_INTEGER,  0,       "PCG / packing", false,     "0|1: non-temporal accesses to the incidence streams (default: by size)") \
    X(DFORM,                SW_PRESENCE, 0,       "PCG / packing", HOST_PACK, "temporal-difference form of the dampers") \
    X(NO_EDGE_CHI,          SW_PRESENCE, 0,       "PCG / packing", HOST_PACK, "chi2 by a pass of its own, not from the edges' records") \
    X(SELL_T,               SW_INTEGER,  0,       "PCG / packing", HOST_PACK, "lanes per row of the sliced layout") \
    X(NO_MORTON,            SW_PRESENCE, 0,       "PCG / packing", false,     "rows in vertex order, not along the Morton curve") \
    X(NO_TILE_SORT,         SW_PRESENCE, 0,       "PCG / packing", false,     "tiles not sorted by halo size") \
    X(ONE_CLASS,            SW_PRESENCE, 0,       "PCG / packing", false,     "one halo class whatever the tiles' spread") \
    X(TILE_CUT_PCT,         SW_REAL,     0,       "PCG / packing", HOST_PACK, "force the halo classes' split at this percentile of the tiles") \
    X(HOST_PACK,            SW_PRESENCE, 0,       "PCG / packing", HOST_PACK, "BA windows built by the host packer") \
    X(HOST_THREADS,         SW_INTEGER,  0,       "PCG / packing", false,     "1..64 host threads of the set-up stages (<= 1: everything inline)") \
    X(HOST_THREADS_SMALL,   SW_INTEGER,  0,       "PCG / packing", false,     "1..8 host threads for single-frame problems of some size") \
    X(SKIN_OP_OWN_LAUNCH,   SW_PRESENCE, 0,       "PCG / packing", false,     "embedded window: k_skin_op in a launch of its own") \
    X(SKIN_ROWS_OWN_LAUNCH, SW_PRESENCE, 0,       "PCG / packing", false,     "embedded window: the observations' row pass in a launch of its own") \
    X(PCG_RTOL,             SW_REAL,     0,       "PCG / packing", false,     "overrides nrs_options.pcg_rtol when > 0 (experiments; read in nrs_create)") \
    X(SHARD_EMBWIN_DEVICE,  SW_PRESENCE, 0,       "PCG / packing", false,     "a rank builds its share of an embedded one-call window's lists on its device") \
    X(KFT_TWO_LAUNCHES,     SW_PRESENCE, 0,       "embedded BA",   false,     "a sweep step of the keyframe-block factorisation as two launches") \
    X(KFT_SCALAR_SWEEP,     SW_PRESENCE, 0,       "embedded BA",   false,     "the pivot block's sweep in the 4-pivot register form") \
    X(KFT_FOUR_WAVES,       SW_PRESENCE, 0,       "embedded BA",   false,     "panel workgroups without the four helper waves") \
    X(KFT_NO_RESIDUAL_TEST, SW_PRESENCE, 0,       "embedded BA",   false,     "M^-1 applied again after the first PCG step, not the step's residual tested") \
    X(SHARD_PACK_ALL,       SW_PRESENCE, 0,       "sharding",      HOST_PACK, "every rank packs the whole window") \
    X(SHARD_FULL_VECTORS,   SW_PRESENCE, 0,       "sharding",      false,     "a rank holds every row of the per-row arrays") \
    X(PO_MULTI_MIN,         SW_INTEGER,  32768,   "a1 / graph",    false,     "a1: points from which a frame takes the many-workgroup form") \
    X(PO_NO_CACHE,          SW_INTEGER,  0,       "a1 / graph",    false,     "a1, non-zero: the single workgroup reads its points from global memory") \
    X(PO_MULTI_GROUPS,      SW_INTEGER,  0,       "a1 / graph",    false,     "a1: at most g >= 1 workgroups in the many-workgroup form") \
    X(HOST_WALK,            SW_PRESENCE, 0,       "a1 / graph",    false,     "a2's neighbour walk on the host") \
    X(WALK_MAX_PASSES,      SW_INTEGER,  0,       "a1 / graph",    false,     "a lower limit on the walk's passes") \
    X(RG_NO_MIRROR,         SW_PRESENCE, 0,       "a1 / graph",    false,     "GetEdges over many rows reads the triangular state directly") \
    X(RG_MAX_CAP,           SW_INTEGER,  0,       "a1 / graph",    false,     "a lower limit on the GetEdges prefix a call may ask for") \
    X(STEREO_NO_MFMA,       SW_PRESENCE, 0,       "evaluation",    false,     "stereo pattern matcher: plain integer correlation") \
    X(FRONT_PER_EYE,        SW_PRESENCE, 0,       "front end",     false,     "nrs_front_process_stereo: grey and CLAHE issued per eye with the single-frame kernels, not as pair launches") \
    X(RECT_OWN_LAUNCH,      SW_PRESENCE, 0,       "front end",     false,     "nrs_front_process_stereo_raw: the remap into a rectified colour buffer, then the pair's grey kernel, not the fused launch") \
    X(RESIZE_OWN_LAUNCH,    SW_PRESENCE, 0,       "front end",     false,     "nrs_front_process_raw: the resize into a colour buffer, then the ordinary grey kernel, not the fused launch") \
    X(DBND_NO_TILE,         SW_PRESENCE, 0,       "initialisation", false,    "nrs_dbscan_nd / nrs_flow_tracks_cluster: a wave per point with candidates from global memory, not the LDS tiles") \
    X(LIN_DBG,              SW_PRESENCE, 0,       "probes",       false,     "make PROBES=1: phase clocks of one lineariser launch") \
    X(SPMV_DBG,             SW_PRESENCE, 0,       "probes",        false,     "make PROBES=1: phase clocks of one operator launch") \
    X(PCG_DBG,              SW_PRESENCE, 0,       "probes",        false,     "make PROBES=1: phase clocks of one fused iteration") \
    X(LIN_EXP,              SW_INTEGER,  0,       "probes",        false,     "make PROBES=1: lineariser removal experiments (wrong results on purpose)")

enum Switch : int {
#define X(id, kind, def, group, hp, desc) SW_##id,
    NRS_SWITCH_TABLE(X)
#undef X
    SW_COUNT
};
struct SwitchRow { Switch id; const char* name; SwitchKind kind; long def; const char* group; bool host_pack; const char* desc; };
constexpr SwitchRow SWITCHES[SW_COUNT] = {
#define X(id, kind, def, group, hp, desc) {SW_##id, "NRS_" #id, kind, def, group, hp, desc},
    NRS_SWITCH_TABLE(X)
#undef X
};
// the clamps every reader of a name shares (a clamp that depends on the site stays at the site)
constexpr int SPEC_TRIALS_MAX = 3;   // (= SPEC_MAX of nrs_engine_types.hpp, which asserts it)
inline int switch_clamp(Switch id, int v) {
    switch (id) {
        case SW_HOST_THREADS: return std::max(1, std::min(64, v));
        case SW_SPEC_TRIALS: return std::max(0, std::min(SPEC_TRIALS_MAX, v));
        case SW_RC: return v & 3;
        default: return v;
    }
}
inline int switch_by_name(const char* name) {                      // SW_COUNT: not in the table
    int i = 0;
    while (i < SW_COUNT && strcmp(SWITCHES[i].name, name) != 0) ++i;
    return i;
}

struct DebugOpts {
    struct Slot { bool on = false; std::string v; } slot[SW_COUNT];
    int n_host_pack = 0;                                           // set rows marked "forces the host packer"
    bool is_set(Switch id) const { return slot[id].on; }
    int int_of(Switch id) const { return slot[id].on ? switch_clamp(id, atoi(slot[id].v.c_str())) : (int)SWITCHES[id].def; }
    long long_of(Switch id) const { return slot[id].on ? atol(slot[id].v.c_str()) : SWITCHES[id].def; }
    double real_of(Switch id) const { return slot[id].on ? atof(slot[id].v.c_str()) : (double)SWITCHES[id].def; }
    bool forces_host_pack() const { return n_host_pack > 0; }
    void set(Switch id, const char* value) {                       // value NULL: unset
        Slot& s = slot[id];
        if (SWITCHES[id].host_pack) n_host_pack += (value ? 1 : 0) - (s.on ? 1 : 0);
        s.on = value != nullptr;
        s.v = value ? value : "";
    }
    // nrs_debug_set and the NRS_DEBUG list: a name that is not in the table has no effect
    void set_by_name(const char* name, const char* value) {
        const int i = switch_by_name(name);
        if (i < SW_COUNT) set((Switch)i, value);
    }
    // envp: "NAME=VALUE" strings, NULL-terminated (the process's `environ`; a made-up one in host/ctx_check.cpp)
    void load_environment(char** envp) {
        *this = DebugOpts();
        const char* list = nullptr;
        for (char** e = envp; e && *e; ++e) {
            if (strncmp(*e, "NRS_", 4) != 0) continue;
            const char* eq = strchr(*e, '=');
            if (!eq) continue;
            const std::string name(*e, eq - *e);
            if (name == "NRS_DEBUG") { list = eq + 1; continue; }
            set_by_name(name.c_str(), eq + 1);
        }
        for (const char* p = list; p && *p;) {                      // NRS_DEBUG="ND=0,NO_LDS=1": NAME=VALUE pairs, names without the NRS_ prefix; the list wins over a variable
            const char* end = strchr(p, ',');
            const std::string item = end ? std::string(p, end - p) : std::string(p);
            const size_t eq = item.find('=');
            if (!item.empty()) set_by_name(("NRS_" + (eq == std::string::npos ? item : item.substr(0, eq))).c_str(), eq == std::string::npos ? "1" : item.c_str() + eq + 1);
            p = end ? end + 1 : nullptr;
        }
    }
    static const DebugOpts& process();   // nrs_ctx.hip: the process-wide snapshot of `environ`, taken on first use
};

// nrs_create's option handling: the caller's struct may be shorter than this build's (an older header) -- its bytes only, defaults behind
// them -- or longer (the tail is ignored); in == NULL: all defaults.  NRS_ERR_INVALID for a struct_size shorter than the first field or
// beyond 4096 (an uninitialised word); *in is not written to.
inline int resolve_options(const nrs_options* in, const DebugOpts& dbg, nrs_options* out) {
    memset(out, 0, sizeof(*out));
    out->device = -1;
    if (in) {
        const size_t n = in->struct_size ? in->struct_size : offsetof(nrs_options, direct_solve);   // (0: the layout before struct_size was filled in)
        if (n < offsetof(nrs_options, pcg_rtol) || n > 4096) return NRS_ERR_INVALID;
        memcpy(out, in, std::min(n, sizeof(*out)));
        out->struct_size = (uint32_t)sizeof(*out);
    }
    if (out->direct_solve < 0 || out->direct_solve > 2) out->direct_solve = 0;
    if (out->embedded_solver < 0 || out->embedded_solver > 2) out->embedded_solver = 0;
    if (out->sharded_kft != 1) out->sharded_kft = 0;
    if (out->pcg_rtol <= 0) out->pcg_rtol = 1e-10;
    if (dbg.real_of(SW_PCG_RTOL) > 0) out->pcg_rtol = dbg.real_of(SW_PCG_RTOL);   // experiments only
    if (out->pcg_max_iters <= 0) out->pcg_max_iters = 2000;
    if (out->pcg_batch <= 0) out->pcg_batch = 8;
    return NRS_OK;
}

}  // namespace nrs
