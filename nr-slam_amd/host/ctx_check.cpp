// Stand-alone check of the context's host logic (csrc/nrs_switches.hpp) for a sanitizer build: `make ctx_check && ./ctx_check`.
// No HIP, no library.  `./ctx_check --list` prints the table, "name kind group" per row (tests/test_switch_table_cpu.py reads it).
//   table        names unique, "NRS_" + capitals / digits / underscores, identifiers dense and in row order, a group and a description in
//                every row, the rows that force the host packer against the twelve names written out
//   environment  made-up environments: foreign variables, a variable without '=', and NRS_DEBUG with empty items, a trailing comma, an item
//                without '=' (-> "1"), NAME= (set, empty), a name given both ways (the list wins), an unknown name; then set, change and
//                unset of every row by name, the path of nrs_debug_set
//   kinds        presence "0" is on, integer "abc" reads 0, the defaults when unset, the shared clamps at their edges
//   options      struct_size 0 / 7 / 4097 / this build's / larger, every solver field out of range, the pcg defaults and the NRS_PCG_RTOL
//                override; the input is not written to
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>
#include "../csrc/nrs_switches.hpp"

using namespace nrs;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "ctx_check: %s:%d: %s\n", __FILE__, __LINE__, #x); std::abort(); } } while (0)

static const char* kind_name(SwitchKind k) { return k == SW_PRESENCE ? "presence" : k == SW_INTEGER ? "integer" : "real"; }

static DebugOpts loaded(std::vector<std::string> vars) {
    std::vector<char*> envp;
    for (std::string& v : vars) envp.push_back(&v[0]);
    envp.push_back(nullptr);
    DebugOpts d;
    d.load_environment(envp.data());
    return d;
}
static int n_set(const DebugOpts& d) { int n = 0; for (int i = 0; i < SW_COUNT; ++i) n += d.is_set((Switch)i); return n; }

static void check_table() {
    std::set<std::string> names, host_pack;
    for (int i = 0; i < SW_COUNT; ++i) {
        const SwitchRow& r = SWITCHES[i];
        CHECK(r.id == i);
        CHECK(strncmp(r.name, "NRS_", 4) == 0 && r.name[4]);
        for (const char* p = r.name; *p; ++p) CHECK((*p >= 'A' && *p <= 'Z') || (*p >= '0' && *p <= '9') || *p == '_');
        CHECK(names.insert(r.name).second);
        CHECK(r.group && r.group[0] && r.desc && r.desc[0]);
        CHECK(r.kind != SW_PRESENCE || r.def == 0);
        CHECK(switch_by_name(r.name) == i);
        if (r.host_pack) host_pack.insert(r.name);
    }
    CHECK(!names.count("NRS_DEBUG"));                              // the list variable is no row
    CHECK(switch_by_name("NRS_DEBUG") == SW_COUNT && switch_by_name("NRS_NO_LDSS") == SW_COUNT && switch_by_name("NRS_") == SW_COUNT);
    const std::set<std::string> want = {"NRS_HOST_PACK", "NRS_NO_PLAIN", "NRS_NO_LDS", "NRS_DFORM", "NRS_NO_EDGE_CHI", "NRS_NO_FUSED", "NRS_SELL_T",
                                        "NRS_FUSED_MAX_ROWS", "NRS_TILE_CUT_PCT", "NRS_HIER", "NRS_NO_ECD", "NRS_SHARD_PACK_ALL"};
    CHECK(host_pack == want);
    // identifiers against the names written out: two rows of the same kind swapped in the table show here
    CHECK(!strcmp(SWITCHES[SW_NO_LDS].name, "NRS_NO_LDS") && !strcmp(SWITCHES[SW_NO_FUSED].name, "NRS_NO_FUSED") && !strcmp(SWITCHES[SW_ND].name, "NRS_ND"));
    CHECK(!strcmp(SWITCHES[SW_HOST_THREADS].name, "NRS_HOST_THREADS") && !strcmp(SWITCHES[SW_RC].name, "NRS_RC") && !strcmp(SWITCHES[SW_SPEC_TRIALS].name, "NRS_SPEC_TRIALS"));
    CHECK(!strcmp(SWITCHES[SW_PCG_RTOL].name, "NRS_PCG_RTOL") && !strcmp(SWITCHES[SW_LIN_EXP].name, "NRS_LIN_EXP") && !strcmp(SWITCHES[SW_TIMING].name, "NRS_TIMING"));
}

static void check_environment() {
    CHECK(n_set(loaded({})) == 0);
    { DebugOpts d; d.load_environment(nullptr); CHECK(n_set(d) == 0); }
    // foreign variables, a variable without '=', a name that only starts like a row's
    DebugOpts d = loaded({"PATH=/bin", "NRS=1", "XNRS_NO_LDS=1", "NRS_NO_LDS", "NRS_NO_LDSS=1", "NRS_NO_FUSED=0", "HOME=NRS_HIER=1"});
    CHECK(n_set(d) == 1 && d.is_set(SW_NO_FUSED) && !d.is_set(SW_NO_LDS) && !d.is_set(SW_HIER));
    // the list: empty items, a trailing comma, an item without '=', NAME=, the list over the variable (whichever comes first), an unknown name
    d = loaded({"NRS_ND=1", "NRS_DEBUG=,,NO_LDS,,ND=0,SELL_T=,NOT_A_SWITCH=3,RC=2,", "NRS_RC=1", "NRS_HIER=x"});
    CHECK(n_set(d) == 5);
    CHECK(d.is_set(SW_NO_LDS) && d.slot[SW_NO_LDS].v == "1");
    CHECK(d.is_set(SW_ND) && d.int_of(SW_ND) == 0);
    CHECK(d.is_set(SW_SELL_T) && d.slot[SW_SELL_T].v.empty() && d.int_of(SW_SELL_T) == 0);
    CHECK(d.int_of(SW_RC) == 2 && d.is_set(SW_HIER));
    CHECK(d.forces_host_pack());
    d = loaded({"NRS_DEBUG="});
    CHECK(n_set(d) == 0 && !d.forces_host_pack());
    d = loaded({"NRS_DEBUG=TIMING"});
    CHECK(n_set(d) == 1 && d.is_set(SW_TIMING) && !d.forces_host_pack());
    // a second load forgets the first
    { DebugOpts e = loaded({"NRS_HIER=1"}); std::string v = "NRS_TIMING=1"; char* envp[] = {&v[0], nullptr}; e.load_environment(envp); CHECK(n_set(e) == 1 && e.is_set(SW_TIMING) && !e.forces_host_pack()); }
    // set, change, unset of every row by name (nrs_debug_set); an unknown name does nothing
    DebugOpts s;
    for (int i = 0; i < SW_COUNT; ++i) {
        const Switch id = (Switch)i;
        s.set_by_name(SWITCHES[i].name, "5");
        CHECK(n_set(s) == 1 && s.is_set(id) && s.slot[i].v == "5" && s.forces_host_pack() == SWITCHES[i].host_pack);
        s.set_by_name(SWITCHES[i].name, "6");
        CHECK(n_set(s) == 1 && s.slot[i].v == "6" && s.forces_host_pack() == SWITCHES[i].host_pack);
        s.set_by_name("NRS_NOT_A_SWITCH", "1");
        CHECK(n_set(s) == 1);
        s.set_by_name(SWITCHES[i].name, nullptr);
        CHECK(n_set(s) == 0 && !s.forces_host_pack() && s.slot[i].v.empty());
        s.set_by_name(SWITCHES[i].name, nullptr);                   // (unset twice)
        CHECK(n_set(s) == 0 && !s.forces_host_pack());
    }
    // two host-packer rows set, one unset: still forced
    s.set(SW_NO_LDS, "1"); s.set(SW_HIER, "1"); s.set(SW_NO_LDS, nullptr);
    CHECK(s.forces_host_pack());
    s.set(SW_HIER, nullptr);
    CHECK(!s.forces_host_pack());
}

static void check_kinds() {
    DebugOpts d;
    // the defaults, each written once in the table
    CHECK(d.int_of(SW_FUSED_MAX_ROWS) == 32768 && d.int_of(SW_ND_MAX_ROWS) == 8000 && d.int_of(SW_COARSE_MIN_TILES) == 48 && d.int_of(SW_PO_MULTI_MIN) == 32768);
    CHECK(d.long_of(SW_SPEC_MAX_ROWS) == (1L << 18) && d.int_of(SW_SPEC_TRIALS) == 2 && d.int_of(SW_RC) == 0 && d.int_of(SW_SPEC_FIRST) == 0);
    CHECK(d.int_of(SW_PO_NO_CACHE) == 0 && d.int_of(SW_SELL_T) == 0 && d.real_of(SW_PCG_RTOL) == 0.0 && d.real_of(SW_TILE_CUT_PCT) == 0.0);
    for (int i = 0; i < SW_COUNT; ++i) {
        const Switch id = (Switch)i;
        CHECK(!d.is_set(id) && d.int_of(id) == (int)SWITCHES[i].def && d.long_of(id) == SWITCHES[i].def && d.real_of(id) == (double)SWITCHES[i].def);
        d.set(id, "0");                                            // presence: on when set to anything
        CHECK(d.is_set(id));
        if (id != SW_HOST_THREADS) CHECK(d.int_of(id) == 0);
        CHECK(d.real_of(id) == 0.0);
        d.set(id, "abc");                                          // garbage reads as 0
        CHECK(d.is_set(id) && d.long_of(id) == 0 && d.real_of(id) == 0.0);
        d.set(id, nullptr);
        CHECK(d.int_of(id) == (int)SWITCHES[i].def);               // ... and the default comes back
    }
    d.set(SW_FUSED_MAX_ROWS, "1000"); CHECK(d.int_of(SW_FUSED_MAX_ROWS) == 1000);
    d.set(SW_SPEC_MAX_ROWS, "4294967296"); CHECK(d.long_of(SW_SPEC_MAX_ROWS) == 4294967296L);
    d.set(SW_TILE_CUT_PCT, "97.5"); CHECK(d.real_of(SW_TILE_CUT_PCT) == 97.5);
    d.set(SW_ND, "0"); CHECK(d.is_set(SW_ND) && d.int_of(SW_ND) == 0);
    d.set(SW_ND_LEAF, " 12x"); CHECK(d.int_of(SW_ND_LEAF) == 12);
    // the shared clamps at their edges
    const struct { Switch id; const char* v; int want; } clamp[] = {
        {SW_HOST_THREADS, "0", 1}, {SW_HOST_THREADS, "-3", 1}, {SW_HOST_THREADS, "1", 1}, {SW_HOST_THREADS, "64", 64}, {SW_HOST_THREADS, "65", 64},
        {SW_HOST_THREADS, "1000", 64}, {SW_HOST_THREADS, "abc", 1}, {SW_SPEC_TRIALS, "-1", 0}, {SW_SPEC_TRIALS, "0", 0}, {SW_SPEC_TRIALS, "3", 3},
        {SW_SPEC_TRIALS, "4", 3}, {SW_RC, "7", 3}, {SW_RC, "4", 0}, {SW_RC, "2", 2}, {SW_RC, "-1", 3}, {SW_ND_MAX_ROWS, "-5", -5}};
    for (const auto& q : clamp) { d.set(q.id, q.v); CHECK(d.int_of(q.id) == q.want); }
}

static void check_options() {
    const DebugOpts none;
    nrs_options out;
    CHECK(resolve_options(nullptr, none, &out) == NRS_OK);
    CHECK(out.device == -1 && out.pcg_rtol == 1e-10 && out.pcg_max_iters == 2000 && out.pcg_batch == 8 && out.profile == 0 && out.exact_trials == 0 &&
          out.direct_solve == 0 && out.embedded_solver == 0 && out.sharded_kft == 0);
    nrs_options in;
    memset(&in, 0, sizeof(in));
    in.device = 3; in.pcg_rtol = 1e-6; in.pcg_max_iters = 77; in.pcg_batch = 4; in.profile = 1; in.exact_trials = 1; in.direct_solve = 2; in.embedded_solver = 1; in.sharded_kft = 1;
    auto run = [&](uint32_t struct_size, const DebugOpts& dbg = DebugOpts()) {
        in.struct_size = struct_size;
        const nrs_options before = in;
        memset(&out, 0xAB, sizeof(out));
        const int rc = resolve_options(&in, dbg, &out);
        CHECK(memcmp(&before, &in, sizeof(in)) == 0);               // the input is not written to
        return rc;
    };
    // this build's size: everything taken
    CHECK(run(sizeof(in)) == NRS_OK);
    CHECK(out.device == 3 && out.struct_size == sizeof(out) && out.pcg_rtol == 1e-6 && out.pcg_max_iters == 77 && out.pcg_batch == 4 && out.profile == 1 &&
          out.exact_trials == 1 && out.direct_solve == 2 && out.embedded_solver == 1 && out.sharded_kft == 1);
    // 0: the layout that ends before direct_solve -- its last field taken, the first behind it not
    CHECK(run(0) == NRS_OK);
    CHECK(out.device == 3 && out.struct_size == sizeof(out) && out.pcg_batch == 4 && out.exact_trials == 1 && out.direct_solve == 0 && out.embedded_solver == 0 && out.sharded_kft == 0);
    // every field boundary: the fields that lie wholly inside the prefix are the caller's, the rest defaults
    const size_t ends[] = {offsetof(nrs_options, pcg_rtol), offsetof(nrs_options, pcg_max_iters), offsetof(nrs_options, pcg_batch), offsetof(nrs_options, profile),
                           offsetof(nrs_options, exact_trials), offsetof(nrs_options, direct_solve), offsetof(nrs_options, embedded_solver),
                           offsetof(nrs_options, sharded_kft), sizeof(nrs_options)};
    for (size_t n : ends) {
        CHECK(run((uint32_t)n) == NRS_OK);
        CHECK(out.device == 3);
        CHECK(out.pcg_rtol == (n > offsetof(nrs_options, pcg_rtol) ? 1e-6 : 1e-10));
        CHECK(out.pcg_max_iters == (n > offsetof(nrs_options, pcg_max_iters) ? 77 : 2000));
        CHECK(out.pcg_batch == (n > offsetof(nrs_options, pcg_batch) ? 4 : 8));
        CHECK(out.profile == (n > offsetof(nrs_options, profile) ? 1 : 0));
        CHECK(out.exact_trials == (n > offsetof(nrs_options, exact_trials) ? 1 : 0));
        CHECK(out.direct_solve == (n > offsetof(nrs_options, direct_solve) ? 2 : 0));
        CHECK(out.embedded_solver == (n > offsetof(nrs_options, embedded_solver) ? 1 : 0));
        CHECK(out.sharded_kft == (n > offsetof(nrs_options, sharded_kft) ? 1 : 0));
    }
    // the bounds
    CHECK(run((uint32_t)offsetof(nrs_options, pcg_rtol) - 1) == NRS_ERR_INVALID);
    CHECK(run(1) == NRS_ERR_INVALID && run(4097) == NRS_ERR_INVALID && run(0xFFFFFFFFu) == NRS_ERR_INVALID);
    // larger than this build's: the tail is ignored (and not read: the sanitizer sees an exact-size object)
    CHECK(run(sizeof(in) + 8) == NRS_OK && out.sharded_kft == 1 && out.struct_size == sizeof(out));
    CHECK(run(4096) == NRS_OK && out.device == 3 && out.embedded_solver == 1);
    // out-of-range solver fields
    for (int v : {-1, 3, 1 << 30}) {
        nrs_options keep = in;
        in.direct_solve = v; CHECK(run(sizeof(in)) == NRS_OK && out.direct_solve == 0 && out.embedded_solver == 1); in = keep;
        in.embedded_solver = v; CHECK(run(sizeof(in)) == NRS_OK && out.embedded_solver == 0 && out.direct_solve == 2); in = keep;
        in.sharded_kft = v; CHECK(run(sizeof(in)) == NRS_OK && out.sharded_kft == 0); in = keep;
    }
    { nrs_options keep = in; in.sharded_kft = 2; CHECK(run(sizeof(in)) == NRS_OK && out.sharded_kft == 0); in.sharded_kft = 0; CHECK(run(sizeof(in)) == NRS_OK && out.sharded_kft == 0);
      in.direct_solve = 0; in.embedded_solver = 2; CHECK(run(sizeof(in)) == NRS_OK && out.direct_solve == 0 && out.embedded_solver == 2); in = keep; }
    // pcg defaults, then the override: after the default, only when > 0
    { nrs_options keep = in; in.pcg_rtol = 0; in.pcg_max_iters = 0; in.pcg_batch = -1;
      CHECK(run(sizeof(in)) == NRS_OK && out.pcg_rtol == 1e-10 && out.pcg_max_iters == 2000 && out.pcg_batch == 8);
      in.pcg_rtol = -1; CHECK(run(sizeof(in)) == NRS_OK && out.pcg_rtol == 1e-10);
      DebugOpts o; o.set(SW_PCG_RTOL, "1e-4");
      CHECK(run(sizeof(in), o) == NRS_OK && out.pcg_rtol == 1e-4);
      in = keep; CHECK(run(sizeof(in), o) == NRS_OK && out.pcg_rtol == 1e-4);
      o.set(SW_PCG_RTOL, "0"); CHECK(run(sizeof(in), o) == NRS_OK && out.pcg_rtol == 1e-6);
      o.set(SW_PCG_RTOL, "-2"); CHECK(run(sizeof(in), o) == NRS_OK && out.pcg_rtol == 1e-6);
      o.set(SW_PCG_RTOL, "abc"); CHECK(run(sizeof(in), o) == NRS_OK && out.pcg_rtol == 1e-6);
      CHECK(resolve_options(nullptr, o, &out) == NRS_OK && out.pcg_rtol == 1e-10); }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--list")) {
        for (const SwitchRow& r : SWITCHES) std::printf("%s %s %s\n", r.name, kind_name(r.kind), r.group);
        return 0;
    }
    check_table();
    check_environment();
    check_kinds();
    check_options();
    std::printf("ctx_check OK: %d switches (names, identifiers, groups, the host packer's twelve), made-up environments and NRS_DEBUG lists, set / change / "
                "unset of every row by name, the three kinds with their defaults and shared clamps, nrs_create's option handling at every field boundary\n", (int)SW_COUNT);
    return 0;
}
