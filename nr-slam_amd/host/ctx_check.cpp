// Stand-alone check of the context's host logic (csrc/nrs_switches.hpp, csrc/nrs_own.hpp) for a sanitizer build: `make ctx_check && ./ctx_check`.
// No HIP, no library.  `./ctx_check --list` prints the table, "name kind group" per row (tests/test_switch_table_cpu.py reads it).
//   table        names unique, "NRS_" + capitals / digits / underscores, identifiers dense and in row order, a group and a description in
//                every row, the rows that force the host packer against the twelve names written out
//   environment  made-up environments: foreign variables, a variable without '=', and NRS_DEBUG with empty items, a trailing comma, an item
//                without '=' (-> "1"), NAME= (set, empty), a name given both ways (the list wins), an unknown name; then set, change and
//                unset of every row by name, the path of nrs_debug_set
//   kinds        presence "0" is on, integer "abc" reads 0, the defaults when unset, the shared clamps at their edges
//   options      struct_size 0 / 7 / 4097 / this build's / larger, every solver field out of range, the pcg defaults and the NRS_PCG_RTOL
//                override; the input is not written to
//   owners       csrc/nrs_own.hpp against counting versions of the four free functions (the library's are in nrs_ctx.hip): a new
//                owner is empty; reset and the destructor free once each and an empty one frees nothing; move construction and move
//                assignment free the old target once and leave the source empty; self-move; a std::vector<DevBuf> that reallocates frees
//                nothing until it is cleared; the growth rule at 0, 1, 1023 and 1 << 32; stream and event owners destroy once; a
//                struct ordered like nrs_ctx frees its buffers before it destroys its stream
// Seeded faults, each tried once in a scratch copy; each one aborts check_owners at the CHECK named:
//   ~DevBuf() without reset()                            "freed(A) == 2 ..." behind the first scope
//   the move constructor leaves the source set           "!a.p && !a.cap && b.p == A ..."
//   the move assignment without its reset()              "freed(B) == 1 && freed(A) == 0 ..."
//   the move assignment without `this != &o`             the self-move: "a.p == A && a.cap == 64 ..."
//   reset() that leaves cap                              "!a.p && !a.cap && freed(A) == 1"
//   PinBuf::reset calling dev_free                       "... order() == std::string(2, kind)"
//   grown_bytes without its 256                          "grown_bytes(0) == 256 ..."
//   CtxLike's stream declared behind its buffers         "order() == \"pddes\"" (the stream goes first)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "../csrc/nrs_own.hpp"
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

// ---- the owners: counting versions of the four free functions; every release is logged in order
static std::vector<std::pair<char, const void*>> free_log;         // ('d' | 'p' | 's' | 'e', what)
namespace nrs {
void dev_free(void* p) noexcept { if (p) free_log.push_back({'d', p}); }
void pin_free(void* p) noexcept { if (p) free_log.push_back({'p', p}); }
void stream_destroy(ihipStream_t* s) noexcept { if (s) free_log.push_back({'s', s}); }
void event_destroy(ihipEvent_t* e) noexcept { if (e) free_log.push_back({'e', e}); }
}
static int freed(const void* p) { int n = 0; for (const auto& f : free_log) n += f.second == p; return n; }
static std::string order() { std::string s; for (const auto& f : free_log) s += f.first; return s; }

template <class Buf>
static void check_buffer_owner(char kind) {
    static_assert(!std::is_copy_constructible_v<Buf> && !std::is_copy_assignable_v<Buf>, "an owner is move-only");
    static_assert(std::is_nothrow_move_constructible_v<Buf> && std::is_nothrow_move_assignable_v<Buf>, "a vector of owners moves them when it grows");
    char mem[8];
    void *A = mem, *B = mem + 1, *C = mem + 2;
    free_log.clear();
    { Buf a; CHECK(!a.p && !a.cap && a.template as<int>() == nullptr); a.reset(); }
    CHECK(free_log.empty());                                       // an empty owner frees nothing, neither by reset nor when it goes
    {
        Buf a; a.p = A; a.cap = 64;
        CHECK(a.template as<char>() == mem);
        a.reset();
        CHECK(!a.p && !a.cap && freed(A) == 1);
        a.reset();
        CHECK(freed(A) == 1);
        a.p = A; a.cap = 64;
    }
    CHECK(freed(A) == 2 && free_log.size() == 2 && order() == std::string(2, kind));   // (once by reset, once by the destructor)
    free_log.clear();
    {
        Buf a; a.p = A; a.cap = 64;
        Buf b(std::move(a));
        CHECK(!a.p && !a.cap && b.p == A && b.cap == 64 && free_log.empty());
        a.p = B; a.cap = 32;
        a = std::move(b);                                          // the old target is freed once, the source is empty
        CHECK(freed(B) == 1 && freed(A) == 0 && a.p == A && a.cap == 64 && !b.p && !b.cap);
        Buf& self = a;
        a = std::move(self);                                       // self-move: nothing freed, nothing lost
        CHECK(a.p == A && a.cap == 64 && free_log.size() == 1);
        Buf c; c.p = C; c.cap = 8;
        c = Buf();                                                 // (how a holder empties itself)
        CHECK(freed(C) == 1 && !c.p && !c.cap);
    }
    CHECK(freed(A) == 1 && freed(B) == 1 && freed(C) == 1 && free_log.size() == 3);
}

static void check_owners() {
    check_buffer_owner<DevBuf>('d');
    check_buffer_owner<PinBuf>('p');
    // a growing vector of buffers (GraphDevice): reallocation moves them, nothing is freed until the vector lets go
    static char cells[100];
    free_log.clear();
    {
        std::vector<DevBuf> v;
        for (int i = 0; i < 100; ++i) { DevBuf b; b.p = &cells[i]; b.cap = 16; v.push_back(std::move(b)); }
        CHECK(free_log.empty());
        for (int i = 0; i < 100; ++i) CHECK(v[i].p == &cells[i] && v[i].cap == 16);
        v.clear();
        CHECK(free_log.size() == 100);
        for (int i = 0; i < 100; ++i) CHECK(freed(&cells[i]) == 1);
    }
    CHECK(free_log.size() == 100);
    // the growth rule of nrs_ctx::ensure
    CHECK(grown_bytes(0) == 256 && grown_bytes(1) == 257 && grown_bytes(1023) == 1023 + 255 + 256);
    CHECK(grown_bytes((size_t)1 << 32) == ((size_t)1 << 32) + ((size_t)1 << 30) + 256);
    // streams and events: destroyed once, by the right function; release() hands the handle on without destroying it
    ihipStream_t* S = reinterpret_cast<ihipStream_t*>(&cells[0]);
    ihipEvent_t* E = reinterpret_cast<ihipEvent_t*>(&cells[1]);
    free_log.clear();
    { Stream s; Event e; CHECK(!s && !e); }
    CHECK(free_log.empty());
    { Stream s(S); Stream t(std::move(s)); CHECK(!s && t.get() == S); }
    CHECK(order() == "s" && freed(S) == 1);
    { Event e(E); e.reset(); CHECK(!e && freed(E) == 1); }
    CHECK(order() == "se" && freed(E) == 1);
    // the order of nrs_ctx: the streams and events are declared before the buffers, so the buffers go first -- also when nrs_create
    // deletes a context whose set-up stopped half way (here: no second event yet)
    struct CtxLike { Stream stream; Event ev0, ev1; DevBuf buf; struct { DevBuf b; } arena; PinBuf pin; };
    free_log.clear();
    {
        CtxLike* c = new CtxLike();
        c->stream.reset(S); c->ev0.reset(E);
        c->buf.p = &cells[2]; c->arena.b.p = &cells[3]; c->pin.p = &cells[4];
        delete c;
    }
    CHECK(order() == "pddes");
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
    check_owners();
    std::printf("ctx_check OK: %d switches (names, identifiers, groups, the host packer's twelve), made-up environments and NRS_DEBUG lists, set / change / "
                "unset of every row by name, the three kinds with their defaults and shared clamps, nrs_create's option handling at every field boundary, the owners of device buffers, pinned memory, "
                "streams and events\n", (int)SW_COUNT);
    return 0;
}
