// The direct solver in a2's single-frame engines (K = 1): the context's plan cache, its plan thread and the two phases of an
// engine's set-up.  Part of nrs_engine.hip (one translation unit).  The layers below it, each in a file of its own:
//   nrs_nd_plan.hpp       the symbolic phase: nested dissection, fronts (plain C++)
//   nrs_nd_kernels.hpp    the device code: k_nd_level / k_nd_tile / k_nd_back (factorise, solve), k_nd_values (entry blocks)
//   nrs_nd_solver.hpp     a plan with its device arrays: upload, the launches of one factorise + solve
//   nrs_nd_debug.hpp      the solver on its own (nrs_debug_nd_solve)
//   nrs_nd_prep_host.hpp  the host stages of the set-up (plain C++; host/nd_prep_check.cpp checks them without a GPU)
// Set-up: nd_prep_run (structure only: pair lists, cache key, plan; on a helper thread of engine_create) and nd_engine_finish
// (value descriptors in the engine's row layout, uploads); the context caches the last plans (NdCache).
#pragma once
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include "nrs_nd_solver.hpp"
#include "nrs_nd_debug.hpp"
#include "nrs_nd_prep_host.hpp"

namespace nrs {
// One symbolic factorisation with everything the device needs for it (plan arrays, value descriptors, assembly areas, factor
// storage).  The context keeps the last few (nd_cache): a frame whose optimised set, edges and fixed flags equal an earlier frame's
// -- tracking in steady state: points are lost and edges added every few frames, not every frame -- takes the slot as it is, no
// plan build (1.0 ms at 1k points, 5 ms at 4.5k) and no upload.  The key is the complete input of nd_engine_setup except the
// positions the dissection bisects (they only steer its quality), compared byte for byte.
struct NdSlot {
    NdSolver S;
    std::shared_ptr<NdStruct> st;
    NdVals vals;
    DevBuf ws, vb;                   // S.buf = &ws (plan + factor storage), value descriptors
    std::vector<uint8_t> key;
    std::vector<char> h_vals;        // host image of the value descriptors (one upload)
    uint64_t hash = 0, used = 0;     // (used: LRU stamp)
    bool busy = false, cached = false;
    int n_free = 0, n_pairs = 0;
};
struct NdCache { std::vector<NdSlot*> slots; uint64_t clock = 0, hits = 0, misses = 0; };
constexpr int ND_CACHE_SLOTS = 4;

struct NdEngine {
    NdSlot* slot = nullptr;
    NdSolver& S() { return slot->S; }
    std::vector<double> pos;         // vertex positions the dissection bisects (M x 3, the caller's vertex order)
    std::vector<uint8_t> sig;        // RF_FIXED of every vertex + the pose's flag at set-up
    bool on = false;
};

static void plan_worker_free(nrs_ctx* c);
void nd_cache_free(nrs_ctx* c) {
    plan_worker_free(c);
    NdCache* nc = c->nd_cache;
    if (!nc) return;
    for (NdSlot* sl : nc->slots) delete sl;
    delete nc;
    c->nd_cache = nullptr;
}
void nd_cache_stats(nrs_ctx* c, int64_t out[2]) {
    const NdCache* nc = c->nd_cache;
    out[0] = nc ? (int64_t)nc->hits : 0; out[1] = nc ? (int64_t)nc->misses : 0;
}
static void nd_slot_release(nrs_ctx* c, NdEngine* nd) {            // the engine lets go of its slot: cached ones stay for later frames
    if (!nd || !nd->slot) return;
    if (nd->slot->cached) nd->slot->busy = false; else delete nd->slot;
    nd->slot = nullptr; nd->on = false;
}

// nrs_options.direct_solve (0: by size, 1: whenever possible, 2: never); NRS_ND / NRS_ND_MAX_ROWS override it for experiments.
// Measured (tools/nd_crossover.py, a2 per frame with a fresh plan per call, direct / PCG ms; flat kNN-16 graph): 129 points 7.9 / 34.6,
// 543: 13.1 / 52.8, 1013: 17.3 / 28.3, 2220: 32.7 / 45.6, 3165: 40.7 / 60.3, 4525: 58.3 / 75.1; on the all-pairs graph (22 neighbours
// per point instead of 13: heavier fronts) 543: 15.5 / 51.7, 1013: 22.4 / 61.8, 2220: 28.3 / 59.7, 3165: 39.8 / 66.3, 4525: 76.3 / 85.0.
// Ahead at every measured size; the default window ends where nothing has been measured.
static bool nd_mode_allows(nrs_ctx* c, int n_free) {
    int mode = c->opt.direct_solve;
    if (c->dbg.is_set(SW_ND)) mode = c->dbg.int_of(SW_ND) ? 1 : 2;
    const int nmax = c->dbg.int_of(SW_ND_MAX_ROWS);
    return mode != 2 && n_free > 0 && (mode == 1 || n_free <= nmax);
}
static bool nd_wanted(nrs_ctx* c, const Dev& d, int n_free) {
    return nd_mode_allows(c, n_free) && d.K == 1 && d.use_lds && !d.dform && !d.sh_on;
}

// ---- set-up in two phases.  Phase A (nd_prep_run) needs the problem's STRUCTURE only -- which vertices are free, which pairs of
// them an edge or a skinned observation couples -- in the caller's vertex order: it builds the pair lists and the cache key, looks
// the key up and, on a miss, builds the plan.  engine_create runs it on a helper thread next to its own packing of the incidence
// streams (both are host work: a 1k-point frame's 0.8 ms plan build disappears behind the 0.9 ms of packing).  Phase B
// (nd_engine_finish) ties the plan to the engine's row layout: value descriptors (rows, incidence slots), uploads, the slot.
// (the stages of both phases, NdIn and NdPrepData: nrs_nd_prep_host.hpp)
struct NdPrep : NdPrepData {
    bool wanted = false, plan_ok = false;
    std::string err;
    NdSlot* hit = nullptr;
    NdPlan plan;
    struct PlanWorker* worker = nullptr;                           // the context's helper thread is running nd_prep_run on this object (joined by wait())
    void wait();
    ~NdPrep() { wait(); }
};

// The context's helper thread for the symbolic phase (nd_prep_run next to engine_create's packing).  ONE thread for the context's lifetime, not one
// per frame: a fresh thread starts on a fresh malloc arena, and the ~15 MB of vectors a frame's plan builds were page-faulted in again every frame
// (embedded 500-node frames: pair lists 1.9 ms on a new thread, the whole phase faster inline on the caller's warm heap than next to it on a cold one).
struct PlanWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, busy = false, quit = false;
    bool start() {
        try { th = std::thread([this] { loop(); }); } catch (const std::system_error&) { return false; }
        return true;
    }
    void loop() {
        std::unique_lock<std::mutex> lk(m);
        while (true) {
            cv.wait(lk, [this] { return has_job || quit; });
            if (quit) return;
            std::function<void()> f = std::move(job);
            has_job = false;
            lk.unlock();
            f();                                                   // (nd_prep_run: lets nothing escape)
            lk.lock();
            busy = false;
            cv.notify_all();
        }
    }
    void submit(std::function<void()> f) {
        { std::lock_guard<std::mutex> lk(m); job = std::move(f); has_job = true; busy = true; }
        cv.notify_all();
    }
    void wait() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [this] { return !busy; }); }
    ~PlanWorker() {
        { std::lock_guard<std::mutex> lk(m); quit = true; }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
};
inline void NdPrep::wait() { if (worker) { worker->wait(); worker = nullptr; } }
static void plan_worker_free(nrs_ctx* c) { delete c->plan_worker; c->plan_worker = nullptr; }   // (idle: every NdPrep waits for it before it goes away)

static void nd_prep_run_body(nrs_ctx* c, const NdIn& in, NdPrep& P);
// (runs on a helper thread of engine_create: nothing may escape it -- an exception there would end the process)
static void nd_prep_run(nrs_ctx* c, const NdIn& in, NdPrep& P) {
    try { nd_prep_run_body(c, in, P); }
    catch (const std::exception& ex) { P.wanted = false; P.plan_ok = false; P.hit = nullptr; P.err = ex.what(); }
    catch (...) { P.wanted = false; P.plan_ok = false; P.hit = nullptr; P.err = "unknown exception in the plan thread"; }
}
// halves of a dissection of this many nodes go to threads of their own (first two levels; NRS_ND_PLAN_PAR=0: never; NRS_HOST_THREADS=1 likewise)
static int nd_plan_par_min(const nrs_ctx* c) {
    if (c->dbg.is_set(SW_ND_PLAN_PAR)) return c->dbg.int_of(SW_ND_PLAN_PAR);
    if (c->dbg.is_set(SW_HOST_THREADS) && c->dbg.int_of(SW_HOST_THREADS) <= 1) return 0;
    return std::thread::hardware_concurrency() >= 4 ? 700 : 0;
}
// the cache (read only here: nobody changes it while an engine is being set up): the free slot an earlier frame left with this key
static NdSlot* nd_cache_lookup(nrs_ctx* c, const NdPrep& P) {
    const NdCache* nc = c->nd_cache;
    if (!nc || c->dbg.is_set(SW_ND_NO_CACHE)) return nullptr;
    for (NdSlot* sl : nc->slots)
        if (!sl->busy && sl->st && sl->hash == P.hash && sl->key == P.key) return sl;
    return nullptr;
}
// phase A, stage by stage (nrs_nd_prep_host.hpp): number, allowed?, key, look-up, edge keys, skin, merge, pose, plan, observation lists
static void nd_prep_run_body(nrs_ctx* c, const NdIn& in, NdPrep& P) {
    P.wanted = false; P.plan_ok = false; P.hit = nullptr; P.st.reset();
    const bool tm = c->dbg.is_set(SW_TIMING);
    auto t_prev = std::chrono::steady_clock::now();
    double t_ms[3] = {0, 0, 0};                                    // key + look-up, pairs, plan
    auto lap = [&](int k) { const auto now = std::chrono::steady_clock::now(); t_ms[k] = std::chrono::duration<double, std::milli>(now - t_prev).count(); t_prev = now; };
    nd_number_nodes(in, P);
    if (!nd_mode_allows(c, P.n_free) || nd_has_window_dampers(in)) return;
    const int leaf_n = nd_leaf_n(c);
    nd_make_key(in, leaf_n, ND_SMAXN, P);
    if ((P.hit = nd_cache_lookup(c, P)) != nullptr) {
        // a frame whose key an earlier one had takes that one's plan and structure as they are; only the skinning weights are its own
        P.st = P.hit->st;
        if (in.n_skin > 0) nd_prep_ske_values(P, in.sk_om);
        P.wanted = true;
        return;
    }
    lap(0);
    P.st = std::make_shared<NdStruct>();
    std::vector<NdEdgeKey> keys;
    const bool twin = nd_edge_keys(in, P.node_of, keys);
    nd_skin_pairs(in, P);
    nd_sort_by_pair(keys, P.n_free);                               // (edge order inside a pair)
    const size_t n_coupl = nd_merge_pairs(keys, twin, P);
    nd_cut_pairs(P, n_coupl, nd_pose_pairs(in, P, n_coupl));
    P.wanted = true;
    lap(1);
    const std::vector<double> pos = nd_node_positions(in, P);
    const NdStruct& T = *P.st;
    P.plan_ok = nd_build_plan(P.n_nodes, pos.data(), P.last.data(), (int)T.pkind.size(), T.pairs.data(), P.plan, &P.err, leaf_n, ND_SMAXN, false, nd_plan_par_min(c), !c->dbg.is_set(SW_ND_NO_COVER));
    if (P.plan_ok && in.n_skin > 0) { nd_prep_ske(P, P.plan); nd_prep_ske_values(P, in.sk_om); }
    lap(2);
    if (tm) fprintf(stderr, "[nrs] direct solve set-up thread: key %.2f ms, pairs %.2f ms, plan %.2f ms\n", t_ms[0], t_ms[1], t_ms[2]);
}

// ---- phase B, step by step
// The slot of a new plan (a miss).  A new cached slot while there is room; then the least recently used one among those whose buffer
// already holds this plan (the factor and assembly storage of a 4.5k-point frame is ~100 MB: a hipMalloc per frame costs
// milliseconds); else the largest free one; and if every cached slot is held by a live engine, one that lives as long as this engine.
// (NRS_ND_NO_CACHE=1 only stops plans from being REUSED -- nd_cache_lookup -- the slots' buffers are.)  Null: out of host memory
static NdSlot* nd_slot_for_new_plan(NdCache* nc, const NdPlan& plan) {
    NdSlot* sl = nullptr;
    if ((int)nc->slots.size() < ND_CACHE_SLOTS) {
        sl = new (std::nothrow) NdSlot();
        if (!sl) return nullptr;
        sl->cached = true;
        nc->slots.push_back(sl);
        return sl;
    }
    const size_t need = 8 * (plan.L_doubles + plan.A_doubles);
    for (NdSlot* q : nc->slots)
        if (!q->busy && q->ws.cap >= need + need / 16 && (!sl || q->used < sl->used)) sl = q;
    if (!sl)
        for (NdSlot* q : nc->slots)
            if (!q->busy && (!sl || q->ws.cap > sl->ws.cap)) sl = q;
    return sl ? sl : new (std::nothrow) NdSlot();
}
// the slot this engine runs on: the one phase A found (*hit) or one for its new plan; counts both.  Null with NRS_OK in *rc: the
// plan could not be built, the PCG takes the problem
static NdSlot* nd_slot_acquire(nrs_ctx* c, NdCache* nc, const NdPrep& P, bool* hit, int* rc) {
    *rc = NRS_OK;
    *hit = P.hit && !P.hit->busy;
    if (*hit) {
        ++nc->hits;
        if (c->dbg.is_set(SW_TIMING)) fprintf(stderr, "[nrs] direct solve: plan of an earlier frame reused (%llu reused, %llu built)\n", (unsigned long long)nc->hits, (unsigned long long)nc->misses);
        return P.hit;
    }
    if (P.hit) { *rc = c->fail(NRS_ERR_STATE, "direct solve: the plan this engine was set up on was taken by another engine meanwhile (engines of one context are created one at a time)"); return nullptr; }
    if (!P.plan_ok) {
        if (c->dbg.is_set(SW_TIMING)) fprintf(stderr, "[nrs] direct solve not used: %s\n", P.err.c_str());
        return nullptr;
    }
    ++nc->misses;
    NdSlot* sl = nd_slot_for_new_plan(nc, P.plan);
    if (!sl) *rc = c->fail(NRS_ERR_ALLOC, "out of host memory");
    return sl;
}
// a miss: the new plan goes into the slot and up.  *fits = false: a front or a boundary beyond the LDS -- like a plan that could not
// be built, the PCG takes the problem
static int nd_slot_upload_plan(nrs_ctx* c, NdSlot* sl, NdPrep& P, int n_spec, bool* fits) {
    *fits = true;
    sl->hash = 0; sl->key.clear(); sl->key.push_back(0xFF);          // (matches no key while it is rebuilt)
    sl->S.buf = &sl->ws;
    sl->S.n_alt = n_spec;                                          // (solve sets for the speculative trials: engine_optimize uses min(e->n_spec, n_alt))
    sl->S.plan = std::move(P.plan);
    const int up = nd_upload(c, sl->S);
    if (up != NRS_ERR_INVALID) return up;
    if (c->dbg.is_set(SW_TIMING)) fprintf(stderr, "[nrs] direct solve not used: %s\n", c->err);
    *fits = false;
    return NRS_OK;
}
// the value descriptors (and, embedded mode, the observation lists built beside the plan) in ONE upload from a staging image the
// slot keeps (no synchronisation); the slot's kernel arguments point into it
static int nd_values_upload(nrs_ctx* c, NdSlot* sl, const NdStruct& T, const NdPrep& P, const NdValDesc& V, bool skinned) {
    const size_t n_nodes = V.nrow.size(), n_pairs = V.pd.size();
    NdStage G;
    const size_t o_nr = G.take(4 * n_nodes), o_no = G.take(4 * n_nodes), o_pd = G.take(sizeof(NdPairD) * n_pairs),
                 o_src = G.take(4 * std::max<size_t>(1, V.src.size())), o_sp = G.take(4 * std::max<size_t>(1, T.ske_ptr.size())),
                 o_st = G.take(4 * std::max<size_t>(1, T.ske_pt.size())), o_sc = G.take(8 * std::max<size_t>(1, P.ske_cf.size()));
    const size_t total = G.off;
    NRS_TRY(c->ensure(sl->vb, total));
    G.base = sl->vb.as<char>();
    sl->h_vals.assign(total, 0);
    G.img = sl->h_vals.data();
    G.put(o_nr, V.nrow.data(), 4 * n_nodes);
    G.put(o_no, V.node_out.data(), 4 * n_nodes);
    G.put(o_pd, V.pd.data(), sizeof(NdPairD) * n_pairs);
    G.put(o_src, V.src.data(), 4 * V.src.size());
    sl->vals.ske_ptr = nullptr; sl->vals.ske_pt = nullptr; sl->vals.ske_coef = nullptr;
    if (skinned) {
        G.put(o_sp, T.ske_ptr.data(), 4 * T.ske_ptr.size());
        G.put(o_st, T.ske_pt.data(), 4 * T.ske_pt.size());
        G.put(o_sc, P.ske_cf.data(), 8 * P.ske_cf.size());
        sl->vals.ske_ptr = G.at<const int>(o_sp); sl->vals.ske_pt = G.at<const int>(o_st); sl->vals.ske_coef = G.at<const double>(o_sc);
    }
    NRS_HIP(c, hipMemcpyAsync(G.base, sl->h_vals.data(), total, hipMemcpyHostToDevice, c->stream));
    sl->vals.node_row = G.at<const int>(o_nr);
    sl->vals.pair = G.at<const NdPairD>(o_pd);
    sl->vals.src = G.at<const int>(o_src);
    sl->vals.ent = sl->S.d_ent; sl->vals.ev = sl->S.d_ev; sl->vals.n_ent = (int)sl->S.plan.ent.size();
    sl->S.dev.node_out = G.at<const int>(o_no);
    sl->n_free = P.n_free; sl->n_pairs = (int)n_pairs;
    return NRS_OK;
}
// the engine's own vectors: where the solved step goes, the status words; and what the engine remembers of the set-up
static int nd_engine_bind(nrs_ctx* c, Engine* e, NdEngine* nd, NdSlot* sl) {
    Dev& d = e->d;
    sl->S.dev.out_rows = d.xv; sl->S.dev.out_pose = d.xp; sl->S.dev.flags = d.flags;
    // rows the solver never writes (fixed, padding) keep a zero step; so does a fixed pose
    NRS_HIP(c, hipMemsetAsync(d.xv, 0, sizeof(double) * 3 * (size_t)d.n_rows, c->stream));
    NRS_HIP(c, hipMemsetAsync(d.xp, 0, sizeof(double) * 6 * (size_t)d.K, c->stream));
    for (int j = 0; j < e->n_spec; ++j) {
        NRS_HIP(c, hipMemsetAsync(e->spec[j].xv, 0, sizeof(double) * 3 * (size_t)d.n_rows, c->stream));
        NRS_HIP(c, hipMemsetAsync(e->spec[j].xp, 0, sizeof(double) * 6 * (size_t)d.K, c->stream));
    }
    nd->sig.assign((size_t)d.M + 1, 0);
    for (int v = 0; v < d.M; ++v) nd->sig[v] = e->h_rflag[e->vrow[v]] & RF_FIXED;
    nd->sig[d.M] = e->h_pose_fixed[0];
    return NRS_OK;
}

// phase B: wait for the plan thread, acquire a slot, upload the plan on a miss, then descriptors, image and binding.  Leaves
// nd->on = false if the problem does not qualify
static int nd_engine_finish(nrs_ctx* c, Engine* e, NdEngine* nd, NdPrep& P) {
    {
        const bool tm = c->dbg.is_set(SW_TIMING);
        const auto t0 = std::chrono::steady_clock::now();
        P.wait();
        if (tm) fprintf(stderr, "[nrs] direct solve: waited %.2f ms for the plan thread\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    StageTimer lapf{c, "direct solve finish:", false};
    nd_slot_release(c, nd);                                        // (a rebuild after the fixed set changed: the old plan goes back to the cache)
    if (!P.wanted || !nd_wanted(c, e->d, P.n_free)) return NRS_OK;
    NdCache* nc = c->nd_cache;
    if (!nc) { nc = new (std::nothrow) NdCache(); if (!nc) return c->fail(NRS_ERR_ALLOC, "out of host memory"); c->nd_cache = nc; }
    bool hit = false;
    int rc = NRS_OK;
    NdSlot* sl = nd_slot_acquire(c, nc, P, &hit, &rc);
    if (!sl) return rc;
    struct SlotGuard {                                             // a slot whose set-up fails holds nothing valid
        NdSlot* sl; bool keep = false;
        ~SlotGuard() { if (keep) return; if (sl->cached) { sl->hash = 0; sl->key.clear(); sl->key.push_back(0xFF); sl->used = 0; } else delete sl; }
    } sguard{sl};
    if (!hit) {
        bool fits = true;
        NRS_TRY(nd_slot_upload_plan(c, sl, P, e->n_spec, &fits));
        if (!fits) return NRS_OK;                                  // (sguard leaves the slot empty; nd->on stays false; the embedded mode reports it, engine_create)
    }
    lapf("plan upload");
    NdValDesc V;
    if (!nd_value_descriptors(*P.st, P, e->vrow.data(), e->sp_pos.data(), e->dm_pos.data(), V)) return NRS_OK;   // (not a single-frame engine)
    lapf("descriptors");
    NRS_TRY(nd_values_upload(c, sl, *P.st, P, V, e->d.sk_n > 0));
    NRS_TRY(nd_engine_bind(c, e, nd, sl));
    lapf("values upload");
    sl->busy = true; sl->used = ++nc->clock;
    nd->slot = sl; nd->on = true;
    if (!hit) { sl->key.swap(P.key); sl->hash = P.hash; sl->st = P.st; }
    sguard.keep = true;
    if (c->dbg.is_set(SW_TIMING))
        fprintf(stderr, "[nrs] direct solve: %d free rows, %d pairs, %d fronts on %d levels, %d workgroups, %.1f MFLOP per factorisation\n", sl->n_free,
                sl->n_pairs, sl->S.plan.n_fronts, sl->S.plan.n_levels, (int)sl->S.plan.wg.size() / 3, sl->S.plan.flops / 1e6);
    return NRS_OK;
}

// both phases at once, from the engine's own mirrors (a rebuild after the fixed set changed)
static int nd_engine_setup(nrs_ctx* c, Engine* e, NdEngine* nd) {
    Dev& d = e->d;
    std::vector<uint8_t> rf(d.M);
    for (int v = 0; v < d.M; ++v) rf[v] = e->h_rflag[e->vrow[v]];
    NdIn in;
    in.M = d.M; in.rflag = rf.data(); in.pose_fixed = e->h_pose_fixed[0] != 0;
    in.n_sp = (int)(e->sp_ij.size() / 2); in.sp_ij = e->sp_ij.data();
    in.n_dm = (int)(e->dm_idx.size() / 4); in.dm_idx = e->dm_idx.data();
    in.n_skin = d.sk_n; in.sk_vert = e->sk_vert.data(); in.sk_om = e->sk_om.data();
    in.vpos = nd->pos.data();
    NdPrep P;
    nd_prep_run(c, in, P);
    return nd_engine_finish(c, e, nd, P);
}

static void nd_engine_free(nrs_ctx* c, NdEngine* nd) { nd_slot_release(c, nd); delete nd; }

}  // namespace nrs
