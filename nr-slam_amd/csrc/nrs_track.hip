// a2: CameraPoseAndDeformationOptimization (reference modules/optimization/g2o_optimization.cc:148-557)
// and the RegularizationGraph operations it embeds:
//   a19 GetEdges      (reference modules/map/regularization_graph.cc:61-87)
//   a20 UpdateVertex  (reference modules/map/regularization_graph.cc:89-146)
//
// Division of labour: every floating-point pass over points or edges (residuals, Jacobians, the
// normal equations, the PCG solves, edge re-weighting, neighbour ranking) is a HIP kernel; the host
// runs the reference's bookkeeping between them (which edges exist, levels between the two inlier
// rounds, the IQR test, statuses), because those are data-dependent container walks whose order is
// part of the reference's semantics (SURVEY.md 8a "container-order dependencies").
#include <algorithm>
#include <cmath>
#include <chrono>
#include "nrs_engine.hpp"
#include "nrs_rgraph.hpp"
#include "nrs_track_host.hpp"

namespace nrs {

// ---------------------------------------------------------------------------------------------
// InterpolationWeight (utilities/geometry_toolbox.cc:26-28): float argument, exp evaluated in
// double and rounded to float -- the value a correctly rounded expf returns (include/nrs.h).
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline float interpolation_weight(float d, float sigma) {
#pragma clang fp contract(off)
    const float arg = -(d * d) / (2.0f * sigma * sigma);
    return (float)exp((double)arg);
}

// a19, step 1: rank of every directed entry inside its row under (status asc, weight desc, index asc).  One wave per row: the row's
// (status, weight) pairs are read once, 64 at a time, and compared lane against lane (a thread per row re-read them from memory
// deg^2 times: 140 us for 1k rows of ~30 entries)
__global__ __launch_bounds__(256) void k_graph_rank(int n, const int* __restrict__ rowptr, const int* __restrict__ eid,
                                                    const float* __restrict__ e_w, const int* __restrict__ e_status, int* rank) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= n) return;
    const int lo = rowptr[p], hi = rowptr[p + 1];
    for (int a0 = lo; a0 < hi; a0 += 64) {
        const int a = a0 + lane;
        int sa = 0;
        float wa = 0.f;
        if (a < hi) { const int e = eid[a]; sa = e_status[e]; wa = e_w[e]; }
        int r = 0;
        for (int b0 = lo; b0 < hi; b0 += 64) {
            const int b = b0 + lane;
            int sb = 0;
            float wb = 0.f;
            if (b < hi) { const int e = eid[b]; sb = e_status[e]; wb = e_w[e]; }
            const int nb = min(64, hi - b0);
            for (int j = 0; j < nb; ++j) {
                const int sj = __shfl(sb, j, 64);
                const float wj = __shfl(wb, j, 64);
                const bool before = (sj != sa) ? (sj < sa) : ((wj != wa) ? (wj > wa) : (b0 + j < a));
                r += before ? 1 : 0;
            }
        }
        if (a < hi) rank[a] = r;
    }
}

// a19, step 2: cut position = rank of the first entry (in sorted order) whose weight < min_weight
__global__ void k_graph_cut(int n, const int* __restrict__ rowptr, const int* __restrict__ eid,
                            const float* __restrict__ e_w, const int* __restrict__ rank, float min_w, int* count) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int lo = rowptr[p], hi = rowptr[p + 1];
    int cut = hi - lo;
    for (int a = lo; a < hi; ++a)
        if (e_w[eid[a]] < min_w) cut = min(cut, rank[a]);
    count[p] = cut;
}

// a19, step 3: scatter the kept entries to their sorted position
__global__ void k_graph_scatter(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                const int* __restrict__ eid, const int* __restrict__ rank,
                                const int* __restrict__ o_rowptr, int* o_col, int* o_eid) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int lo = rowptr[p], hi = rowptr[p + 1];
    const int base = o_rowptr[p], cnt = o_rowptr[p + 1] - base;
    for (int a = lo; a < hi; ++a)
        if (rank[a] < cnt) { o_col[base + rank[a]] = col[a]; o_eid[base + rank[a]] = eid[a]; }
}

// a20: UpdateVertex for a list of points.  Two points sharing an edge compute the same values
// (the positions are final), so concurrent updates of one edge are idempotent.
__global__ void k_graph_update(int n_ids, const int* __restrict__ ids, const int* __restrict__ rowptr,
                               const int* __restrict__ col, const int* __restrict__ eid, const float* __restrict__ pos,
                               float* e_w, float* e_max, float* e_min, int* e_status, float sigma, float stretch_th,
                               int* good) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_ids) return;
    const int p = ids[i];
    const float px = pos[3 * p], py = pos[3 * p + 1], pz = pos[3 * p + 2];
    int n_good = 0;
    for (int a = rowptr[p]; a < rowptr[p + 1]; ++a) {
        const int o = col[a], e = eid[a];
        const float dx = px - pos[3 * o], dy = py - pos[3 * o + 1], dz = pz - pos[3 * o + 2];
        const float d = sqrtf(dx * dx + dy * dy + dz * dz);
        float mx = e_max[e], mn = e_min[e];
        if (d > mx) mx = d;
        if (d < mn) mn = d;
        e_max[e] = mx;
        e_min[e] = mn;
        e_w[e] = interpolation_weight(mx, sigma);
        if (fabsf((mx - mn) / mn) > stretch_th) e_status[e] = NRS_GRAPH_BAD;
        else ++n_good;
    }
    good[i] = n_good;
}

struct GraphDevice {            // device mirror of an nrs_graph for the duration of one call
    nrs_ctx* c;
    std::vector<DevBuf> allocs;
    int *rowptr = nullptr, *col = nullptr, *eid = nullptr, *status = nullptr, *rank = nullptr, *count = nullptr;
    int *o_rowptr = nullptr, *o_col = nullptr, *o_eid = nullptr, *ids = nullptr, *good = nullptr;
    float *w = nullptr, *mx = nullptr, *mn = nullptr, *pos = nullptr;
    int n = 0, nnz = 0, ne = 0;
    template <class Tp> int alloc(Tp** p, size_t n_) {
        DevBuf b;
        hipError_t e = c->alloc(b, std::max<size_t>(16, n_ * sizeof(Tp)));
        if (e != hipSuccess) return c->fail(NRS_ERR_ALLOC, "hipMalloc failed: %s", hipGetErrorString(e));
        *p = b.as<Tp>();
        allocs.push_back(std::move(b));
        return NRS_OK;
    }
};

static int graph_validate(nrs_ctx* c, const nrs_graph* g) {
    if (!g || g->n_points < 0 || g->n_edges < 0 || !g->rowptr) return c->fail(NRS_ERR_INVALID, "graph: null/negative");
    const int nnz = g->rowptr[g->n_points];
    if (nnz > 0 && (!g->col || !g->eid || !g->e_w || !g->e_d0 || !g->e_max || !g->e_min || !g->e_status))
        return c->fail(NRS_ERR_INVALID, "graph: null arrays");
    if (!(g->sigma > 0)) return c->fail(NRS_ERR_INVALID, "graph: sigma must be positive");
    for (int p = 0; p < g->n_points; ++p) {
        if (g->rowptr[p + 1] < g->rowptr[p]) return c->fail(NRS_ERR_INVALID, "graph: rowptr not monotone");
        for (int a = g->rowptr[p]; a < g->rowptr[p + 1]; ++a) {
            if (g->col[a] < 0 || g->col[a] >= g->n_points || g->eid[a] < 0 || g->eid[a] >= g->n_edges)
                return c->fail(NRS_ERR_INVALID, "graph: index out of range");
            if (a > g->rowptr[p] && g->col[a] <= g->col[a - 1]) return c->fail(NRS_ERR_INVALID, "graph: row not in ascending index order");
        }
    }
    return NRS_OK;
}

static int graph_upload(nrs_ctx* c, GraphDevice& G, const nrs_graph* g) {
    G.c = c;
    G.n = g->n_points;
    G.nnz = g->rowptr[g->n_points];
    G.ne = g->n_edges;
    NRS_TRY(G.alloc(&G.rowptr, G.n + 1)); NRS_TRY(G.alloc(&G.col, G.nnz)); NRS_TRY(G.alloc(&G.eid, G.nnz));
    NRS_TRY(G.alloc(&G.status, G.ne)); NRS_TRY(G.alloc(&G.w, G.ne)); NRS_TRY(G.alloc(&G.mx, G.ne)); NRS_TRY(G.alloc(&G.mn, G.ne));
    NRS_TRY(G.alloc(&G.rank, G.nnz)); NRS_TRY(G.alloc(&G.count, G.n + 1));
    NRS_TRY(G.alloc(&G.o_rowptr, G.n + 1)); NRS_TRY(G.alloc(&G.o_col, G.nnz)); NRS_TRY(G.alloc(&G.o_eid, G.nnz));
    NRS_TRY(G.alloc(&G.ids, G.n)); NRS_TRY(G.alloc(&G.good, G.n)); NRS_TRY(G.alloc(&G.pos, 3 * (size_t)G.n));
    NRS_HIP(c, hipMemcpyAsync(G.rowptr, g->rowptr, sizeof(int) * (G.n + 1), hipMemcpyHostToDevice, c->stream));
    if (G.nnz) {
        NRS_HIP(c, hipMemcpyAsync(G.col, g->col, sizeof(int) * G.nnz, hipMemcpyHostToDevice, c->stream));
        NRS_HIP(c, hipMemcpyAsync(G.eid, g->eid, sizeof(int) * G.nnz, hipMemcpyHostToDevice, c->stream));
    }
    if (G.ne) {
        NRS_HIP(c, hipMemcpyAsync(G.status, g->e_status, sizeof(int) * G.ne, hipMemcpyHostToDevice, c->stream));
        NRS_HIP(c, hipMemcpyAsync(G.w, g->e_w, sizeof(float) * G.ne, hipMemcpyHostToDevice, c->stream));
        NRS_HIP(c, hipMemcpyAsync(G.mx, g->e_max, sizeof(float) * G.ne, hipMemcpyHostToDevice, c->stream));
        NRS_HIP(c, hipMemcpyAsync(G.mn, g->e_min, sizeof(float) * G.ne, hipMemcpyHostToDevice, c->stream));
    }
    return NRS_OK;
}

// GetEdges for all points on the device copy; result on the host
static int graph_select(nrs_ctx* c, GraphDevice& G, float sigma, std::vector<int>& o_rowptr, std::vector<int>& o_col,
                        std::vector<int>& o_eid) {
    const float min_w = interpolation_weight((float)((double)sigma * 1.5), sigma);   // regularization_graph.cc:30
    const dim3 b(256), g((G.n + 255) / 256);
    o_rowptr.assign(G.n + 1, 0);
    if (G.n == 0) return NRS_OK;
    hipLaunchKernelGGL(k_graph_rank, dim3((G.n + 3) / 4), b, 0, c->stream, G.n, G.rowptr, G.eid, G.w, G.status, G.rank);
    hipLaunchKernelGGL(k_graph_cut, g, b, 0, c->stream, G.n, G.rowptr, G.eid, G.w, G.rank, min_w, G.count);
    NRS_HIP(c, hipGetLastError());
    std::vector<int> cnt(G.n);
    NRS_HIP(c, hipMemcpyAsync(cnt.data(), G.count, sizeof(int) * G.n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    for (int p = 0; p < G.n; ++p) o_rowptr[p + 1] = o_rowptr[p] + cnt[p];
    NRS_HIP(c, hipMemcpyAsync(G.o_rowptr, o_rowptr.data(), sizeof(int) * (G.n + 1), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_graph_scatter, g, b, 0, c->stream, G.n, G.rowptr, G.col, G.eid, G.rank, G.o_rowptr, G.o_col, G.o_eid);
    NRS_HIP(c, hipGetLastError());
    const int tot = o_rowptr[G.n];
    o_col.resize(tot);
    o_eid.resize(tot);
    if (tot) {
        NRS_HIP(c, hipMemcpyAsync(o_col.data(), G.o_col, sizeof(int) * tot, hipMemcpyDeviceToHost, c->stream));
        NRS_HIP(c, hipMemcpyAsync(o_eid.data(), G.o_eid, sizeof(int) * tot, hipMemcpyDeviceToHost, c->stream));
    }
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    return NRS_OK;
}

static int graph_update(nrs_ctx* c, GraphDevice& G, nrs_graph* g, const float* pos, int n_ids, const int* ids,
                        int* good) {
    if (n_ids == 0) return NRS_OK;
    NRS_HIP(c, hipMemcpyAsync(G.pos, pos, sizeof(float) * 3 * (size_t)G.n, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(G.ids, ids, sizeof(int) * n_ids, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_graph_update, dim3((n_ids + 255) / 256), dim3(256), 0, c->stream, n_ids, G.ids, G.rowptr, G.col,
                       G.eid, G.pos, G.w, G.mx, G.mn, G.status, g->sigma, g->stretch_th, G.good);
    NRS_HIP(c, hipGetLastError());
    NRS_HIP(c, hipMemcpyAsync(good, G.good, sizeof(int) * n_ids, hipMemcpyDeviceToHost, c->stream));
    if (G.ne) {
        NRS_HIP(c, hipMemcpyAsync(g->e_w, G.w, sizeof(float) * G.ne, hipMemcpyDeviceToHost, c->stream));
        NRS_HIP(c, hipMemcpyAsync(g->e_max, G.mx, sizeof(float) * G.ne, hipMemcpyDeviceToHost, c->stream));
        NRS_HIP(c, hipMemcpyAsync(g->e_min, G.mn, sizeof(float) * G.ne, hipMemcpyDeviceToHost, c->stream));
        NRS_HIP(c, hipMemcpyAsync(g->e_status, G.status, sizeof(int) * G.ne, hipMemcpyDeviceToHost, c->stream));
    }
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    return NRS_OK;
}

// Where a2 gets RegularizationGraph::GetEdges / UpdateVertex from: the host-owned flat graph (nrs_graph) or the
// device-resident dense one (nrs_rgraph: the reference's all-pairs density).
struct NeighbourSource {
    int n_points = 0;
    virtual ~NeighbourSource() {}
    // GetEdges of the map points in `want` (a source may serve every point), in the reference's order: entries beg[p] .. end[p] of
    // (col = other, w = weight, d0 = first distance, st = status) for a map point p that was asked for; the arrays are the source's
    // (valid until its next select)
    virtual int select(const std::vector<int>& want) = 0;
    std::vector<int> beg, end;
    const int* col = nullptr; const float* w = nullptr; const float* d0 = nullptr; const int* st = nullptr;
    // UpdateVertex of the listed points from the last world positions; good[i] = its return value
    virtual int update(const float* map_pos, int n, const int* ids, int* good) = 0;
    std::vector<char> truncated;      // per point: select() returned only a prefix of its list
    // per map point, may be null: 1 = the caller's walk passes over this point's connections without any effect unless they are
    // BAD; a source may leave them out of the lists (the dense one does: an embedded-mode walk would read ~N/M entries per node found)
    const std::vector<uint8_t>* pass_over = nullptr;
    virtual bool grow() { return false; }                          // fetch longer prefixes next time (false: there is nothing longer)
    // GetEdges of `want` AND the walk of OPT:252-279 over the lists where they are (a source that holds them on the device): what the
    // walks accept (nrs_track_host.hpp WalkOut).  *done = false: not available (the caller selects and walks itself).
    using WalkOut = nrs_track::WalkOut;
    nrs_track::ListView view() const { return {beg.data(), end.data(), col, w, d0, st, truncated.empty() ? nullptr : truncated.data()}; }
    virtual int device_walk(const std::vector<int>&, const std::vector<int>&, const uint8_t*, WalkOut&, bool* done) { *done = false; return NRS_OK; }
    virtual void prefix_hint(int) {}                               // the next walks read about this many entries (grow() still applies)
};

struct FlatSource : NeighbourSource {
    nrs_ctx* c; nrs_graph* g; GraphDevice G;
    int init() { n_points = g->n_points; return graph_upload(c, G, g); }
    std::vector<int> rp_, col_, st_;
    std::vector<float> w_, d0_;
    int select(const std::vector<int>&) override {
        std::vector<int> eid;
        NRS_TRY(graph_select(c, G, g->sigma, rp_, col_, eid));
        w_.resize(eid.size()); d0_.resize(eid.size()); st_.resize(eid.size());
        for (size_t a = 0; a < eid.size(); ++a) { w_[a] = g->e_w[eid[a]]; d0_[a] = g->e_d0[eid[a]]; st_[a] = g->e_status[eid[a]]; }
        beg.assign(rp_.begin(), rp_.end() - 1); end.assign(rp_.begin() + 1, rp_.end());
        col = col_.data(); w = w_.data(); d0 = d0_.data(); st = st_.data();
        return NRS_OK;
    }
    int update(const float* map_pos, int n, const int* ids, int* good) override { return graph_update(c, G, g, map_pos, n, ids, good); }
};

struct DenseSource : NeighbourSource {
    nrs_ctx* c; nrs_rgraph* g; int cap;
    int select(const std::vector<int>& want) override {           // (the lists are read where they land: the graph's pinned staging area)
        const size_t n = (size_t)n_points, m = want.size();
        beg.assign(n, 0); end.assign(n, 0);
        truncated.assign(n, 0);
        col = nullptr; w = nullptr; d0 = nullptr; st = nullptr;
        if (m == 0) return NRS_OK;
        RgDeviceLists l;
        NRS_TRY(rg_get_edges_staged(g, (int32_t)m, want.data(), cap, &l, pass_over ? pass_over->data() : nullptr));
        col = l.col; st = l.status; w = l.w; d0 = l.d0;
        for (size_t r = 0; r < m; ++r) {
            const int p = want[r];
            truncated[p] = l.count[r] > cap;
            beg[p] = (int)(r * (size_t)cap); end[p] = beg[p] + std::min(l.count[r], cap);
        }
        return NRS_OK;
    }
    int device_walk(const std::vector<int>& want, const std::vector<int>& code, const uint8_t* is_node, WalkOut& o, bool* done) override {
        *done = false;
        const size_t n = (size_t)n_points, m = want.size();
        if (m == 0 || code.size() != n) return NRS_OK;
        RgDeviceLists l;                                           // (its counts only: the lists stay on the device)
        NRS_TRY(rg_get_edges_staged(g, (int32_t)m, want.data(), cap, &l, pass_over ? pass_over->data() : nullptr, false));
        truncated.assign(n, 0);
        for (size_t r = 0; r < m; ++r) truncated[want[r]] = l.count[r] > cap;
        o.n_acc.resize(m); o.acc.resize(11 * m); o.w.resize(11 * m); o.d0.resize(11 * m); o.ended.resize(m); o.lost.resize(n);
        int conv = 0;
        NRS_TRY(rg_walk(g, (int)n, code.data(), is_node, o.n_acc.data(), o.acc.data(), o.w.data(), o.d0.data(), o.ended.data(), o.lost.data(), &conv, &o.passes));
        *done = conv != 0;
        return NRS_OK;
    }
    // (longer prefixes up to what one row's sort buffer holds in LDS; a walk that needs more than that is reported, not cut)
    bool grow() override {
        const int lim = std::min(n_points, rg_max_cap_per_point(g));
        if (cap >= lim) return false;
        cap = std::min(lim, 4 * cap);
        return true;
    }
    void prefix_hint(int n) override { cap = std::min(cap, std::max(n, 16)); }
    int update(const float* map_pos, int n, const int* ids, int* good) override { return n ? nrs_rgraph_update(g, map_pos, n, ids, good) : NRS_OK; }
};

namespace th = nrs_track;
static_assert(th::VERTEX_FIXED == RF_FIXED, "nrs_track_host.hpp states the engine's fixed-vertex bit");

// A walk that ran off a truncated list starts again on longer prefixes: body() until it reports completion
template <class Body> static int walk_to_completion(nrs_ctx* c, NeighbourSource& src, const char* whose, Body body) {
    for (;;) {
        th::Status st;
        NRS_TRY(body(st));
        if (st.what != th::RAN_OFF) return NRS_OK;
        if (!src.grow()) return c->fail(NRS_ERR_INVALID, "the neighbour walk of %smap point %d ran off its list", whose, st.point);
    }
}

// ---- edge construction OPT:224-337: GetEdges of the optimised points and the walk over them (order as in the reference)
static int build_edges(nrs_ctx* c, NeighbourSource& src, const th::FrameIndex& x, th::EdgeSet& es, StageTimer& mark) {
    const bool host_walk = c->dbg.is_set(SW_HOST_WALK);     // (A/B switch: the walk on the host, as before round 5)
    es.init(x);
    if (x.M < x.N) src.pass_over = &x.no_vertex;
    int ran_off_idx = -1;
    NRS_TRY(walk_to_completion(c, src, "", [&](th::Status& st) -> int {
        if (mark.on && ran_off_idx >= 0) fprintf(stderr, "[nrs] a2 device walk: point %d ran off its list: longer prefixes\n", ran_off_idx);
        ran_off_idx = -1;
        if (!host_walk) {
            // the dense graph walks on the device (nrs_rgraph.hip k_rg_walk): the lists never leave it, what comes back are the <= 11 accepted
            // connections per point; the edges are made from them here in the order the sequential walk makes them
            NeighbourSource::WalkOut wo;
            bool dev = false;
            const auto tw0 = std::chrono::steady_clock::now();
            NRS_TRY(src.device_walk(x.ids, x.walk_code, x.M < x.N ? x.is_node.data() : nullptr, wo, &dev));
            if (mark.on) fprintf(stderr, "[nrs] a2 device_walk call %.2f ms (N %d)\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count(), x.N);
            if (mark.on) fprintf(stderr, "[nrs] a2 device walk: %d passes, %s\n", wo.passes, dev ? "converged" : "not taken");
            if (dev) {
                mark("GetEdges + device walk");
                st = th::edges_from_walk(x, wo, src.view().truncated, es);
                if (st.what == th::RAN_OFF) ran_off_idx = x.id_to_idx[st.point];
                return NRS_OK;
            }
        }
        NRS_TRY(src.select(x.ids));                                // the walks start from the optimised points only
        mark("GetEdges");
        st = th::host_walk(x, src.view(), es);
        return NRS_OK;
    }));
    src.pass_over = nullptr;
    return NRS_OK;
}

// ---- the problem of the two inlier rounds, one vertex per node: the arrays its EngineSpec points into
struct RoundsProblem {
    Pose seed;
    std::vector<double> X0, zeros, skX0;
    std::vector<float> uv, skuv;
    std::vector<int> lm_pose;
    std::vector<uint8_t> rflag, dm_active, sk_active;
};
static void gather_obs(const th::FrameIndex& x, const std::vector<int>& idx, const float* f_pos, const float* f_uv, std::vector<double>& X0, std::vector<float>& uv) {
    X0.resize(3 * idx.size()); uv.resize(2 * idx.size());
    for (size_t v = 0; v < idx.size(); ++v) {
        const size_t fi = (size_t)x.opt_f[idx[v]];
        for (int k = 0; k < 3; ++k) X0[3 * v + k] = (double)f_pos[3 * fi + k];
        uv[2 * v] = f_uv[2 * fi];
        uv[2 * v + 1] = f_uv[2 * fi + 1];
    }
}
static void fill_spec(EngineSpec& s, RoundsProblem& P, const th::FrameIndex& x, const th::EdgeSet& es, const nrs_camera* cam, const float* f_pos,
                      const float* f_uv, const double pose_qt[7], float scale) {
    const int M = x.M, E = (int)es.dm_w.size(), S = (int)es.sk_idx.size();
    for (int i = 0; i < 4; ++i) P.seed.q[i] = pose_qt[i];
    for (int i = 0; i < 3; ++i) P.seed.t[i] = pose_qt[4 + i];
    quat_normalize(P.seed.q);
    gather_obs(x, x.node_idx, f_pos, f_uv, P.X0, P.uv);
    gather_obs(x, es.sk_idx, f_pos, f_uv, P.skX0, P.skuv);
    P.zeros.assign(3 * (size_t)M, 0.0); P.lm_pose.assign(M, 0);
    P.rflag.assign(M, RF_OBS | RF_REPROJ_ACTIVE); P.dm_active.assign(E, 1); P.sk_active.assign(S, 1);
    s.K = 1; s.M = M;
    s.poses = &P.seed;
    s.x = P.zeros.data(); s.X0 = P.X0.data();
    s.lm_pose = P.lm_pose.data(); s.uv = P.uv.data(); s.rflag = P.rflag.data();
    s.n_sp = E; s.sp_ij = es.sp_ij.data(); s.sp_d0 = es.sp_d0.data();
    s.n_dm = E; s.dm_idx = es.dm_idx.data(); s.dm_w = es.dm_w.data(); s.dm_active = P.dm_active.data();
    s.n_skin = S; s.sk_uv = P.skuv.data(); s.sk_X0 = P.skX0.data(); s.sk_node = es.sk_node.data(); s.sk_om = es.sk_om.data();
    s.cam.model = cam->model;
    for (int i = 0; i < 8; ++i) s.cam.p[i] = cam->params[i];
    ba_constants(s, scale);
    s.delta_pos = s.delta_spatial;                                // Huber sqrt(0.584) on the springs (OPT:324-326)
    s.spring_form = 1;
}

// ---- OPT:338-395: optimise, gate every edge by its chi2, optimise what passed
struct Chi2 { std::vector<double> r, d, s; };                     // per node (reprojection), per regulariser, per skinned observation
static int inlier_rounds(nrs_ctx* c, Engine* eng, const th::FrameIndex& x, const th::EdgeSet& es, RoundsProblem& P, Chi2& chi, std::vector<char>& inl,
                         nrs_lm_trace* trace, StageTimer& mark) {
    const int M = x.M, E = (int)es.dm_w.size(), S = (int)es.sk_idx.size();
    chi.r.resize(M); chi.d.resize(E); chi.s.resize(S);
    for (int rnd = 0; rnd < 2; ++rnd) {
        NRS_TRY(engine_reset(c, eng));
        NRS_TRY(engine_optimize(c, eng, 10, rnd, trace));
        mark("  round: optimize");
        NRS_TRY(engine_edge_chi2(c, eng, chi.r.data(), nullptr, chi.d.data()));
        mark("  round: edge chi2");
        for (int v = 0; v < M; ++v) {
            const bool out = (float)chi.r[v] > th::TH2_SQ;
            inl[x.node_idx[v]] = !out;
            P.rflag[v] = RF_OBS | (out ? 0 : RF_REPROJ_ACTIVE);
        }
        // OPT:365-383 sets the level of every regulariser of a vertex twice -- by the vertex's reprojection gate, then by the edge's own
        // chi2 -- and the second assignment stands: every edge (each has a vertex) ends at its own gate
        for (int k = 0; k < E; ++k) P.dm_active[k] = chi.d[k] > (double)th::TH3_SQ ? 0 : 1;
        // (the levels decide what the NEXT round optimises: after the last round only their host copies are read -- by stage 2 -- and this engine is not optimised again)
        if (rnd < 1) NRS_TRY(engine_update_flags(c, eng, P.rflag.data(), nullptr, nullptr, P.dm_active.data()));
        mark("  round: levels");
        if (S) {                                                  // the skinned observations' levels, by the same gate
            NRS_TRY(engine_skin_chi2(c, eng, chi.s.data()));
            for (int q = 0; q < S; ++q) { const bool out = (float)chi.s[q] > th::TH2_SQ; inl[es.sk_idx[q]] = !out; P.sk_active[q] = out ? 0 : 1; }
            if (rnd < 1) NRS_TRY(engine_skin_set_active(c, eng, P.sk_active.data()));
        }
    }
    return NRS_OK;
}

// the pose and the deformation of every optimised point: a node's own, a skinned point's the interpolated one
static int read_result(nrs_ctx* c, Engine* eng, const th::FrameIndex& x, const th::EdgeSet& es, Pose& pose_out, double pose_qt[7], std::vector<double>& delta_v,
                       std::vector<double>& delta) {
    delta_v.resize(3 * (size_t)x.M); delta.assign(3 * (size_t)x.N, 0.0);
    NRS_TRY(engine_download(c, eng, &pose_out, delta_v.data()));
    for (int i = 0; i < 4; ++i) pose_qt[i] = pose_out.q[i];
    for (int i = 0; i < 3; ++i) pose_qt[4 + i] = pose_out.t[i];
    for (int v = 0; v < x.M; ++v)
        for (int k = 0; k < 3; ++k) delta[3 * (size_t)x.node_idx[v] + k] = delta_v[3 * (size_t)v + k];
    for (size_t q = 0; q < es.sk_idx.size(); ++q)
        for (int k = 0; k < 3; ++k) {
            double a = 0;
            for (int j = 0; j < 11; ++j)
                if (es.sk_node[11 * q + j] >= 0) a += es.sk_om[11 * q + j] * delta_v[3 * (size_t)es.sk_node[11 * q + j] + k];
            delta[3 * (size_t)es.sk_idx[q] + k] = a;
        }
    return NRS_OK;
}

// ---- graph update OPT:457-474
static int update_graph(nrs_ctx* c, NeighbourSource& src, const th::FrameIndex& x, const std::vector<char>& inl, const float* map_pos, int32_t* f_status) {
    std::vector<int> upd_ids, upd_idx;
    for (int idx = 0; idx < x.N; ++idx)
        if (inl[idx]) { upd_ids.push_back(x.ids[idx]); upd_idx.push_back(idx); }
    std::vector<int> good(upd_ids.size());
    NRS_TRY(src.update(map_pos, (int)upd_ids.size(), upd_ids.data(), good.data()));
    for (size_t i = 0; i < upd_ids.size(); ++i)
        if (good[i] < 10 * 0.5) f_status[x.opt_f[upd_idx[i]]] = NRS_BAD;
    return NRS_OK;
}

static int track_core(nrs_ctx* c, const nrs_camera* cam, NeighbourSource& src, float* map_pos, int32_t n_f, const int32_t* f_map,
                      int32_t* f_status, const float* f_uv, float* f_pos, double pose_qt[7], float scale, float* deform_median,
                      int32_t* n_lost, int32_t* lost, nrs_lm_trace* trace, const uint8_t* f_node = nullptr) {
    StageTimer mark{c, "a2", false, 22};
    if (trace) { trace->count = 0; trace->iterations = 0; }
    *n_lost = 0;
    if (deform_median) *deform_median = 0.f;
    th::FrameIndex x;                                             // OPT:174-192
    switch (th::frame_index(x, src.n_points, n_f, f_map, f_status, f_node).what) {
        case th::EMPTY: return NRS_OK;
        case th::F_MAP_RANGE: return c->fail(NRS_ERR_INVALID, "f_map out of range");
        case th::NO_NODE: return c->fail(NRS_ERR_INVALID, "embedded mode: no node among the optimised points");
        default: break;
    }
    th::EdgeSet es;                                               // OPT:224-337
    NRS_TRY(build_edges(c, src, x, es, mark));
    mark("GetEdges + edge construction");

    EngineSpec s;
    RoundsProblem P;
    fill_spec(s, P, x, es, cam, f_pos, f_uv, pose_qt, scale);
    Engine* eng = nullptr;
    NRS_TRY(engine_create(c, s, &c->arena_trk, &eng));
    struct EG { nrs_ctx* c; Engine* e; ~EG() { engine_destroy(c, e); } } eg{c, eng};
    mark("engine 1");
    std::vector<char> inl(x.N, 1);
    Chi2 chi;
    NRS_TRY(inlier_rounds(c, eng, x, es, P, chi, inl, trace, mark));   // OPT:338-395
    mark("two rounds");
    Pose pose_out;
    std::vector<double> delta_v, delta;
    NRS_TRY(read_result(c, eng, x, es, pose_out, pose_qt, delta_v, delta));

    const float median = th::deformation_statistics(x, es, delta.data(), chi.r.data(), chi.s.data(), P.rflag.data(), inl.data(), f_status, f_pos, map_pos);   // OPT:401-455
    if (deform_median) *deform_median = median;
    mark("statistics");
    NRS_TRY(update_graph(c, src, x, inl, map_pos, f_status));       // OPT:457-474
    mark("UpdateVertex");

    th::Stage2 st2;                                               // OPT:476-553
    st2.lost_ids = es.lost_ids();
    if (st2.lost_ids.empty()) return NRS_OK;
    th::stage2_vertices(x, st2);
    std::vector<uint8_t> not_optimised(x.n_map);
    for (int i = 0; i < x.n_map; ++i) not_optimised[i] = x.id_to_idx[i] < 0;
    src.pass_over = &not_optimised;
    src.prefix_hint(32);
    NRS_TRY(walk_to_completion(c, src, "lost ", [&](th::Status& st) -> int {
        NRS_TRY(src.select(st2.lost_ids));                         // GetEdges sees the updated graph
        st = th::lost_walk(x, src.view(), st2);
        return NRS_OK;
    }));
    src.pass_over = nullptr;
    mark("GetEdges 2 + walk");
    th::Compact sub;
    th::compact_stage2(x, st2, es, P.rflag.data(), P.dm_active.data(), delta_v.data(), delta.data(), P.X0.data(), P.uv.data(), sub);
    const uint8_t pose_fixed = 1;
    EngineSpec s2 = s;
    s2.M = sub.M;
    s2.poses = &pose_out;
    s2.pose_fixed = &pose_fixed;
    s2.x = sub.x.data(); s2.X0 = sub.X0.data();
    s2.lm_pose = sub.lm_pose.data(); s2.uv = sub.uv.data(); s2.rflag = sub.rflag.data();
    s2.n_sp = (int)sub.sp_d0.size(); s2.sp_ij = sub.sp_ij.data(); s2.sp_d0 = sub.sp_d0.data();
    s2.n_dm = (int)sub.dm_w.size(); s2.dm_idx = sub.dm_idx.data(); s2.dm_w = sub.dm_w.data(); s2.dm_active = sub.dm_active.data();
    s2.n_un = (int)st2.un_w.size(); s2.un_ij = sub.un_ij.data(); s2.un_w = st2.un_w.data();
    s2.n_skin = 0;                                                // (the skinned observations take part in the two rounds only)
    engine_destroy(c, eng);
    eg.e = nullptr;
    Engine* eng2 = nullptr;
    NRS_TRY(engine_create(c, s2, &c->arena_trk, &eng2));
    eg.e = eng2;
    mark("engine 2");
    NRS_TRY(engine_optimize(c, eng2, 10, 2, trace));
    mark("stage 2 solve");
    std::vector<double> x_out(3 * (size_t)sub.M);
    NRS_TRY(engine_download(c, eng2, nullptr, x_out.data()));
    const int L = (int)st2.lost_ids.size();
    for (int li = 0; li < L; ++li) {
        for (int a = 0; a < 3; ++a)
            map_pos[3 * (size_t)st2.lost_ids[li] + a] = (float)x_out[3 * (size_t)sub.newid[st2.NV + li] + a] + map_pos[3 * (size_t)st2.lost_ids[li] + a];
        if (lost) lost[li] = st2.lost_ids[li];
    }
    *n_lost = L;
    return NRS_OK;
}

// what the three entry points of a2 ask of their arguments alike (extra_ok: the entry point's own conditions)
static int track_validate(nrs_ctx* c, const char* fn, const nrs_camera* cam, bool extra_ok, const float* map_pos, int32_t n_f, const int32_t* f_map,
                          const int32_t* f_status, const float* f_uv, const float* f_pos, const double* pose_qt, const int32_t* n_lost) {
    if (!c) return NRS_ERR_INVALID;
    if (!cam || !extra_ok || !map_pos || n_f < 0 || !pose_qt || !n_lost || (n_f > 0 && (!f_map || !f_status || !f_uv || !f_pos)))
        return c->fail(NRS_ERR_INVALID, "%s: bad argument", fn);
    if (cam->model != NRS_CAM_PINHOLE && cam->model != NRS_CAM_KB8) return c->fail(NRS_ERR_INVALID, "unknown camera model %d", cam->model);
    return NRS_OK;
}

// a2 on the device-resident dense graph, with or without f_node
static int track_dense(nrs_ctx* c, const char* fn, const nrs_camera* cam, nrs_rgraph* g, int32_t n_points, int32_t cap_per_point, float* map_pos, int32_t n_f,
                       const int32_t* f_map, int32_t* f_status, const float* f_uv, float* f_pos, const uint8_t* f_node, bool node_ok, double pose_qt[7],
                       float scale, float* deform_median, int32_t* n_lost, int32_t* lost, nrs_lm_trace* trace) {
    NRS_TRY(track_validate(c, fn, cam, g && n_points > 0 && cap_per_point > 0 && node_ok, map_pos, n_f, f_map, f_status, f_uv, f_pos, pose_qt, n_lost));
    // the dense state is capacity x capacity and map_pos has one row per point of it: a different n_points would index either
    // past the end (regularization_graph.cc has no such failure mode: its maps are keyed by ID)
    if (n_points != rg_capacity(g)) return c->fail(NRS_ERR_INVALID, "%s: n_points %d is not the graph's capacity %d", fn, n_points, rg_capacity(g));
    NRS_HIP(c, hipSetDevice(c->device));
    DenseSource src;
    src.c = c; src.g = g; src.cap = std::min(cap_per_point, rg_max_cap_per_point(g)); src.n_points = n_points;
    return track_core(c, cam, src, map_pos, n_f, f_map, f_status, f_uv, f_pos, pose_qt, scale, deform_median, n_lost, lost, trace, f_node);
}

}  // namespace nrs

using namespace nrs;

extern "C" int nrs_graph_select_neighbours(nrs_ctx* c, const nrs_graph* g, int32_t* o_rowptr, int32_t* o_col,
                                           int32_t* o_eid) {
    if (!c) return NRS_ERR_INVALID;
    NRS_TRY(graph_validate(c, g));
    if (!o_rowptr || (g->rowptr[g->n_points] > 0 && (!o_col || !o_eid))) return c->fail(NRS_ERR_INVALID, "null output");
    NRS_HIP(c, hipSetDevice(c->device));
    GraphDevice G;
    NRS_TRY(graph_upload(c, G, g));
    std::vector<int> rp, oc, oe;
    NRS_TRY(graph_select(c, G, g->sigma, rp, oc, oe));
    std::copy(rp.begin(), rp.end(), o_rowptr);
    std::copy(oc.begin(), oc.end(), o_col);
    std::copy(oe.begin(), oe.end(), o_eid);
    return NRS_OK;
}

extern "C" int nrs_graph_update(nrs_ctx* c, nrs_graph* g, const float* pos, int32_t n_ids, const int32_t* ids,
                                int32_t* good_count) {
    if (!c) return NRS_ERR_INVALID;
    NRS_TRY(graph_validate(c, g));
    if (n_ids < 0 || (n_ids > 0 && (!ids || !good_count || !pos))) return c->fail(NRS_ERR_INVALID, "nrs_graph_update: bad argument");
    for (int i = 0; i < n_ids; ++i)
        if (ids[i] < 0 || ids[i] >= g->n_points) return c->fail(NRS_ERR_INVALID, "point index out of range");
    NRS_HIP(c, hipSetDevice(c->device));
    GraphDevice G;
    NRS_TRY(graph_upload(c, G, g));
    return graph_update(c, G, g, pos, n_ids, ids, good_count);
}

extern "C" int nrs_track_deform_solve(nrs_ctx* c, const nrs_camera* cam, nrs_graph* g, float* map_pos,
                                      int32_t n_f, const int32_t* f_map, int32_t* f_status, const float* f_uv,
                                      float* f_pos, double pose_qt[7], float scale, float* deform_median,
                                      int32_t* n_lost, int32_t* lost, nrs_lm_trace* trace) {
    NRS_TRY(track_validate(c, "nrs_track_deform_solve", cam, true, map_pos, n_f, f_map, f_status, f_uv, f_pos, pose_qt, n_lost));
    NRS_TRY(graph_validate(c, g));
    NRS_HIP(c, hipSetDevice(c->device));
    FlatSource src;
    src.c = c; src.g = g;
    NRS_TRY(src.init());
    return track_core(c, cam, src, map_pos, n_f, f_map, f_status, f_uv, f_pos, pose_qt, scale, deform_median, n_lost, lost, trace);
}

// The same function on the device-resident dense graph (include/nrs.h): GetEdges / UpdateVertex see all N - 1
// connections of a point, as in the reference.
extern "C" int nrs_track_deform_solve_rg(nrs_ctx* c, const nrs_camera* cam, nrs_rgraph* g, int32_t n_points, int32_t cap_per_point,
                                         float* map_pos, int32_t n_f, const int32_t* f_map, int32_t* f_status, const float* f_uv,
                                         float* f_pos, double pose_qt[7], float scale, float* deform_median, int32_t* n_lost,
                                         int32_t* lost, nrs_lm_trace* trace) {
    return track_dense(c, "nrs_track_deform_solve_rg", cam, g, n_points, cap_per_point, map_pos, n_f, f_map, f_status, f_uv, f_pos, nullptr, true, pose_qt, scale,
                       deform_median, n_lost, lost, trace);
}

// N2 (include/nrs.h): the embedded-deformation mode on the device-resident dense graph
extern "C" int nrs_track_deform_solve_embedded(nrs_ctx* c, const nrs_camera* cam, nrs_rgraph* g, int32_t n_points, int32_t cap_per_point,
                                               float* map_pos, int32_t n_f, const int32_t* f_map, int32_t* f_status, const float* f_uv,
                                               float* f_pos, const uint8_t* f_node, double pose_qt[7], float scale, float* deform_median,
                                               int32_t* n_lost, int32_t* lost, nrs_lm_trace* trace) {
    return track_dense(c, "nrs_track_deform_solve_embedded", cam, g, n_points, cap_per_point, map_pos, n_f, f_map, f_status, f_uv, f_pos, f_node,
                       n_f <= 0 || f_node, pose_qt, scale, deform_median, n_lost, lost, trace);
}
