// a2, the host half (reference modules/optimization/g2o_optimization.cc:148-557, "OPT"): the container walks between the kernels -- which
// edges exist, the IQR test and the statuses, the stage-2 sub-problem -- as plain loops over host arrays.  No HIP and no context: nrs_track.hip
// calls these between its launches and turns a Status into the error text; host/track_check.cpp runs them under sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../include/nrs.h"

namespace nrs_track {

constexpr uint8_t VERTEX_FIXED = 4;                               // (= RF_FIXED of nrs_engine.hpp: asserted in nrs_track.hip)
constexpr float TH2_SQ = 5.99f, TH3_SQ = 0.584f;                  // chi2 gates of a reprojection edge / a regulariser (OPT:338-395)

enum What { DONE = 0, EMPTY, F_MAP_RANGE, NO_NODE, RAN_OFF };
struct Status { What what = DONE; int point = -1; };              // RAN_OFF: the walk of map point `point` ran off a truncated list

// ---- the frame's points as the optimisation sees them (OPT:174-192)
struct FrameIndex {
    int n_map = 0, N = 0, M = 0;                                  // map points, optimised points, nodes among them
    std::vector<int> map_to_frame, opt_f, ids, id_to_idx, node_of, node_idx;
    // what a walk does with a connection to map point o (OPT:262-275): >= 0 its index among the optimised points (a vertex: an edge, or
    // a skinning weight), -1 nothing (not in the frame, just triangulated, or optimised without a vertex: passed over), -2 a lost point
    std::vector<int> walk_code;
    std::vector<uint8_t> no_vertex, is_node;                      // embedded mode (M < N) only: per map point / per optimised point
};

// f_node (may be null: every optimised point is a node = the reference function): the EMBEDDED-DEFORMATION mode (N2, SURVEY.md 8d;
// stated in oracle/embedded_oracle.py).  Nodes carry the vertices and the regularisers of OPT:255-335; every other optimised point is
// skinned to the <= 11 nodes its own GetEdges walk accepts (normalised connection weights) and its reprojection edge constrains them.
inline Status frame_index(FrameIndex& x, int n_map, int n_f, const int32_t* f_map, const int32_t* f_status, const uint8_t* f_node) {
    x.n_map = n_map;
    x.map_to_frame.assign(n_map, -1);
    for (int i = 0; i < n_f; ++i) {
        if (f_map[i] >= n_map) return {F_MAP_RANGE, f_map[i]};
        if (f_map[i] >= 0) x.map_to_frame[f_map[i]] = i;
    }
    // points in the optimisation: TRACKED_WITH_3D in frame index order; the nodes among them carry the vertices
    for (int i = 0; i < n_f; ++i)
        if (f_status[i] == NRS_TRACKED_WITH_3D && f_map[i] >= 0) { x.opt_f.push_back(i); x.ids.push_back(f_map[i]); }
    const int N = x.N = (int)x.opt_f.size();
    if (N == 0) return {EMPTY, -1};                               // nothing to optimise (g2o: empty graph)
    x.id_to_idx.assign(n_map, -1); x.node_of.assign(N, -1);
    for (int i = 0; i < N; ++i) {
        x.id_to_idx[x.ids[i]] = i;
        if (!f_node || f_node[x.opt_f[i]]) { x.node_of[i] = (int)x.node_idx.size(); x.node_idx.push_back(i); }
    }
    x.M = (int)x.node_idx.size();
    if (x.M == 0) return {NO_NODE, -1};
    if (x.M < N) {                                                // optimised points without a vertex: a walk passes over them
        x.no_vertex.assign(n_map, 0); x.is_node.resize(N);
        for (int i = 0; i < N; ++i) { x.no_vertex[x.ids[i]] = x.node_of[i] < 0; x.is_node[i] = x.node_of[i] >= 0; }
    }
    x.walk_code.assign(n_map, -1);
    for (int o = 0; o < n_map; ++o) {
        const int fo = x.map_to_frame[o];
        if (fo < 0) continue;
        if (f_status[fo] != NRS_TRACKED_WITH_3D) { if (f_status[fo] != NRS_JUST_TRIANGULATED) x.walk_code[o] = -2; continue; }
        const int io = x.id_to_idx[o];
        if (io >= 0 && x.node_of[io] >= 0) x.walk_code[o] = io;
    }
    return {};
}

// ---- edge construction OPT:224-337: the regularisers between nodes, the skinned observations, the lost points met on the way
struct EdgeSet {
    std::vector<int> dm_idx, sp_ij, sk_node, sk_of, sk_idx, acc;  // (sk_*: skinned observations: nodes as vertex indices, slot per point, points)
    std::vector<float> dm_w, sp_d0;
    std::vector<double> sk_om;
    std::vector<uint8_t> n_acc, lost_flag;                        // (lost_flag: btree_set<ID> (OPT:222) as a flag per id, read out in ascending order)
    size_t ne = 0;
    void init(const FrameIndex& x) {
        const size_t N = x.N, M = x.M;
        acc.assign(11 * N, -1); n_acc.assign(N, 0); lost_flag.assign(x.n_map, 0);
        dm_idx.reserve(48 * M); sp_ij.reserve(24 * M); dm_w.reserve(12 * M); sp_d0.reserve(12 * M);
        sk_node.assign((N - M) * 11, -1); sk_om.assign((N - M) * 11, 0.0); sk_of.assign(N, -1);
    }
    // before a walk: room for max_edges connections (the edge arrays are sized once and written by index -- ~50 ns an edge with four
    // vector appends -- and cut to size by close())
    void reset(size_t max_edges) {
        ne = 0;
        dm_idx.resize(4 * max_edges); sp_ij.resize(2 * max_edges); dm_w.resize(max_edges); sp_d0.resize(max_edges);
        std::fill(n_acc.begin(), n_acc.end(), 0); std::fill(lost_flag.begin(), lost_flag.end(), 0);
        sk_idx.clear(); std::fill(sk_of.begin(), sk_of.end(), -1); std::fill(sk_node.begin(), sk_node.end(), -1); std::fill(sk_om.begin(), sk_om.end(), 0.0);
    }
    void connect(int va, int vb, float w, float d0) {             // spring + damper between two nodes: r = w (delta_a - delta_b)
        int* dq = &dm_idx[4 * ne];
        dq[0] = -1; dq[1] = -1; dq[2] = va; dq[3] = vb;
        dm_w[ne] = w;
        sp_ij[2 * ne] = va; sp_ij[2 * ne + 1] = vb;
        sp_d0[ne] = d0;
        ++ne;
    }
    // the k-th node of the skinned point that would take the next slot (kept only if it meets a node: skin_close)
    void skin(int k, int node, float w) { const size_t s = 11 * sk_idx.size() + k; sk_node[s] = node; sk_om[s] = (double)w; }
    void skin_close(int idx, int n) {                             // omega = w / sum w (float weights, double arithmetic, in walk order)
        if (n == 0) return;
        const size_t slot = sk_idx.size();
        double wsum = 0;
        for (int k = 0; k < n; ++k) wsum += sk_om[11 * slot + k];
        for (int k = 0; k < n; ++k) sk_om[11 * slot + k] /= wsum;
        sk_of[idx] = (int)slot;
        sk_idx.push_back(idx);
    }
    void close() { dm_idx.resize(4 * ne); sp_ij.resize(2 * ne); dm_w.resize(ne); sp_d0.resize(ne); }
    std::vector<int> lost_ids() const { std::vector<int> l; for (size_t i = 0; i < lost_flag.size(); ++i) if (lost_flag[i]) l.push_back((int)i); return l; }
};

// GetEdges lists as a source hands them over: entries beg[p] .. end[p] of map point p; truncated (may be null) per point: only a prefix
struct ListView { const int *beg, *end, *col; const float *w, *d0; const int* st; const char* truncated; };

// The walk of OPT:252-279 on the host.  The reference keeps per vertex the (other, edge) pairs it is part of and skips a neighbour it is
// already paired with (OPT:268-272).  A pair {idx, io} exists when idx's walk reaches io iff io was walked EARLIER (io < idx) and accepted
// idx (a list holds a connection once): the test reads io's accepted neighbours -- at most 11, one cache line -- instead of a container
inline Status host_walk(const FrameIndex& x, const ListView& l, EdgeSet& e) {
    e.reset(11 * (size_t)x.M);                                    // (at most 11 edges a walk)
    for (int idx = 0; idx < x.N; ++idx) {
        const int p = x.ids[idx];
        if (idx + 6 < x.N) {                                      // (the lists have just arrived from the device: every walk would start on lines that are in no cache)
            const int pb = l.beg[x.ids[idx + 6]];
            for (int o = 0; o < 32; o += 16) {
                __builtin_prefetch(l.col + pb + o); __builtin_prefetch(l.st + pb + o);
                __builtin_prefetch(l.w + pb + o); __builtin_prefetch(l.d0 + pb + o);
            }
        }
        const bool is_node = x.node_of[idx] >= 0;
        int n_reg = 0;
        bool ended = false;
        for (int a = l.beg[p]; a < l.end[p]; ++a) {
            const int other = l.col[a];
            if (n_reg > 10 || l.st[a] == NRS_GRAPH_BAD) { ended = true; break; }
            const int io = x.walk_code[other];                    // (one look-up instead of four dependent ones: ~2 x 10^5 entries are walked at 4.4k points)
            if (io < 0) {
                if (io == -2) e.lost_flag[other] = 1;
                continue;
            }
            if (is_node) {
                bool dup = false;
                if (io < idx) { const int* al = &e.acc[11 * (size_t)io]; for (int k = 0, nk = e.n_acc[io]; k < nk; ++k) dup = dup || al[k] == idx; }
                if (dup) continue;
                e.connect(x.node_of[idx], x.node_of[io], l.w[a], l.d0[a]);
                e.acc[11 * (size_t)idx + e.n_acc[idx]++] = io;    // (n_reg <= 10 here: at most 11 per walk)
            } else
                e.skin(n_reg, x.node_of[io], l.w[a]);
            ++n_reg;
        }
        if (!is_node) e.skin_close(idx, n_reg);
        if (!ended && l.truncated && l.truncated[p]) return {RAN_OFF, p};
    }
    e.close();
    return {};
}

// The same walk done on the device (nrs_rgraph.hip k_rg_walk): per optimised point (in order) the <= 11 connections its walk accepted --
// indices among the optimised points -- with weight and first distance, whether the walk ended before its list did, and the lost-point flags
struct WalkOut { std::vector<int> n_acc, acc; std::vector<float> w, d0; std::vector<uint8_t> ended, lost; int passes = 0; };

// ... and its read-out: the edges are made in the order the sequential walk makes them
inline Status edges_from_walk(const FrameIndex& x, const WalkOut& wo, const char* truncated, EdgeSet& e) {
    size_t n_e = 0;
    for (int idx = 0; idx < x.N; ++idx) if (x.node_of[idx] >= 0) n_e += wo.n_acc[idx];
    e.reset(n_e);
    std::copy(wo.lost.begin(), wo.lost.end(), e.lost_flag.begin());
    for (int idx = 0; idx < x.N; ++idx) {
        const bool is_node = x.node_of[idx] >= 0;
        const int nr = wo.n_acc[idx];
        for (int k = 0; k < nr; ++k) {
            const size_t s = 11 * (size_t)idx + k;
            if (is_node) e.connect(x.node_of[idx], x.node_of[wo.acc[s]], wo.w[s], wo.d0[s]);
            else e.skin(k, x.node_of[wo.acc[s]], wo.w[s]);
        }
        if (!is_node) e.skin_close(idx, nr);
        if (!wo.ended[idx] && truncated && truncated[x.ids[idx]]) return {RAN_OFF, x.ids[idx]};
    }
    e.close();
    return {};
}

// ---- OPT:401-455: deformation statistics, status / position updates (all optimised points alike).  delta: 3 doubles per optimised point;
// chi_r / chi_s: the last round's chi2 per node / per skinned observation.  Returns the median magnitude.
inline float deformation_statistics(const FrameIndex& x, const EdgeSet& e, const double* delta, const double* chi_r, const double* chi_s,
                                    uint8_t* rflag, char* inl, int32_t* f_status, float* f_pos, float* map_pos) {
    const int N = x.N;
    std::vector<float> mag(N), dfl(3 * (size_t)N);
    for (int i = 0; i < N; ++i) {
        const float d0 = (float)delta[3 * (size_t)i], d1 = (float)delta[3 * (size_t)i + 1], d2 = (float)delta[3 * (size_t)i + 2];
        dfl[3 * (size_t)i] = d0; dfl[3 * (size_t)i + 1] = d1; dfl[3 * (size_t)i + 2] = d2;
        mag[i] = std::sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    }
    std::vector<float> srt = mag;                                 // (the two order statistics of the sorted magnitudes, without sorting all of them)
    const int i1 = (int)(N * 0.25f), i3 = (int)(N * 0.75f);
    std::nth_element(srt.begin(), srt.begin() + i3, srt.end());
    std::nth_element(srt.begin(), srt.begin() + i1, srt.begin() + i3);
    const float q1 = srt[i1], q3 = srt[i3];
    const float th = 1.5f * (q3 - q1);
    for (int idx = 0; idx < N; ++idx) {
        const int fi = x.opt_f[idx];
        const double chi = x.node_of[idx] >= 0 ? chi_r[x.node_of[idx]] : (e.sk_of[idx] >= 0 ? chi_s[e.sk_of[idx]] : 0.0);
        if ((float)chi > TH2_SQ) { inl[idx] = 0; f_status[fi] = NRS_TRACKED; }
        if (mag[idx] >= q3 + th) { f_status[fi] = NRS_TRACKED; continue; }
        if (x.node_of[idx] >= 0) rflag[x.node_of[idx]] |= VERTEX_FIXED;
        for (int k = 0; k < 3; ++k) {
            const float cur = dfl[3 * (size_t)idx + k] + f_pos[3 * (size_t)fi + k];
            f_pos[3 * (size_t)fi + k] = cur;
            map_pos[3 * (size_t)x.ids[idx] + k] = cur;
        }
    }
    std::nth_element(mag.begin(), mag.begin() + N / 2, mag.end());
    return mag[N / 2];
}

// ---- stage 2 OPT:476-553: lost points follow their (fixed) optimised neighbours.  Vertices: the nodes, then the optimised points
// without a vertex as constants (their interpolated deformation), then the lost points
struct Stage2 {
    int NV = 0;                                                   // vertices before the lost points
    std::vector<int> vert_of, others, lost_ids, un_ij;            // (un_*: a lost point tied to an optimised neighbour)
    std::vector<float> un_w;
};
inline void stage2_vertices(const FrameIndex& x, Stage2& s) {
    s.vert_of.assign(x.N, -1);
    for (int v = 0; v < x.M; ++v) s.vert_of[x.node_idx[v]] = v;
    for (int idx = 0; idx < x.N; ++idx)
        if (x.node_of[idx] < 0) { s.vert_of[idx] = x.M + (int)s.others.size(); s.others.push_back(idx); }
    s.NV = x.M + (int)s.others.size();
}
// the walk counts optimised neighbours only and stops after 11: everything else may stay out of the lists
inline Status lost_walk(const FrameIndex& x, const ListView& l, Stage2& s) {
    const int L = (int)s.lost_ids.size();
    s.un_ij.clear(); s.un_w.clear();
    for (int li = 0; li < L; ++li) {
        const int p = s.lost_ids[li];
        if (li + 6 < L) { const int pb = l.beg[s.lost_ids[li + 6]]; __builtin_prefetch(l.col + pb); __builtin_prefetch(l.w + pb); __builtin_prefetch(l.col + pb + 16); __builtin_prefetch(l.w + pb + 16); }
        int n_reg = 0;
        bool ended = false;
        for (int a = l.beg[p]; a < l.end[p]; ++a) {
            if (n_reg > 10) { ended = true; break; }
            const int io = x.id_to_idx[l.col[a]];
            if (io < 0) continue;
            s.un_ij.insert(s.un_ij.end(), {s.NV + li, s.vert_of[io]});
            s.un_w.push_back(l.w[a]);
            ++n_reg;
        }
        if (!ended && l.truncated && l.truncated[p]) return {RAN_OFF, p};
    }
    return {};
}

// Only the free vertices (nodes the statistics left free, lost points) and what an edge ties them to take part: an edge between
// two fixed vertices is not in the problem (g2o skips allVerticesFixed edges; the engine masks them) and a fixed vertex no
// kept edge touches is read by nothing.  The engine is built on that part -- a few hundred vertices instead of all of them.
struct Compact {
    int M = 0;
    std::vector<int> newid, lm_pose, sp_ij, dm_idx, un_ij;       // newid: vertex of stage 2 -> vertex of the compacted problem, or -1
    std::vector<double> x, X0;
    std::vector<float> uv, sp_d0, dm_w;
    std::vector<uint8_t> rflag, dm_active;
};
inline void compact_stage2(const FrameIndex& fx, const Stage2& s, const EdgeSet& e, const uint8_t* rflag, const uint8_t* dm_active,
                           const double* delta_v, const double* delta, const double* X0, const float* uv, Compact& o) {
    const int M = fx.M, NV = s.NV, M2 = NV + (int)s.lost_ids.size(), E = (int)e.dm_w.size();
    std::vector<uint8_t> rflag_all(M2, 0), keep_v(M2, 0), keep_e(E, 0);
    std::copy(rflag, rflag + M, rflag_all.begin());
    for (int v = M; v < NV; ++v) rflag_all[v] = VERTEX_FIXED;
    for (int v = 0; v < M2; ++v) keep_v[v] = !(rflag_all[v] & VERTEX_FIXED);
    for (int k = 0; k < E; ++k) {
        const int a = e.sp_ij[2 * (size_t)k], b = e.sp_ij[2 * (size_t)k + 1];
        if (!(rflag_all[a] & VERTEX_FIXED) || !(rflag_all[b] & VERTEX_FIXED)) { keep_e[k] = 1; keep_v[a] = 1; keep_v[b] = 1; }
    }
    for (int q : s.un_ij) keep_v[q] = 1;
    o.newid.assign(M2, -1);
    for (int v = 0; v < M2; ++v) if (keep_v[v]) o.newid[v] = o.M++;
    o.x.assign(3 * (size_t)o.M, 0.0); o.X0.assign(3 * (size_t)o.M, 0.0); o.uv.assign(2 * (size_t)o.M, 0.f);
    o.lm_pose.assign(o.M, 0); o.rflag.assign(o.M, 0);
    for (int v = 0; v < M2; ++v) {
        const int nv = o.newid[v];
        if (nv < 0) continue;
        o.rflag[nv] = rflag_all[v];
        if (v < M) {
            for (int k = 0; k < 3; ++k) { o.x[3 * (size_t)nv + k] = delta_v[3 * (size_t)v + k]; o.X0[3 * (size_t)nv + k] = X0[3 * (size_t)v + k]; }
            o.uv[2 * (size_t)nv] = uv[2 * (size_t)v]; o.uv[2 * (size_t)nv + 1] = uv[2 * (size_t)v + 1];
        } else if (v < NV) {
            for (int k = 0; k < 3; ++k) o.x[3 * (size_t)nv + k] = delta[3 * (size_t)s.others[v - M] + k];
        }
    }
    for (int k = 0; k < E; ++k) {
        if (!keep_e[k]) continue;
        const int a = o.newid[e.sp_ij[2 * (size_t)k]], b = o.newid[e.sp_ij[2 * (size_t)k + 1]];
        o.sp_ij.insert(o.sp_ij.end(), {a, b});
        o.sp_d0.push_back(e.sp_d0[k]);
        o.dm_idx.insert(o.dm_idx.end(), {-1, -1, o.newid[e.dm_idx[4 * (size_t)k + 2]], o.newid[e.dm_idx[4 * (size_t)k + 3]]});
        o.dm_w.push_back(e.dm_w[k]);
        o.dm_active.push_back(dm_active[k]);
    }
    o.un_ij.resize(s.un_ij.size());
    for (size_t q = 0; q < s.un_ij.size(); ++q) o.un_ij[q] = o.newid[s.un_ij[q]];
}

}  // namespace nrs_track
