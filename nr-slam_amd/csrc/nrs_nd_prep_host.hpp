// Host stages of the direct solver's set-up for a2's single-frame engines (drivers: nrs_engine_nd.hpp nd_prep_run_body and
// nd_engine_finish): from the frame's structure -- which vertices are free, which pairs of them an edge or a skinned observation
// couples -- to the node pairs the plan is built on, the cache key, the embedded mode's observation lists and the value descriptors.
// Plain C++17: no HIP, no context, no environment, no output, no clocks -- what the context decides comes in as a parameter.
// host/nd_prep_check.cpp holds every stage to a brute-force restatement under sanitizers (`make nd_prep_check`).
#pragma once
#include <memory>
#include "nrs_engine_consts.hpp"
#include "nrs_nd_plan.hpp"

namespace nrs {

// the structure of one frame, in the caller's vertex order
struct NdIn {
    int M = 0;
    const uint8_t* rflag = nullptr;      // M, RF_* bits
    bool pose_fixed = false;
    int n_sp = 0; const int* sp_ij = nullptr;
    int n_dm = 0; const int* dm_idx = nullptr;
    int n_skin = 0; const int* sk_vert = nullptr; const double* sk_om = nullptr;
    const double* vpos = nullptr;        // M x 3: where the dissection bisects
};
// what a plan's key determines besides the plan itself: the node pairs with their edges and, in the embedded mode, which
// observations add to which plan entry.  Built once per plan; a frame that reuses the plan only fills in its own weights.
struct NdStruct {
    std::vector<int> pairs;                                        // node pairs: row-row couplings (sorted, unique), then the pose's
    std::vector<uint8_t> pkind;                                    // 0 row-row, 1 pose half (first node) - row, 2 pose - pose
    std::vector<int> eptr, eid;                                    // row-row pair -> its edges in edge order: (index << 1) | (0 spring, 1 damper)
    // embedded mode, per plan entry: the observations that add to it (ske_pt) and their coefficient as a product of skinning weights,
    // w[ske_ia] * w[ske_ib] (ske_ib < 0: w[ske_ia] alone); indices into the frame's SK_MAX-wide weight table
    std::vector<int> ske_ptr, ske_pt, ske_ia, ske_ib;
};
struct NdEdgeKey { uint64_t k; int id; };                        // (pair key, (edge index << 1) | (0 spring, 1 damper))
struct NdSkT { uint64_t k; int ia, ib; };                        // (pair key, the two weights' places in the weight table)
// what the stages build for one frame (NdPrep, nrs_engine_nd.hpp, adds the plan, the cache hit and the thread)
struct NdPrepData {
    int n_free = 0, n_nodes = 0;
    bool pose_free = false;
    std::vector<int> node_of, node_vtx;                            // vertex -> node (-1: fixed), node -> vertex
    std::shared_ptr<NdStruct> st;                                  // this engine's, or the reused slot's
    std::vector<uint8_t> last;
    std::vector<NdSkT> skt;                                        // embedded mode: (pair, weight places), sorted by pair
    std::vector<int> nl_ptr, nl_ix, pair_sk0, pair_sk1;            // per free node: the weight-table places of the observations that reach it
    std::vector<double> ske_cf;                                    // this frame's coefficients for st->ske_*
    std::vector<uint8_t> key;
    uint64_t hash = 0;
};

// ---- node numbering: the free vertices in vertex order, then the two halves of a free pose
inline void nd_number_nodes(const NdIn& in, NdPrepData& P) {
    P.node_of.assign(in.M, -1); P.node_vtx.clear();
    for (int v = 0; v < in.M; ++v)
        if (!(in.rflag[v] & RF_FIXED)) { P.node_of[v] = (int)P.node_vtx.size(); P.node_vtx.push_back(v); }
    P.n_free = (int)P.node_vtx.size();
    P.pose_free = !in.pose_fixed;
    P.n_nodes = P.n_free + (P.pose_free ? 2 : 0);
}
// four-vertex dampers: a BA window, not this solver's problem
inline bool nd_has_window_dampers(const NdIn& in) {
    for (int q = 0; q < in.n_dm; ++q)
        if (in.dm_idx[4 * (size_t)q] >= 0 || in.dm_idx[4 * (size_t)q + 1] >= 0) return true;
    return false;
}

// ---- the key: everything the stages below (and the plan) depend on -- not the positions, which may be an earlier frame's, and not
// the skinning weights, which a frame that reuses a plan fills in itself.  leaf_n / smax_n: the dissection's two tuning constants
inline uint64_t nd_hash(const uint8_t* p, size_t n) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ n;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, p + i, 8); h = (h ^ w) * 0xFF51AFD7ED558CCDull; h ^= h >> 29; }
    for (; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}
inline void nd_make_key(const NdIn& in, int leaf_n, int smax_n, NdPrepData& P) {
    std::vector<uint8_t> bits(in.M);
    for (int v = 0; v < in.M; ++v) bits[v] = in.rflag[v] & (RF_FIXED | RF_OBS);
    const int hdr[8] = {P.n_free, P.pose_free ? 1 : 0, in.M, in.n_skin, leaf_n, smax_n, in.n_sp, in.n_dm};
    std::vector<uint8_t>& key = P.key;
    key.clear();
    auto put = [&](const void* p, size_t bytes) { const uint8_t* b = static_cast<const uint8_t*>(p); key.insert(key.end(), b, b + bytes); };
    key.reserve(sizeof(hdr) + bits.size() + 8 * (size_t)in.n_sp + 16 * (size_t)in.n_dm + (size_t)SK_MAX * in.n_skin * 4);
    put(hdr, sizeof(hdr)); put(bits.data(), bits.size());
    put(in.sp_ij, 8 * (size_t)in.n_sp); put(in.dm_idx, 16 * (size_t)in.n_dm);
    if (in.n_skin > 0) put(in.sk_vert, 4 * (size_t)SK_MAX * in.n_skin);
    P.hash = nd_hash(key.data(), key.size());
}

// ---- row-row couplings of the regularisers, one key per edge between two different free nodes, in edge order (unsorted).
// a2 gives every regulariser as a spring AND a damper over the same two vertices, index for index (OPT:281-335): one key per edge
// then stands for both (`twin`, returned) -- half the records to sort; the merge puts the damper back behind the springs of its pair
inline bool nd_edge_keys(const NdIn& in, const std::vector<int>& node_of, std::vector<NdEdgeKey>& keys) {
    keys.clear();
    keys.reserve((size_t)in.n_sp + in.n_dm);
    auto add = [&](int va, int vb, int id) {
        const int a = node_of[va], b = node_of[vb];
        if (a < 0 || b < 0 || a == b) return;
        keys.push_back(NdEdgeKey{((uint64_t)std::min(a, b) << 32) | (uint32_t)std::max(a, b), id});
    };
    bool twin = in.n_sp == in.n_dm;
    for (int q = 0; twin && q < in.n_sp; ++q)
        twin = in.sp_ij[2 * (size_t)q] == in.dm_idx[4 * (size_t)q + 2] && in.sp_ij[2 * (size_t)q + 1] == in.dm_idx[4 * (size_t)q + 3];
    for (int q = 0; q < in.n_sp; ++q) add(in.sp_ij[2 * (size_t)q], in.sp_ij[2 * (size_t)q + 1], q << 1);
    if (!twin) for (int q = 0; q < in.n_dm; ++q) add(in.dm_idx[4 * (size_t)q + 2], in.dm_idx[4 * (size_t)q + 3], (q << 1) | 1);
    return twin;
}

// records with a key k = (low node << 32) | high node into key order, equal keys in their order of arrival: two stable counting
// passes (least significant half first) -- a comparison sort of the ~10^5 records of a 4.5k-point frame took longer than its plan
template <class T>
inline void nd_sort_by_pair(std::vector<T>& v, int n_free) {
    std::vector<T> tmp(v.size());
    std::vector<int> cnt(n_free + 1);
    for (int pass = 0; pass < 2; ++pass) {
        const std::vector<T>& inv = pass == 0 ? v : tmp;
        std::vector<T>& outv = pass == 0 ? tmp : v;
        std::fill(cnt.begin(), cnt.end(), 0);
        auto dig = [&](const T& t) { return pass == 0 ? (int)(t.k & 0xFFFFFFFFu) : (int)(t.k >> 32); };
        for (const T& t : inv) cnt[dig(t) + 1]++;
        for (int u = 0; u < n_free; ++u) cnt[u + 1] += cnt[u];
        for (const T& t : inv) outv[cnt[dig(t)]++] = t;
    }
}

// ---- embedded mode: the node pairs every skinned observation couples (all pairs of its <= 11 free nodes) with the places of the
// two weights, sorted by pair (P.skt), and per free node the observations that reach it (P.nl_ptr / nl_ix); everything in
// observation order (fixed summation order)
inline void nd_skin_pairs(const NdIn& in, NdPrepData& P) {
    const std::vector<int>& node_of = P.node_of;
    const int n_free = P.n_free;
    P.skt.clear();
    P.nl_ptr.assign(n_free + 1, 0); P.nl_ix.clear();
    if (in.n_skin <= 0) return;
    std::vector<int>& nl_ptr = P.nl_ptr;
    size_t n_pairs_sk = 0;
    for (int i = 0; i < in.n_skin; ++i) {
        int cnt = 0;
        for (int a = 0; a < SK_MAX; ++a) {
            const int va = in.sk_vert[(size_t)SK_MAX * i + a];
            if (va >= 0 && node_of[va] >= 0) { nl_ptr[node_of[va] + 1]++; ++cnt; }
        }
        n_pairs_sk += (size_t)cnt * (cnt - 1) / 2;
    }
    for (int u = 0; u < n_free; ++u) nl_ptr[u + 1] += nl_ptr[u];
    P.nl_ix.resize(nl_ptr[n_free]);
    std::vector<int> fill(nl_ptr.begin(), nl_ptr.end() - 1);
    std::vector<NdSkT> raw;
    raw.reserve(n_pairs_sk);
    for (int i = 0; i < in.n_skin; ++i)
        for (int a = 0; a < SK_MAX; ++a) {
            const int va = in.sk_vert[(size_t)SK_MAX * i + a];
            if (va < 0 || node_of[va] < 0) continue;
            const int na = node_of[va];
            P.nl_ix[fill[na]++] = SK_MAX * i + a;
            for (int b = a + 1; b < SK_MAX; ++b) {
                const int vb = in.sk_vert[(size_t)SK_MAX * i + b];
                if (vb < 0 || node_of[vb] < 0 || node_of[vb] == na) continue;
                const int nb2 = node_of[vb];
                raw.push_back(NdSkT{((uint64_t)std::min(na, nb2) << 32) | (uint32_t)std::max(na, nb2), SK_MAX * i + a, SK_MAX * i + b});
            }
        }
    nd_sort_by_pair(raw, n_free);                                   // by (low node, high node), observation order inside
    P.skt.swap(raw);
}

// ---- the union of the regularisers' couplings (keys, sorted) and the observations' (P.skt): a merge of the two sorted sequences
// into pairs / pkind / eptr / eid and the pairs' ranges of P.skt.  Inside a pair the springs come first and the dampers after them,
// each as they arrive.  The arrays are sized for the most there can be, the pose's pairs included, and written by index -- seven
// vector appends a pair were a third of this phase; nd_cut_pairs cuts them.  Returns the number of row-row couplings.
inline size_t nd_merge_pairs(const std::vector<NdEdgeKey>& keys, bool twin, NdPrepData& P) {
    NdStruct& T = *P.st;
    const std::vector<NdSkT>& skt = P.skt;
    const size_t pairs_max = keys.size() + skt.size() + (P.pose_free ? 2 * (size_t)P.n_free + 1 : 0);
    T.pairs.resize(2 * pairs_max); T.pkind.resize(pairs_max); T.eptr.resize(pairs_max + 1);
    T.eid.resize(keys.size() * (twin ? 2 : 1));                     // (exact: every key leaves one edge, or its two twins)
    P.pair_sk0.resize(pairs_max); P.pair_sk1.resize(pairs_max);
    size_t np = 0, ne = 0;
    T.eptr[0] = 0;
    for (size_t i = 0, st = 0; i < keys.size() || st < skt.size();) {
        const uint64_t kk = i < keys.size() && (st >= skt.size() || keys[i].k <= skt[st].k) ? keys[i].k : skt[st].k;
        const size_t i0 = i;
        for (; i < keys.size() && keys[i].k == kk; ++i) T.eid[ne++] = keys[i].id;
        if (twin) for (size_t j = i0; j < i; ++j) T.eid[ne++] = keys[j].id | 1;
        T.eptr[np + 1] = (int)ne;
        T.pairs[2 * np] = (int)(kk >> 32); T.pairs[2 * np + 1] = (int)(kk & 0xFFFFFFFFu);
        T.pkind[np] = 0;
        P.pair_sk0[np] = (int)st;
        while (st < skt.size() && skt[st].k == kk) ++st;
        P.pair_sk1[np] = (int)st;
        ++np;
    }
    return np;
}
// ---- the pose's pairs behind the n_coupl couplings -- both halves with every observed row, then the halves with each other -- and
// `last`: the nodes the dissection eliminates at the root.  Returns the number of pairs.
inline size_t nd_pose_pairs(const NdIn& in, NdPrepData& P, size_t n_coupl) {
    NdStruct& T = *P.st;
    const int n_free = P.n_free;
    size_t np = n_coupl;
    P.last.assign(P.n_nodes, 0);
    if (!P.pose_free) return np;
    P.last[n_free] = P.last[n_free + 1] = 1;
    for (int a = 0; a < n_free; ++a)
        if (in.rflag[P.node_vtx[a]] & RF_OBS)
            for (int h = 0; h < 2; ++h) { T.pkind[np] = 1; T.pairs[2 * np] = n_free + h; T.pairs[2 * np + 1] = a; ++np; }
    T.pkind[np] = 2; T.pairs[2 * np] = n_free + 1; T.pairs[2 * np + 1] = n_free; ++np;
    return np;
}
// ---- the three final lengths: pairs and pkind cover all np pairs; the edge lists and the observation ranges cover the n_coupl
// row-row couplings only (the pose's pairs carry neither), eptr with its closing entry
inline void nd_cut_pairs(NdPrepData& P, size_t n_coupl, size_t np) {
    NdStruct& T = *P.st;
    T.pairs.resize(2 * np); T.pkind.resize(np);
    T.eptr.resize(n_coupl + 1);
    P.pair_sk0.resize(n_coupl); P.pair_sk1.resize(n_coupl);
}

// where the dissection bisects: the free nodes at their vertices, the pose halves at the origin (they are `last` anyway)
inline std::vector<double> nd_node_positions(const NdIn& in, const NdPrepData& P) {
    std::vector<double> pos(3 * (size_t)P.n_nodes, 0.0);
    for (int a = 0; a < P.n_free; ++a)
        for (int k = 0; k < 3; ++k) pos[3 * (size_t)a + k] = in.vpos[3 * (size_t)P.node_vtx[a] + k];
    return pos;
}

// ---- embedded mode: the observation lists of a plan's entries
inline void nd_prep_ske(NdPrepData& P, const NdPlan& PL) {
    NdStruct& T = *P.st;
    const int n_free = P.n_free;
    T.ske_ptr.assign(PL.ent.size() + 1, 0);
    T.ske_pt.clear(); T.ske_ia.clear(); T.ske_ib.clear();
    const size_t guess = 4 * P.nl_ix.size() + P.skt.size();
    T.ske_pt.reserve(guess); T.ske_ia.reserve(guess); T.ske_ib.reserve(guess);
    auto push = [&](int ia, int ib) { T.ske_pt.push_back(ia / SK_MAX); T.ske_ia.push_back(ia); T.ske_ib.push_back(ib); };
    for (size_t q = 0; q < PL.ent.size(); ++q) {
        const uint32_t kind = PL.ent[q].src >> ND_KIND_SHIFT, idx = PL.ent[q].src & ND_SRC_MASK;
        auto node_list = [&](int u, bool squared) {
            if (u >= n_free) return;
            for (int t = P.nl_ptr[u]; t < P.nl_ptr[u + 1]; ++t) push(P.nl_ix[t], squared ? P.nl_ix[t] : -1);
        };
        if (kind == 0) node_list((int)idx, true);
        else if (kind == 2) node_list((int)idx, false);
        else if (T.pkind[idx] == 0) { for (int t = P.pair_sk0[idx]; t < P.pair_sk1[idx]; ++t) push(P.skt[t].ia, P.skt[t].ib); }
        else if (T.pkind[idx] == 1) node_list(T.pairs[2 * (size_t)idx + 1], false);
        T.ske_ptr[q + 1] = (int)T.ske_pt.size();
    }
}
// ... and this frame's coefficients for them
inline void nd_prep_ske_values(NdPrepData& P, const double* sk_om) {
    const NdStruct& T = *P.st;
    const size_t n = T.ske_pt.size();
    P.ske_cf.resize(n);
    for (size_t t = 0; t < n; ++t) {
        const double a = sk_om[T.ske_ia[t]];
        P.ske_cf[t] = T.ske_ib[t] < 0 ? a : a * sk_om[T.ske_ib[t]];
    }
}

// ---- value descriptors: the plan's nodes and pairs in terms of an engine's rows (vrow: vertex -> row) and incidence slots
// (sp_pos / dm_pos: 2 / 4 per edge).  nrow: node -> row or -1 - pose half; node_out: where the node's unknowns go (NdDev::node_out);
// src: per edge of a pair, in eid order, (slot << 1) | (0 spring, 1 damper).  False: an edge has no slot here (an incidence of
// another rank) -- not a single-frame engine
struct NdValDesc { std::vector<int> nrow, node_out, src; std::vector<NdPairD> pd; };
inline bool nd_value_descriptors(const NdStruct& T, const NdPrepData& P, const int* vrow, const int* sp_pos, const int* dm_pos, NdValDesc& V) {
    const int n_free = P.n_free, n_nodes = P.n_nodes, n_pairs = (int)T.pkind.size();
    std::vector<int>& nrow = V.nrow;
    nrow.resize(n_nodes); V.node_out.resize(n_nodes);
    for (int a = 0; a < n_free; ++a) { nrow[a] = vrow[P.node_vtx[a]]; V.node_out[a] = 3 * nrow[a]; }
    if (P.pose_free) { nrow[n_free] = -1; nrow[n_free + 1] = -2; V.node_out[n_free] = -1; V.node_out[n_free + 1] = -1 - 3; }
    V.pd.resize(n_pairs);
    V.src.resize(T.eid.size());                                     // (one source per edge of a pair, written by index)
    size_t n_src = 0;
    for (int i = 0; i < n_pairs; ++i) {
        const int a = T.pairs[2 * (size_t)i], b = T.pairs[2 * (size_t)i + 1];
        if (T.pkind[i] == 0) {
            // (the factor of an edge sits in both endpoints' incidence slots with the same value when both are free: the first one is read)
            V.pd[i] = NdPairD{0, nrow[a], nrow[b], (int)n_src, 0};
            for (int t = T.eptr[i]; t < T.eptr[i + 1]; ++t) {
                const int id = T.eid[t] >> 1, kind = T.eid[t] & 1;
                const int slot = kind ? dm_pos[4 * (size_t)id + 2] : sp_pos[2 * (size_t)id];
                if (slot < 0) return false;
                V.src[n_src++] = (slot << 1) | kind;
            }
            V.pd[i].nsrc = (int)n_src - V.pd[i].src0;
        } else if (T.pkind[i] == 1) V.pd[i] = NdPairD{1, a - n_free, nrow[b], 0, 0};
        else V.pd[i] = NdPairD{2, 0, 0, 0, 0};
    }
    return true;
}

}  // namespace nrs
