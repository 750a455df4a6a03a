// Host stages of the keyframe-block factorisation's set-up (driver: nrs_engine_kft_setup.hpp kft_setup): from an embedded BA window's
// structure -- which rows are free, which springs, dampers and skinned observations couple them -- to the compact numbering, the
// eligibility decision, the same-keyframe pair lists, the temporal coupling lists and the layout of the one device buffer.
// Plain C++17: no HIP, no context, no environment, no output, no clocks -- what the context decides comes in as a parameter.
// host/kft_prep_check.cpp holds every stage to a brute-force restatement under sanitizers (`make kft_prep_check`).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "nrs_engine_consts.hpp"

namespace nrs {

// ---- the sort key of a node pair, k << 24 | hi << 12 | lo (KftDev::pp_id is its low 32 bits; the kernels' readers decode the same fields)
constexpr int KFT_KEY_NODE_BITS = 12, KFT_KEY_K_SHIFT = 24;
constexpr uint32_t KFT_KEY_NODE_MASK = 0xFFF;
constexpr int KFT_K_MAX = (1 << (32 - KFT_KEY_K_SHIFT)) - 1;       // keyframes a 32-bit pp_id can name
constexpr int KFT_NF_LIMIT = 1 << KFT_KEY_NODE_BITS;               // free nodes per keyframe: below this
static_assert(KFT_KEY_K_SHIFT == 2 * KFT_KEY_NODE_BITS && KFT_KEY_NODE_MASK == (1u << KFT_KEY_NODE_BITS) - 1 && KFT_K_MAX == 255 && KFT_NF_LIMIT == 4096,
              "the key's fields: two node indices below the keyframe index, all inside pp_id's 32 bits");
inline uint64_t kft_key(int k, int hi, int lo) { return ((uint64_t)k << KFT_KEY_K_SHIFT) | ((uint64_t)hi << KFT_KEY_NODE_BITS) | (uint64_t)lo; }
inline int kft_key_k(uint64_t key) { return (int)(key >> KFT_KEY_K_SHIFT); }
inline int kft_key_hi(uint64_t key) { return (int)((key >> KFT_KEY_NODE_BITS) & KFT_KEY_NODE_MASK); }
inline int kft_key_lo(uint64_t key) { return (int)(key & KFT_KEY_NODE_MASK); }
// a list entry's source, type << 30 | index (KftDev::pe_src): whose value the entry reads
enum : uint32_t { KFT_SRC_SPRING = 0, KFT_SRC_DAMPER = 1, KFT_SRC_SKIN = 2, KFT_SRC_BOUNDARY = 3 };
inline uint32_t kft_src(uint32_t type, int index) { return (type << 30) | (uint32_t)index; }
constexpr uint32_t KFT_TE_MINUS = 0x80000000u;                     // te_src: the coupling takes - s

// the window, in the caller's vertex order, and what the context decided
struct KftIn {
    int K = 0, n_rows = 0;
    const int* pose_grp_ptr = nullptr;   // K + 1: first ROW_ALIGN group of every keyframe
    const uint8_t* rflag = nullptr;      // n_rows, RF_* bits (fixed and padding rows: RF_FIXED)
    const uint8_t* pose_fixed = nullptr; // K or null (none fixed)
    int M = 0;
    const int* lm_pose = nullptr;        // M: vertex -> keyframe
    const int* vrow = nullptr;           // M: vertex -> row
    int n_sp = 0; const int* sp_ij = nullptr; const int* sp_pos = nullptr;     // 2 per spring: vertices, incidence slots (null: none were kept)
    int n_dm = 0; const int* dm_idx = nullptr; const int* dm_pos = nullptr;    // 4 per damper (1c, 2c, 1n, 2n), -1: absent
    int n_skin = 0;
    const int* sk_pose = nullptr; const int* sk_node = nullptr; const double* sk_om = nullptr; const int* sk_slot = nullptr;
    // sharded (on: world > 1): this rank holds the keyframes [sh_k0, sh_k0 + sh_nk); kb: world + 1 keyframe ranges of the ranks.
    // One GPU: off, [0, K), kb = {0, K}
    bool sh = false; int world = 1, sh_k0 = 0, sh_nk = 0; const int* kb = nullptr;
    int embedded_solver = 0;             // nrs_options.embedded_solver: 0 the cost model decides, otherwise the caller did
    size_t lds_cap = 0, step_lds = 0, panel_lds = 0;   // the device's LDS per workgroup; what k_kft_step and k_kft_panel need whatever the window
    int threads = 1;                     // for the pair lists
};
// why a window does not take the factorisation (the driver leaves the block-Jacobi PCG in place for every one of them)
enum KftReason {
    KFT_ELIGIBLE = 0, KFT_NO_POSITIONS, KFT_KEYFRAME_COUNT, KFT_NO_FREE_NODE, KFT_BLOCK_BEYOND_KEY, KFT_BEYOND_LDS, KFT_PCG_CHEAPER,
    KFT_SPRING_ACROSS_KEYFRAMES, KFT_DAMPER_ACROSS_PAIR, KFT_DAMPER_NOT_CONSECUTIVE
};
inline const char* kft_reason_name(KftReason r) {
    static const char* const names[] = {"eligible", "no incidence positions", "too many keyframes (or none)", "no free node", "block too large for the key", "beyond LDS",
                                        "cost model prefers the PCG", "a spring across keyframes", "a damper across one keyframe's pairs", "a damper that does not join consecutive keyframes"};
    return names[r];
}

struct KftVert { int16_t k, c; };                                  // a vertex's keyframe and compact node (-1: fixed); 16 bits: K <= KFT_K_MAX, nf_max < KFT_NF_LIMIT
struct KftNum { std::vector<int> row_ci, kf_nf, kf_np, kf_row; std::vector<KftVert> vert; int nf_max = 0; };
struct KftDims { int ld = 0, nb = 0, nfm = 0; };
struct KftEnt { uint64_t key; uint32_t src; double w; };
struct KftCpl { uint64_t key; uint32_t src; };                     // a temporal coupling's entry: no weight, so 16 bytes to sort where KftEnt's are 24
struct KftEdges { std::vector<KftEnt> pe; std::vector<KftCpl> te; std::vector<int> bd_slot; };
struct KftKfLists { std::vector<uint32_t> pp_id, pe_src; std::vector<int> pp_ptr; std::vector<double> pe_w; };
struct KftSkinIndex { std::vector<size_t> small_ptr; std::vector<KftEnt> small; std::vector<int> sk_ptr, sk_of; };
struct KftPairs { std::vector<uint32_t> pp_id; std::vector<int> pp_ptr; std::vector<size_t> ent_base; };
struct KftCouplings { std::vector<uint64_t> tp_key; std::vector<int> tp_ptr; std::vector<uint32_t> te_src; std::vector<int> cl_ptr[2], cl_from[2], cl_tp[2]; };

// ---- the window itself: guarantees 1 <= K <= KFT_K_MAX and incidence slots for the springs there are
inline KftReason kft_window_reason(const KftIn& in) {
    if (in.K < 1 || in.K > KFT_K_MAX) return KFT_KEYFRAME_COUNT;
    if (!in.sp_pos && in.n_sp > 0) return KFT_NO_POSITIONS;
    return KFT_ELIGIBLE;
}
// ---- numbering: per keyframe, its free rows in row order get 0 .. kf_nf[k] - 1 (row_ci; -1: fixed / padding); kf_np 6 / 0
inline void kft_number_rows(const KftIn& in, KftNum& N) {
    N.kf_nf.assign(in.K, 0); N.kf_np.assign(in.K, 0); N.row_ci.assign((size_t)in.n_rows, -1);
    N.nf_max = 0;
    for (int k = 0; k < in.K; ++k) {
        int n = 0;
        for (int r = in.pose_grp_ptr[k] * ROW_ALIGN; r < in.pose_grp_ptr[k + 1] * ROW_ALIGN; ++r)
            if (!(in.rflag[r] & RF_FIXED)) N.row_ci[r] = n++;
        N.kf_nf[k] = n;
        N.kf_np[k] = (in.pose_fixed && in.pose_fixed[k]) ? 0 : 6;
        N.nf_max = std::max(N.nf_max, n);
    }
}
// ... and its inverse with the blocks' stride: kf_row[k * nfm + compact node] = row, -1 behind a keyframe's last node
inline void kft_rows_of_nodes(const KftIn& in, int nfm, KftNum& N) {
    N.kf_row.assign((size_t)in.K * nfm, -1);
    for (int k = 0; k < in.K; ++k)
        for (int r = in.pose_grp_ptr[k] * ROW_ALIGN; r < in.pose_grp_ptr[k + 1] * ROW_ALIGN; ++r)
            if (N.row_ci[r] >= 0) N.kf_row[(size_t)k * nfm + N.row_ci[r]] = r;
}
// ... and per vertex: what the two passes over the edges look up, one load where lm_pose, vrow and row_ci are three (behind kft_limits:
// the fields hold every index)
inline void kft_vertex_table(const KftIn& in, KftNum& N) {
    N.vert.resize((size_t)in.M);
    for (int v = 0; v < in.M; ++v) N.vert[v] = KftVert{(int16_t)in.lm_pose[v], (int16_t)N.row_ci[in.vrow[v]]};
}

// ---- cost model of the two solvers, ms per LM trial, fitted on tools/kft_probe.py runs (10 .. 40 keyframes, 100 .. 650 nodes per keyframe,
// profiles/r06_kft_crossover.txt): the factorisation is ceil(K / 2) dependent inversions of nb + 1 launches, (16.5 + 0.72 nb) us a launch
// (the panel workgroup's path: sweep, look-ahead, tile I/O), + 0.05 K ms per trial (assembly, Schur updates,
// one pass over the chains); the block-Jacobi PCG took 14 ms (K / 20)^0.45 per trial whatever the node count.  Measured on 20 keyframes:
// 7.8 x the PCG's rate at 100 nodes per keyframe, 4.8 x at 200, 3.3 x at 300, 2.3 x at 400, 1.6 x at 458 (C2: 118 against 73 LM
// iterations / s); 2.3 x at 458 x 10 keyframes.  A heuristic of this scene family: nrs_options.embedded_solver = 1 / 2 decide.
// Beyond ~550 nodes per keyframe the launch is bound by its nb^2 tiles, (9 + 0.045 nb^2) us, and the PCG's trial grows by 16 us a node:
// 600 nodes x 20 keyframes 91.4 against 62.6 LM iterations / s, 700 nodes 60.4 against 57.8 (the crossover), 600 x 10 keyframes 165 against 134.
struct KftCost { double kft_ms, pcg_ms; };
inline KftCost kft_cost_model(int K, int nb, int nf_max) {
    const double launch_us = std::max(16.5 + 0.72 * nb, 9.0 + 0.045 * nb * nb);
    const double kft_ms = ((K + 1) / 2) * (nb + 1.0) * launch_us * 1e-3 + 0.05 * K, pcg_ms = (14.0 + 0.016 * std::max(0, nf_max - 500)) * std::pow(K / 20.0, 0.45);
    return KftCost{kft_ms, pcg_ms};
}
// ---- dimensions and limits: ld the padded block dimension (a multiple of KFT_B that holds 3 nf_max + 6), nb = ld / KFT_B, nfm = ld / 3.
// Eligible: every node index fits its key field, the launches fit the device's LDS (k_kft_tgt stages KFT_TC rows of ld doubles, k_kft_step
// its panels: ld > 5120 on gfx950 would fail on every trial) and, where the caller left the choice open, the cost model prefers it
inline KftReason kft_limits(const KftIn& in, int nf_max, KftDims& D) {
    if (nf_max >= KFT_NF_LIMIT) return KFT_BLOCK_BEYOND_KEY;
    if (nf_max < 1) return KFT_NO_FREE_NODE;
    D.ld = ((3 * nf_max + 6 + KFT_B - 1) / KFT_B) * KFT_B; D.nb = D.ld / KFT_B; D.nfm = D.ld / 3;
    if (sizeof(double) * KFT_TC * (size_t)D.ld > in.lds_cap || in.step_lds > in.lds_cap || in.panel_lds > in.lds_cap) return KFT_BEYOND_LDS;
    if (in.embedded_solver == 0) {
        const KftCost t = kft_cost_model(in.K, D.nb, nf_max);
        if (t.kft_ms > t.pcg_ms) return KFT_PCG_CHEAPER;
    }
    return KFT_ELIGIBLE;
}
// the factor is worth its memory (otherwise the PCG stays block-Jacobi).  Sharded: judged on the rank's own nk blocks, and agreed afterwards
inline bool kft_factor_fits(int nk, int ld) { return (size_t)nk * ld * ld * sizeof(double) <= ((size_t)6 << 30); }

// ---- a rank's share.  Sharded, every decision on the structure is taken on the complete window, which every rank uploads; a rank holds the
// blocks of its own keyframes [k_lo, k_hi), the couplings that touch them and the hand-over slots [zlo, zhi); its rows are [own_lo, own_hi)
struct KftShard {
    int k_lo, k_hi, zlo, zhi, own_lo, own_hi;
    bool own(int k) const { return k >= k_lo && k < k_hi; }
};
inline KftShard kft_shard(const KftIn& in) {
    KftShard S;
    S.k_lo = in.sh_k0; S.k_hi = in.sh_k0 + in.sh_nk;               // (the whole window on one GPU)
    S.zlo = std::max(0, S.k_lo - 1); S.zhi = std::min(in.K, S.k_hi + 1);
    S.own_lo = in.pose_grp_ptr[S.k_lo] * ROW_ALIGN; S.own_hi = in.pose_grp_ptr[S.k_hi] * ROW_ALIGN;
    return S;
}
inline int kft_owner(const int* kb, int k) { int r = 0; while (k >= kb[r + 1]) ++r; return r; }

// a damper's four vertices (1c, 2c, 1n, 2n) in terms of keyframes (kk; -1: absent) and compact nodes (cc; -1: absent or fixed); rs: the first
// free one, -1: none
struct KftDamper { const int* v; int kk[4], cc[4], rs; };
inline KftDamper kft_damper(const KftIn& in, const KftNum& N, int q) {
    KftDamper d;
    d.v = in.dm_idx + 4 * (size_t)q; d.rs = -1;
    for (int r = 0; r < 4; ++r) {
        const KftVert t = d.v[r] >= 0 ? N.vert[d.v[r]] : KftVert{-1, -1};
        d.kk[r] = t.k; d.cc[r] = t.c;
        if (d.rs < 0 && d.cc[r] >= 0) d.rs = r;
    }
    return d;
}
static const int KFT_DM_CUR[2] = {0, 1}, KFT_DM_NXT[2] = {2, 3};

// ---- edge entries, first pass: the window-wide decisions.  They read the complete window and nothing of the rank's share, so every rank
// takes them alike: eligible guarantees every spring inside one keyframe and every damper with a free vertex joining two vertex pairs of
// consecutive keyframes k, k + 1
inline KftReason kft_edges_reason(const KftIn& in, const KftNum& N) {
    for (int q = 0; q < in.n_sp; ++q)
        if (N.vert[in.sp_ij[2 * (size_t)q]].k != N.vert[in.sp_ij[2 * (size_t)q + 1]].k) return KFT_SPRING_ACROSS_KEYFRAMES;   // (not a BA window's)
    for (int q = 0; q < in.n_dm; ++q) {
        const KftDamper d = kft_damper(in, N, q);
        if (d.rs < 0) continue;
        if (d.kk[0] >= 0 && d.kk[1] >= 0 && d.kk[0] != d.kk[1]) return KFT_DAMPER_ACROSS_PAIR;
        if (d.kk[2] >= 0 && d.kk[3] >= 0 && d.kk[2] != d.kk[3]) return KFT_DAMPER_ACROSS_PAIR;
        for (int x = 0; x < 2; ++x)
            for (int y = 0; y < 2; ++y) {
                const int a = KFT_DM_CUR[x], b = KFT_DM_NXT[y];
                if (d.cc[a] >= 0 && d.cc[b] >= 0 && d.kk[b] != d.kk[a] + 1) return KFT_DAMPER_NOT_CONSECUTIVE;
            }
    }
    return KFT_ELIGIBLE;
}
// a same-keyframe pair of two different free nodes joins pe under its key
inline void kft_add_pair(std::vector<KftEnt>& pe, int k, int a, int b, uint32_t src) {
    if (a < 0 || b < 0 || a == b) return;
    pe.push_back(KftEnt{kft_key(k, std::max(a, b), std::min(a, b)), src, 0.0});
}
// ---- edge entries, second pass, the springs in edge order: each reads the slot of its free end (the first where both are)
inline void kft_spring_entries(const KftIn& in, const KftNum& N, KftEdges& E) {
    for (int q = 0; q < in.n_sp; ++q) {
        const KftVert i = N.vert[in.sp_ij[2 * (size_t)q]], j = N.vert[in.sp_ij[2 * (size_t)q + 1]];
        const int pos = i.c >= 0 ? in.sp_pos[2 * (size_t)q] : in.sp_pos[2 * (size_t)q + 1];
        if (pos >= 0) kft_add_pair(E.pe, i.k, i.c, j.c, kft_src(KFT_SRC_SPRING, pos));
    }
}
// ---- ... then this rank's damper entries in edge order: the same-keyframe halves behind the springs in pe, the couplings (a of k, b of k + 1)
// in te.  A damper's value is read from the slot of its first free vertex (one GPU: every slot is linearised).  Sharded, that slot is
// linearised by the rank whose rows hold the vertex only: a damper whose vertices lie on two ranks is a boundary damper, and its value
// reaches the other rank through bd_val (all-reduced per factorisation, kft_assemble) -- the same bits as the slot's.  Every rank that sees
// a boundary damper numbers it alike (bd_slot grows by one on each); the rank that holds the vertex keeps its slot there, the others -1
inline void kft_damper_entries(const KftIn& in, const KftNum& N, const KftShard& S, KftEdges& E) {
    for (int q = 0; q < in.n_dm; ++q) {
        const KftDamper d = kft_damper(in, N, q);
        if (d.rs < 0) continue;
        int pos = -1, klo = in.K, khi = -1;
        uint32_t pe_ref = 0, te_ref = 0;
        for (int r = 0; r < 4; ++r) if (d.kk[r] >= 0) { klo = std::min(klo, d.kk[r]); khi = std::max(khi, d.kk[r]); }
        const int row = in.vrow[d.v[d.rs]];
        const bool held = row >= S.own_lo && row < S.own_hi;
        if (in.sh && kft_owner(in.kb, klo) != kft_owner(in.kb, khi)) {
            const int bd = (int)E.bd_slot.size();
            E.bd_slot.push_back(held ? in.dm_pos[4 * (size_t)q + d.rs] : -1);
            pe_ref = kft_src(KFT_SRC_BOUNDARY, bd); te_ref = KFT_BD | (uint32_t)bd; pos = 0;
        } else if (held || !in.sh) {
            pos = in.dm_pos[4 * (size_t)q + d.rs];
            pe_ref = kft_src(KFT_SRC_DAMPER, pos); te_ref = (uint32_t)pos;
        }
        if (pos < 0) continue;                                     // (sharded: a damper of other ranks' keyframes)
        // J = (-w, +w, +w, -w) I on (1c, 2c, 1n, 2n): block (p, q) = sg_p sg_q s I
        if (d.kk[0] >= 0 && d.kk[1] >= 0) kft_add_pair(E.pe, d.kk[0], d.cc[0], d.cc[1], pe_ref);
        if (d.kk[2] >= 0 && d.kk[3] >= 0) kft_add_pair(E.pe, d.kk[2], d.cc[2], d.cc[3], pe_ref);
        for (int x = 0; x < 2; ++x)
            for (int y = 0; y < 2; ++y) {
                const int a = KFT_DM_CUR[x], b = KFT_DM_NXT[y];
                if (d.cc[a] < 0 || d.cc[b] < 0) continue;
                if (!S.own(d.kk[a]) && !S.own(d.kk[b])) continue;  // (sharded: the couplings that touch an own keyframe)
                const bool minus = (x == y);                       // (1c,1n), (2c,2n): - s ; (1c,2n), (2c,1n): + s
                E.te.push_back(KftCpl{kft_key(d.kk[a], d.cc[a], d.cc[b]), (minus ? KFT_TE_MINUS : 0u) | te_ref});
            }
    }
}
inline void kft_edge_entries(const KftIn& in, const KftNum& N, const KftShard& S, KftEdges& E) {
    E.pe.clear(); E.te.clear(); E.bd_slot.clear();
    E.pe.reserve((size_t)in.n_sp + 2 * (size_t)in.n_dm); E.te.reserve(4 * (size_t)in.n_dm);
    kft_spring_entries(in, N, E);
    kft_damper_entries(in, N, S, E);
}

// ---- per-keyframe pair lists.  The skinned observations' pairs (55 per observation: 5 M at C2) are never materialised: per keyframe -- in
// parallel -- a counting pass over (hi, lo) < nf^2, then a placing pass straight into the keyframe's sorted source / weight arrays.  Order
// inside a pair's list: springs and dampers in edge order, then the observations in caller order (the summation order of k_kft_pairs).
// First the two indices by keyframe: the edge entries (small, in edge order) and the observations (sk_of, in caller order)
inline void kft_index_by_keyframe(const KftIn& in, const std::vector<KftEnt>& pe, KftSkinIndex& X) {
    const int K = in.K;
    X.small_ptr.assign(K + 1, 0); X.small.resize(pe.size());
    for (const KftEnt& x : pe) X.small_ptr[kft_key_k(x.key) + 1]++;
    for (int k = 0; k < K; ++k) X.small_ptr[k + 1] += X.small_ptr[k];
    std::vector<size_t> fill(X.small_ptr.begin(), X.small_ptr.end() - 1);
    for (const KftEnt& x : pe) X.small[fill[kft_key_k(x.key)]++] = x;
    X.sk_ptr.assign(K + 1, 0); X.sk_of.resize((size_t)in.n_skin);
    for (int i = 0; i < in.n_skin; ++i) X.sk_ptr[in.sk_pose[i] + 1]++;
    for (int k = 0; k < K; ++k) X.sk_ptr[k + 1] += X.sk_ptr[k];
    std::vector<int> fill_sk(X.sk_ptr.begin(), X.sk_ptr.end() - 1);
    for (int i = 0; i < in.n_skin; ++i) X.sk_of[fill_sk[in.sk_pose[i]]++] = i;
}
// fn(hi * nf + lo, observation, place of one node, place of the other) for every pair of different free nodes of keyframe k's observations.
// (hi and lo from the two indices by value: through std::max / std::min on the array's elements the compiler selects between their
// addresses with a branch that the nodes' order mispredicts, twice the time per pair)
template <class Fn>
inline void kft_each_skin_pair(const KftIn& in, const KftNum& N, const KftSkinIndex& X, int k, Fn&& fn) {
    const size_t nf = (size_t)N.kf_nf[k];
    int cn[SK_MAX];
    for (int q = X.sk_ptr[k]; q < X.sk_ptr[k + 1]; ++q) {
        const int i = X.sk_of[q];
        for (int a = 0; a < SK_MAX; ++a) { const int v = in.sk_node[SK_MAX * (size_t)i + a]; cn[a] = v >= 0 ? N.row_ci[in.vrow[v]] : -1; }
        for (int a = 0; a < SK_MAX; ++a)
            for (int b = a + 1; b < SK_MAX; ++b) {
                const int ca = cn[a], cb = cn[b];
                if (ca < 0 || cb < 0 || ca == cb) continue;
                fn((size_t)(ca > cb ? ca : cb) * nf + (ca > cb ? cb : ca), i, a, b);
            }
    }
}
// one keyframe's lists: its unique pairs in ascending (hi, lo) and every pair's entries (cnt: scratch the caller keeps between keyframes)
inline void kft_keyframe_pairs(const KftIn& in, const KftNum& N, const KftSkinIndex& X, int k, std::vector<int>& cnt, KftKfLists& o) {
    const size_t nf = (size_t)N.kf_nf[k], nkey = nf * nf;
    auto slot = [&](const KftEnt& x) { return (size_t)kft_key_hi(x.key) * nf + kft_key_lo(x.key); };
    cnt.assign(nkey + 1, 0);
    for (size_t q = X.small_ptr[k]; q < X.small_ptr[k + 1]; ++q) cnt[slot(X.small[q]) + 1]++;
    kft_each_skin_pair(in, N, X, k, [&](size_t key, int, int, int) { cnt[key + 1]++; });
    for (size_t key = 0; key < nkey; ++key) {
        if (cnt[key + 1] > 0) { o.pp_id.push_back((uint32_t)kft_key(k, (int)(key / nf), (int)(key % nf))); o.pp_ptr.push_back(cnt[key]); }
        cnt[key + 1] += cnt[key];
    }
    const size_t ne = (size_t)cnt[nkey];
    o.pp_ptr.push_back((int)ne);
    o.pe_src.resize(ne); o.pe_w.resize(ne);
    for (size_t q = X.small_ptr[k]; q < X.small_ptr[k + 1]; ++q) {
        const int at = cnt[slot(X.small[q])]++;
        o.pe_src[at] = X.small[q].src; o.pe_w[at] = X.small[q].w;
    }
    kft_each_skin_pair(in, N, X, k, [&](size_t key, int i, int a, int b) {
        const int at = cnt[key]++;
        o.pe_src[at] = kft_src(KFT_SRC_SKIN, in.sk_slot[i]);
        o.pe_w[at] = in.sk_om[SK_MAX * (size_t)i + a] * in.sk_om[SK_MAX * (size_t)i + b];
    });
}
// the own keyframes' lists (sharded: the others' stay empty), over min(in.threads, K) shares of the keyframes: run(n, fn) calls fn(t, n) for
// every t < n, in any order or at once -- a keyframe's lists depend on nothing another share writes
template <class Run>
inline void kft_pair_lists(const KftIn& in, const KftNum& N, const KftShard& S, const KftSkinIndex& X, std::vector<KftKfLists>& kl, Run&& run) {
    kl.assign(in.K, KftKfLists());
    run(std::min(in.threads, in.K), [&](int ti, int n) {
        std::vector<int> cnt;
        for (int k = (int)((int64_t)in.K * ti / n); k < (int)((int64_t)in.K * (ti + 1) / n); ++k)
            if (S.own(k)) kft_keyframe_pairs(in, N, X, k, cnt, kl[k]);
    });
}
// the keyframes' pairs behind each other; the entries themselves go up keyframe by keyframe (no concatenated host copy): ent_base[k] is where
// keyframe k's start.  False: more entries than pp_ptr's int can address
inline bool kft_concat_pairs(const std::vector<KftKfLists>& kl, KftPairs& P) {
    const int K = (int)kl.size();
    P.ent_base.assign(K + 1, 0); P.pp_id.clear(); P.pp_ptr.clear();
    size_t n_pairs = 0;
    for (int k = 0; k < K; ++k) { n_pairs += kl[k].pp_id.size(); P.ent_base[k + 1] = P.ent_base[k] + kl[k].pe_src.size(); }
    P.pp_id.reserve(n_pairs); P.pp_ptr.reserve(n_pairs + 1);
    for (int k = 0; k < K; ++k) {
        P.pp_id.insert(P.pp_id.end(), kl[k].pp_id.begin(), kl[k].pp_id.end());
        for (size_t q = 0; q + 1 < kl[k].pp_ptr.size(); ++q) P.pp_ptr.push_back((int)P.ent_base[k] + kl[k].pp_ptr[q]);
    }
    P.pp_ptr.push_back((int)P.ent_base[K]);
    return P.ent_base[K] < ((size_t)1 << 31);
}

// ---- temporal couplings: te into key order (equal keys in edge order), the unique pairs (a of k, b of k + 1) with their entries' sources
inline void kft_coupling_pairs(std::vector<KftCpl>& te, KftCouplings& C) {
    std::stable_sort(te.begin(), te.end(), [](const KftCpl& a, const KftCpl& b) { return a.key < b.key; });
    C.tp_key.clear(); C.tp_ptr.clear(); C.te_src.resize(te.size());
    for (size_t i = 0; i < te.size(); ++i) {
        if (i == 0 || te[i].key != te[i - 1].key) { C.tp_key.push_back(te[i].key); C.tp_ptr.push_back((int)i); }
        C.te_src[i] = te[i].src;
    }
    C.tp_ptr.push_back((int)te.size());
}
// ---- coupling lists by the 'to' node, one direction: dir 0 at keyframe k + 1 by b (from a of k), dir 1 at keyframe k by a (from b of k + 1);
// cl_ptr K x (nfm + 1), every list in tp order = ascending (k, a, b): a fixed order
inline void kft_coupling_lists(const KftCouplings& C, int K, int nfm, int dir, std::vector<int>& cl_ptr, std::vector<int>& cl_from, std::vector<int>& cl_tp) {
    const size_t n_tp = C.tp_key.size();
    auto to = [&](uint64_t key) { return dir == 0 ? (size_t)(kft_key_k(key) + 1) * nfm + kft_key_lo(key) : (size_t)kft_key_k(key) * nfm + kft_key_hi(key); };
    cl_ptr.assign((size_t)K * (nfm + 1), 0);
    std::vector<int> cnt((size_t)K * nfm, 0);
    for (size_t i = 0; i < n_tp; ++i) cnt[to(C.tp_key[i])]++;
    int run = 0;
    for (int k = 0; k < K; ++k) {
        for (int n = 0; n < nfm; ++n) { cl_ptr[(size_t)k * (nfm + 1) + n] = run; run += cnt[(size_t)k * nfm + n]; }
        cl_ptr[(size_t)k * (nfm + 1) + nfm] = run;
    }
    cl_from.assign(n_tp + 1, 0); cl_tp.assign(n_tp + 1, 0);
    std::vector<int> fill((size_t)K * nfm);
    for (int k = 0; k < K; ++k) for (int n = 0; n < nfm; ++n) fill[(size_t)k * nfm + n] = cl_ptr[(size_t)k * (nfm + 1) + n];
    for (size_t i = 0; i < n_tp; ++i) {
        const int q = fill[to(C.tp_key[i])]++;
        cl_from[q] = dir == 0 ? kft_key_hi(C.tp_key[i]) : kft_key_lo(C.tp_key[i]); cl_tp[q] = (int)i;
    }
}

// ---- the one device buffer: its regions in order, every one 256-byte aligned, every size stated once (kft_layout)
enum KftRegion {
    KR_A, KR_YT, KR_Bb, KR_Cb, KR_Pv, KR_z, KR_xs, KR_vb, KR_kf_nf, KR_kf_np, KR_kf_row, KR_row_ci, KR_pp_id, KR_pp_ptr, KR_pe_src, KR_pe_w,
    KR_tp_ptr, KR_te_src, KR_tp_val, KR_cl_ptr0, KR_cl_ptr1, KR_cl_from0, KR_cl_from1, KR_cl_tp0, KR_cl_tp1, KR_cl_val0, KR_cl_val1,
    KR_bd_slot, KR_bd_buf, KR_pose_ws, KR_rn, KR_COUNT
};
struct KftLayout {
    size_t off[KR_COUNT], bytes[KR_COUNT], total = 0;
    bool zeroed[KR_COUNT];                                         // cleared at set-up: z, xs, vb; bd_buf, pose_ws, rn
    size_t end(int r) const { return r + 1 < KR_COUNT ? off[r + 1] : off[r] + bytes[r]; }   // (with the padding up to the next region, where there is one)
    template <class T> T* at(char* base, int r) const { return reinterpret_cast<T*>(base + off[r]); }
};
// (nk own blocks, nz hand-over vectors; the list sizes are this rank's)
inline KftLayout kft_layout(const KftIn& in, const KftShard& S, const KftDims& dim, const KftPairs& P, const KftCouplings& C, size_t n_bd) {
    struct { size_t nk, nz, ld, nb, nfm, n_rows, n_pp, n_pe, n_tp, n_te, n_bd; bool sh; } const n = {
        (size_t)(S.k_hi - S.k_lo), (size_t)(S.zhi - S.zlo), (size_t)dim.ld, (size_t)dim.nb, (size_t)dim.nfm, (size_t)in.n_rows,
        P.pp_id.size(), P.ent_base[in.K], C.tp_key.size(), C.te_src.size(), n_bd, in.sh};
    const size_t n2 = n.ld * n.ld, tile = (size_t)KFT_B * KFT_B, K = (size_t)in.K;
    const size_t I = 4, D = 8;                                     // bytes of an int / uint32_t, of a double
    const struct { KftRegion r; size_t bytes; bool zero; } table[KR_COUNT] = {
        {KR_A, D * n.nk * n2, false}, {KR_YT, D * 2 * n2, false}, {KR_Bb, D * 4 * n.nb * tile, false}, {KR_Cb, D * 4 * n.nb * tile, false}, {KR_Pv, D * 4 * tile, false},
        {KR_z, D * n.nz * n.ld, true}, {KR_xs, D * n.nz * n.ld, true}, {KR_vb, D * 2 * n.ld, true},
        {KR_kf_nf, I * K, false}, {KR_kf_np, I * K, false}, {KR_kf_row, I * K * n.nfm, false}, {KR_row_ci, I * n.n_rows, false},
        {KR_pp_id, I * (n.n_pp + 1), false}, {KR_pp_ptr, I * (n.n_pp + 1), false}, {KR_pe_src, I * (n.n_pe + 1), false}, {KR_pe_w, D * (n.n_pe + 1), false},
        {KR_tp_ptr, I * (n.n_tp + 1), false}, {KR_te_src, I * (n.n_te + 1), false}, {KR_tp_val, D * (n.n_tp + 1), false},
        {KR_cl_ptr0, I * K * (n.nfm + 1), false}, {KR_cl_ptr1, I * K * (n.nfm + 1), false}, {KR_cl_from0, I * (n.n_tp + 1), false}, {KR_cl_from1, I * (n.n_tp + 1), false},
        {KR_cl_tp0, I * (n.n_tp + 1), false}, {KR_cl_tp1, I * (n.n_tp + 1), false}, {KR_cl_val0, D * (n.n_tp + 1), false}, {KR_cl_val1, D * (n.n_tp + 1), false},
        {KR_bd_slot, I * (n.n_bd + 1), false}, {KR_bd_buf, D * 2 * (n.n_bd + 1), true}, {KR_pose_ws, n.sh ? D * 12 * K : 0, true}, {KR_rn, D * 4, true}};
    KftLayout L;
    for (int i = 0; i < KR_COUNT; ++i) {
        L.off[table[i].r] = L.total; L.bytes[table[i].r] = table[i].bytes; L.zeroed[table[i].r] = table[i].zero;
        L.total += (table[i].bytes + 255) & ~(size_t)255;
    }
    return L;
}
// what set-up clears, as runs of neighbouring zeroed regions: (offset, bytes) each
struct KftSpan { size_t off, bytes; };
inline std::vector<KftSpan> kft_zero_spans(const KftLayout& L) {
    std::vector<KftSpan> z;
    for (int r = 0; r < KR_COUNT; ++r) {
        if (!L.zeroed[r]) continue;
        if (r > 0 && L.zeroed[r - 1]) z.back().bytes = L.end(r) - z.back().off;
        else z.push_back(KftSpan{L.off[r], L.end(r) - L.off[r]});
    }
    return z;
}
// what set-up uploads: `bytes` from src to `at` bytes into region r (the entries of the pair lists go up keyframe by keyframe)
struct KftUpload { KftRegion r; size_t at; const void* src; size_t bytes; };
inline std::vector<KftUpload> kft_uploads(const KftNum& N, const std::vector<KftKfLists>& kl, const KftPairs& P, const KftCouplings& C, const std::vector<int>& bd_slot) {
    const size_t n_tp = C.tp_key.size();
    std::vector<KftUpload> u = {
        {KR_kf_nf, 0, N.kf_nf.data(), 4 * N.kf_nf.size()}, {KR_kf_np, 0, N.kf_np.data(), 4 * N.kf_np.size()}, {KR_kf_row, 0, N.kf_row.data(), 4 * N.kf_row.size()},
        {KR_row_ci, 0, N.row_ci.data(), 4 * N.row_ci.size()}, {KR_pp_id, 0, P.pp_id.data(), 4 * P.pp_id.size()}, {KR_pp_ptr, 0, P.pp_ptr.data(), 4 * P.pp_ptr.size()}};
    for (size_t k = 0; k < kl.size(); ++k) {
        u.push_back(KftUpload{KR_pe_src, 4 * P.ent_base[k], kl[k].pe_src.data(), 4 * kl[k].pe_src.size()});
        u.push_back(KftUpload{KR_pe_w, 8 * P.ent_base[k], kl[k].pe_w.data(), 8 * kl[k].pe_w.size()});
    }
    u.insert(u.end(), {{KR_tp_ptr, 0, C.tp_ptr.data(), 4 * C.tp_ptr.size()}, {KR_te_src, 0, C.te_src.data(), 4 * C.te_src.size()},
                       {KR_cl_ptr0, 0, C.cl_ptr[0].data(), 4 * C.cl_ptr[0].size()}, {KR_cl_ptr1, 0, C.cl_ptr[1].data(), 4 * C.cl_ptr[1].size()},
                       {KR_cl_from0, 0, C.cl_from[0].data(), 4 * n_tp}, {KR_cl_from1, 0, C.cl_from[1].data(), 4 * n_tp},
                       {KR_cl_tp0, 0, C.cl_tp[0].data(), 4 * n_tp}, {KR_cl_tp1, 0, C.cl_tp[1].data(), 4 * n_tp}, {KR_bd_slot, 0, bd_slot.data(), 4 * bd_slot.size()}});
    return u;
}

}  // namespace nrs
