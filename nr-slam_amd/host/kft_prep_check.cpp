// Stand-alone check of the host stages of the keyframe-block factorisation's set-up (csrc/nrs_kft_prep_host.hpp) for a sanitizer build:
// `make kft_prep_check && ./kft_prep_check`.  Hand-made windows of 1-5 keyframes and at most a dozen nodes each go through the stages in
// the driver's order (nrs_engine_kft_setup.hpp kft_setup), one GPU and as every rank of worlds 2 and 3; the uploads go into a host image of
// the device buffer, and what is read back from it is held to a brute-force restatement over ordered maps, written here without the
// stages' counting and placing.  No HIP, no library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <thread>
#include <tuple>
#include <utility>
#include "../csrc/nrs_kft_prep_host.hpp"

using namespace nrs;
typedef std::vector<int> VI;
typedef std::tuple<int, int, int> Key;                              // (k, hi, lo) of a pair list; (k, a, b) of a coupling
typedef std::pair<uint32_t, double> Ent;                            // (src, w)

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "kft_prep_check: %s:%d: %s\n", __FILE__, __LINE__, #x); std::abort(); } } while (0)

// a window: one ROW_ALIGN group per keyframe, every row fixed (padding) until a vertex sits on it
struct Win {
    int K;
    VI grp, lm_pose, vrow, sp, dm, sk_pose, sk_node;
    std::vector<uint8_t> rflag, pose_fixed;
    std::vector<double> sk_om;
    explicit Win(int K_) : K(K_), grp(K_ + 1), rflag((size_t)K_ * ROW_ALIGN, RF_FIXED), pose_fixed(K_, 0) { for (int k = 0; k <= K; ++k) grp[k] = k; }
    int vtx(int k, int row, bool fixed = false) {
        lm_pose.push_back(k); vrow.push_back(k * ROW_ALIGN + row);
        rflag[(size_t)k * ROW_ALIGN + row] = fixed ? RF_FIXED : RF_OBS;
        return (int)lm_pose.size() - 1;
    }
    void spring(int i, int j) { sp.push_back(i); sp.push_back(j); }
    void damper(int c1, int c2, int n1, int n2) { dm.push_back(c1); dm.push_back(c2); dm.push_back(n1); dm.push_back(n2); }
    void obs(int k, std::initializer_list<std::pair<int, int>> nodes) {   // (vertex, weight in 16ths)
        size_t n = 0;
        sk_pose.push_back(k);
        for (const auto& x : nodes) { sk_node.push_back(x.first); sk_om.push_back(x.second / 16.0); ++n; }
        for (; n < (size_t)SK_MAX; ++n) { sk_node.push_back(-1); sk_om.push_back(0.0); }
    }
    bool free_v(int v) const { return !(rflag[vrow[v]] & RF_FIXED); }
};
// whose view: one GPU, or rank `rank` of `world` with the keyframe ranges kb
struct Rank {
    bool sh; int world, rank; VI kb;
    int k_lo() const { return kb[rank]; }
    int k_hi() const { return kb[rank + 1]; }
    bool own(int k) const { return k >= k_lo() && k < k_hi(); }
    int owner(int k) const { int r = 0; while (k >= kb[r + 1]) ++r; return r; }
};
static Rank one_gpu(const Win& W) { return Rank{false, 1, 0, {0, W.K}}; }
// the engine's incidence slots as this rank has them: a number per (edge, incidence) whatever the rank, -1 on fixed rows and on rows of other ranks
static int sp_slot(int q, int r) { return 100 + 2 * q + r; }
static int dm_slot(int q, int r) { return 1000 + 4 * q + r; }
static int sk_slot_of(int i) { return 500 + i; }
struct View { KftIn in; VI sp_pos, dm_pos, sk_slot; };
static void make_view(const Win& W, const Rank& R, int threads, View& V) {
    auto slot_ok = [&](int v) { return v >= 0 && W.free_v(v) && R.own(W.lm_pose[v]); };
    for (size_t i = 0; i < W.sp.size(); ++i) V.sp_pos.push_back(slot_ok(W.sp[i]) ? sp_slot((int)i / 2, (int)i % 2) : -1);
    for (size_t i = 0; i < W.dm.size(); ++i) V.dm_pos.push_back(W.dm[i] >= 0 && W.free_v(W.dm[i]) ? dm_slot((int)i / 4, (int)i % 4) : -1);   // (known on every rank: the stage must not rely on -1)
    for (size_t i = 0; i < W.sk_pose.size(); ++i) V.sk_slot.push_back(R.own(W.sk_pose[i]) ? sk_slot_of((int)i) : -1);
    KftIn& in = V.in;
    in.K = W.K; in.n_rows = (int)W.rflag.size(); in.pose_grp_ptr = W.grp.data(); in.rflag = W.rflag.data(); in.pose_fixed = W.pose_fixed.data();
    in.M = (int)W.lm_pose.size(); in.lm_pose = W.lm_pose.data(); in.vrow = W.vrow.data();
    in.n_sp = (int)W.sp.size() / 2; in.sp_ij = W.sp.data(); in.sp_pos = V.sp_pos.empty() ? nullptr : V.sp_pos.data();
    in.n_dm = (int)W.dm.size() / 4; in.dm_idx = W.dm.data(); in.dm_pos = V.dm_pos.data();
    in.n_skin = (int)W.sk_pose.size(); in.sk_pose = W.sk_pose.data(); in.sk_node = W.sk_node.data(); in.sk_om = W.sk_om.data(); in.sk_slot = V.sk_slot.data();
    in.sh = R.sh; in.world = R.world; in.sh_k0 = R.k_lo(); in.sh_nk = R.k_hi() - R.k_lo(); in.kb = R.kb.data();
    in.embedded_solver = 1; in.lds_cap = 160 * 1024; in.step_lds = 140 * 1024; in.panel_lds = 70 * 1024; in.threads = threads;
}

// ---- the stages in the driver's order; the lists as the device would see them, read back from a host image of the buffer
struct Built {
    KftNum num; KftDims dim; KftShard sd; KftEdges ed; KftSkinIndex ix; std::vector<KftKfLists> kl; KftPairs pairs; KftCouplings cpl; KftLayout lay;
    std::vector<char> buf;
    std::map<Key, std::vector<Ent>> pair_lists;                     // (k, hi, lo) -> entries in list order
    std::map<Key, std::vector<uint32_t>> couplings;                 // (k, a, b) -> sources in list order
};
static void run_threads(int nt, const std::function<void(int, int)>& fn) {
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back([&fn, t, nt] { fn(t, nt); });
    fn(0, nt);
    for (auto& x : th) x.join();
}
struct Counts { int K, nk, nz, ld, nb, n_rows, nfm; size_t n_pp, n_pe, n_tp, n_te, n_bd; bool sh; };
static void check_layout(const Built& B, const Counts& n);
static KftReason build(const View& V, Built& B) {
    const KftIn& in = V.in;
    KftReason why = kft_window_reason(in);
    if (why != KFT_ELIGIBLE) return why;
    kft_number_rows(in, B.num);
    if ((why = kft_limits(in, B.num.nf_max, B.dim)) != KFT_ELIGIBLE) return why;
    B.sd = kft_shard(in);
    kft_rows_of_nodes(in, B.dim.nfm, B.num);
    kft_vertex_table(in, B.num);
    if ((why = kft_edges_reason(in, B.num)) != KFT_ELIGIBLE) return why;
    kft_edge_entries(in, B.num, B.sd, B.ed);
    kft_index_by_keyframe(in, B.ed.pe, B.ix);
    kft_pair_lists(in, B.num, B.sd, B.ix, B.kl, [](int nt, auto&& fn) { run_threads(nt, fn); });
    CHECK(kft_concat_pairs(B.kl, B.pairs));
    kft_coupling_pairs(B.ed.te, B.cpl);
    for (int dir = 0; dir < 2; ++dir) kft_coupling_lists(B.cpl, in.K, B.dim.nfm, dir, B.cpl.cl_ptr[dir], B.cpl.cl_from[dir], B.cpl.cl_tp[dir]);
    Counts n;                                                       // (the restatement's own: what check_layout sizes the regions from)
    n.K = in.K; n.nk = B.sd.k_hi - B.sd.k_lo; n.nz = B.sd.zhi - B.sd.zlo; n.ld = B.dim.ld; n.nb = B.dim.nb; n.n_rows = in.n_rows; n.nfm = B.dim.nfm;
    n.n_pp = B.pairs.pp_id.size(); n.n_pe = B.pairs.ent_base[in.K]; n.n_tp = B.cpl.tp_key.size(); n.n_te = B.cpl.te_src.size(); n.n_bd = B.ed.bd_slot.size();
    n.sh = in.sh;
    B.lay = kft_layout(in, B.sd, B.dim, B.pairs, B.cpl, B.ed.bd_slot.size());
    check_layout(B, n);
    // the image: poisoned, the uploads, the cleared spans (a write outside the image is the sanitizer's to report)
    B.buf.assign(B.lay.total, (char)0xAB);
    for (const KftUpload& u : kft_uploads(B.num, B.kl, B.pairs, B.cpl, B.ed.bd_slot)) {
        CHECK(u.at + u.bytes <= B.lay.bytes[u.r]);                  // (a region is at least as large as what goes into it)
        if (u.bytes) memcpy(B.buf.data() + B.lay.off[u.r] + u.at, u.src, u.bytes);
    }
    for (const KftSpan& z : kft_zero_spans(B.lay)) { CHECK(z.off + z.bytes <= B.lay.total); memset(B.buf.data() + z.off, 0, z.bytes); }
    char* base = B.buf.data();
    const uint32_t* pp_id = B.lay.at<uint32_t>(base, KR_pp_id); const int* pp_ptr = B.lay.at<int>(base, KR_pp_ptr);
    const uint32_t* pe_src = B.lay.at<uint32_t>(base, KR_pe_src); const double* pe_w = B.lay.at<double>(base, KR_pe_w);
    for (size_t i = 0; i < n.n_pp; ++i) {
        const Key key(kft_key_k(pp_id[i]), kft_key_hi(pp_id[i]), kft_key_lo(pp_id[i]));
        CHECK(!B.pair_lists.count(key) && pp_ptr[i] < pp_ptr[i + 1]);
        if (i) CHECK(pp_id[i - 1] < pp_id[i]);
        for (int q = pp_ptr[i]; q < pp_ptr[i + 1]; ++q) B.pair_lists[key].push_back(Ent(pe_src[q], pe_w[q]));
    }
    CHECK(pp_ptr[0] == 0 && pp_ptr[n.n_pp] == (int)n.n_pe);
    const int* tp_ptr = B.lay.at<int>(base, KR_tp_ptr); const uint32_t* te_src = B.lay.at<uint32_t>(base, KR_te_src);
    for (size_t i = 0; i < n.n_tp; ++i) {
        const uint64_t k = B.cpl.tp_key[i];
        if (i) CHECK(B.cpl.tp_key[i - 1] < k);
        CHECK(tp_ptr[i] < tp_ptr[i + 1]);
        for (int q = tp_ptr[i]; q < tp_ptr[i + 1]; ++q) B.couplings[Key(kft_key_k(k), kft_key_hi(k), kft_key_lo(k))].push_back(te_src[q]);
    }
    CHECK(tp_ptr[n.n_tp] == (int)n.n_te);
    return KFT_ELIGIBLE;
}

// ---- layout: disjoint, aligned, inside the total, in the order and at the offsets of the one expression the set-up used to take them in;
// the cleared spans are exactly z, xs, vb and bd_buf, pose_ws, rn
static void check_layout(const Built& B, const Counts& n) {
    const KftLayout& L = B.lay;
    const size_t n2 = (size_t)n.ld * n.ld, tile = (size_t)KFT_B * KFT_B, K = n.K, n_tp = n.n_tp;
    const size_t was[KR_COUNT] = {8 * (size_t)n.nk * n2, 8 * 2 * n2, 8 * 4 * n.nb * tile, 8 * 4 * n.nb * tile, 8 * 4 * tile, 8 * (size_t)n.nz * n.ld, 8 * (size_t)n.nz * n.ld,
        8 * 2 * (size_t)n.ld, 4 * K, 4 * K, 4 * K * n.nfm, 4 * (size_t)n.n_rows, 4 * (n.n_pp + 1), 4 * (n.n_pp + 1), 4 * (n.n_pe + 1), 8 * (n.n_pe + 1), 4 * (n_tp + 1),
        4 * (n.n_te + 1), 8 * (n_tp + 1), 4 * K * (n.nfm + 1), 4 * K * (n.nfm + 1), 4 * (n_tp + 1), 4 * (n_tp + 1), 4 * (n_tp + 1), 4 * (n_tp + 1), 8 * (n_tp + 1), 8 * (n_tp + 1),
        4 * (n.n_bd + 1), 8 * 2 * (n.n_bd + 1), n.sh ? 8 * 12 * K : 0, 8 * 4};
    size_t off = 0;
    for (int r = 0; r < KR_COUNT; ++r) {
        CHECK(L.off[r] == off && L.off[r] % 256 == 0 && L.bytes[r] == was[r] && L.off[r] + L.bytes[r] <= L.end(r));
        off += (was[r] + 255) & ~(size_t)255;
    }
    CHECK(L.total == off);
    const std::set<int> named = {KR_z, KR_xs, KR_vb, KR_bd_buf, KR_pose_ws, KR_rn};
    std::vector<char> hit(L.total, 0);
    for (const KftSpan& z : kft_zero_spans(L)) for (size_t b = z.off; b < z.off + z.bytes; ++b) { CHECK(b < L.total && !hit[b]); hit[b] = 1; }
    for (int r = 0; r < KR_COUNT; ++r) {
        CHECK(L.zeroed[r] == (named.count(r) > 0));
        for (size_t b = L.off[r]; b < L.off[r] + L.bytes[r]; ++b) CHECK(hit[b] == (named.count(r) ? 1 : 0));
    }
    const std::vector<KftSpan> z = kft_zero_spans(L);                // the two clears set-up has always made: z up to kf_nf, bd_buf up to rn's 32 bytes
    CHECK(z.size() == 2 && z[0].off == L.off[KR_z] && z[0].off + z[0].bytes == L.off[KR_kf_nf] && z[1].off == L.off[KR_bd_buf] && z[1].off + z[1].bytes == L.off[KR_rn] + 32);
}

// ---- the brute-force restatement: what rank R's lists must be
struct Expect {
    VI row_ci, kf_nf;
    std::map<Key, std::vector<Ent>> pair_lists;
    std::map<Key, std::vector<uint32_t>> couplings;
    VI bd_slot;
};
static Expect expect(const Win& W, const Rank& R, const View& V) {
    Expect E;
    E.row_ci.assign(W.rflag.size(), -1); E.kf_nf.assign(W.K, 0);
    for (size_t r = 0; r < W.rflag.size(); ++r) if (!(W.rflag[r] & RF_FIXED)) E.row_ci[r] = E.kf_nf[r / ROW_ALIGN]++;
    auto node = [&](int v) { return v >= 0 ? E.row_ci[W.vrow[v]] : -1; };
    auto pair = [&](int k, int va, int vb, uint32_t src, double w) {
        const int a = node(va), b = node(vb);
        if (a < 0 || b < 0 || a == b || !R.own(k)) return;
        E.pair_lists[Key(k, std::max(a, b), std::min(a, b))].push_back(Ent(src, w));
    };
    for (size_t q = 0; q < W.sp.size() / 2; ++q) {
        const int i = W.sp[2 * q], j = W.sp[2 * q + 1];
        const int slot = W.free_v(i) ? V.sp_pos[2 * q] : V.sp_pos[2 * q + 1];
        if (slot >= 0) pair(W.lm_pose[i], i, j, (0u << 30) | (uint32_t)slot, 0.0);
    }
    for (size_t q = 0; q < W.dm.size() / 4; ++q) {
        const int* v = &W.dm[4 * q];
        int first = -1, klo = W.K, khi = -1;
        for (int r = 0; r < 4; ++r) {
            if (v[r] >= 0) { klo = std::min(klo, W.lm_pose[v[r]]); khi = std::max(khi, W.lm_pose[v[r]]); }
            if (first < 0 && node(v[r]) >= 0) first = r;
        }
        if (first < 0) continue;
        uint32_t psrc, tsrc;
        const bool held = R.own(W.lm_pose[v[first]]);               // (the rank that linearises the first free vertex's slot)
        if (R.sh && R.owner(klo) != R.owner(khi)) {
            psrc = (3u << 30) | (uint32_t)E.bd_slot.size(); tsrc = KFT_BD | (uint32_t)E.bd_slot.size();
            E.bd_slot.push_back(held ? V.dm_pos[4 * q + first] : -1);
        } else {
            if (!held) continue;
            psrc = (1u << 30) | (uint32_t)V.dm_pos[4 * q + first]; tsrc = (uint32_t)V.dm_pos[4 * q + first];
        }
        if (v[0] >= 0 && v[1] >= 0) pair(W.lm_pose[v[0]], v[0], v[1], psrc, 0.0);
        if (v[2] >= 0 && v[3] >= 0) pair(W.lm_pose[v[2]], v[2], v[3], psrc, 0.0);
        for (int c = 0; c < 2; ++c)
            for (int x = 2; x < 4; ++x) {
                if (node(v[c]) < 0 || node(v[x]) < 0) continue;
                const int k = W.lm_pose[v[c]];
                if (!R.own(k) && !R.own(k + 1)) continue;
                E.couplings[Key(k, node(v[c]), node(v[x]))].push_back((x - 2 == c ? 0x80000000u : 0u) | tsrc);
            }
    }
    for (size_t i = 0; i < W.sk_pose.size(); ++i)
        for (int a = 0; a < SK_MAX; ++a)
            for (int b = a + 1; b < SK_MAX; ++b)
                pair(W.sk_pose[i], W.sk_node[SK_MAX * i + a], W.sk_node[SK_MAX * i + b], (2u << 30) | (uint32_t)V.sk_slot[i], W.sk_om[SK_MAX * i + a] * W.sk_om[SK_MAX * i + b]);
    return E;
}
// one rank's stages against the restatement; the coupling lists by the 'to' node against the couplings themselves
static void check_rank(const Win& W, const Rank& R, int threads, Built& B) {
    View V;
    make_view(W, R, threads, V);
    CHECK(build(V, B) == KFT_ELIGIBLE);
    const Expect E = expect(W, R, V);
    CHECK(B.num.row_ci == E.row_ci && B.num.kf_nf == E.kf_nf);
    for (int k = 0; k < W.K; ++k) {
        CHECK(B.num.kf_np[k] == (W.pose_fixed[k] ? 0 : 6));
        for (int n = 0; n < B.dim.nfm; ++n) {
            const int r = B.num.kf_row[(size_t)k * B.dim.nfm + n];
            CHECK(n < E.kf_nf[k] ? (r / ROW_ALIGN == k && E.row_ci[r] == n) : r == -1);
        }
    }
    CHECK(B.dim.ld % KFT_B == 0 && B.dim.ld >= 3 * B.num.nf_max + 6 && B.dim.ld < 3 * B.num.nf_max + 6 + KFT_B && B.dim.nb * KFT_B == B.dim.ld && B.dim.nfm == B.dim.ld / 3);
    CHECK(B.pair_lists == E.pair_lists);
    CHECK(B.couplings == E.couplings);
    CHECK(B.ed.bd_slot == E.bd_slot);
    for (const auto& x : B.pair_lists) CHECK(R.own(std::get<0>(x.first)));
    // by 'to': dir 0 the node b of keyframe k + 1 lists (a, coupling) in ascending (k, a, b); dir 1 the node a of keyframe k lists (b, coupling)
    for (int dir = 0; dir < 2; ++dir) {
        std::map<std::pair<int, int>, std::vector<std::pair<int, int>>> want;   // (keyframe, to) -> (from, coupling index)
        int i = 0;
        for (const auto& x : E.couplings) {
            const int k = std::get<0>(x.first), a = std::get<1>(x.first), b = std::get<2>(x.first);
            if (dir == 0) want[{k + 1, b}].push_back({a, i}); else want[{k, a}].push_back({b, i});
            ++i;
        }
        const int* cl_ptr = B.lay.at<int>(B.buf.data(), KR_cl_ptr0 + dir); const int* cl_from = B.lay.at<int>(B.buf.data(), KR_cl_from0 + dir);
        const int* cl_tp = B.lay.at<int>(B.buf.data(), KR_cl_tp0 + dir);
        int at = 0;
        for (int k = 0; k < W.K; ++k)
            for (int n = 0; n <= B.dim.nfm; ++n) {
                CHECK(cl_ptr[(size_t)k * (B.dim.nfm + 1) + n] == at);
                if (n == B.dim.nfm || !want.count({k, n})) continue;
                for (const auto& fe : want[{k, n}]) { CHECK(cl_from[at] == fe.first && cl_tp[at] == fe.second); ++at; }
            }
        CHECK(at == (int)E.couplings.size());
    }
}

// ---- the windows
// five keyframes of six vertices on rows with padding between them; keyframe 4 has no free node
static Win big_window(VI* vout = nullptr) {
    Win W(5);
    VI v;
    const int rows[6] = {0, 2, 3, 7, 9, 12};
    for (int k = 0; k < 5; ++k)
        for (int j = 0; j < 6; ++j) v.push_back(W.vtx(k, rows[j], k == 4 || (k == 1 && j == 2) || (k == 2 && j == 0)));   // fixed: all of keyframe 4, (1, 2), (2, 0)
    auto V = [&](int k, int j) { return v[6 * k + j]; };
    W.pose_fixed[0] = 1;
    for (int k = 0; k < 5; ++k) { W.spring(V(k, 0), V(k, 1)); W.spring(V(k, 3), V(k, 1)); W.spring(V(k, 1), V(k, 0)); W.spring(V(k, 4), V(k, 5)); }
    W.spring(V(1, 2), V(1, 3));                                     // one end fixed: nothing to couple
    W.spring(V(4, 0), V(4, 1));                                     // both ends fixed
    for (int k = 0; k + 1 < 5; ++k) {
        W.damper(V(k, 0), V(k, 1), V(k + 1, 0), V(k + 1, 1));
        W.damper(V(k, 1), V(k, 3), V(k + 1, 1), V(k + 1, 3));
        W.damper(V(k, 1), V(k, 0), V(k + 1, 1), V(k + 1, 0));       // the same pairs again, the other way round: lists of two
        W.damper(V(k, 4), -1, V(k + 1, 4), V(k + 1, 5));            // an absent vertex
        W.damper(V(k, 2), V(k, 5), V(k + 1, 2), V(k + 1, 5));
    }
    W.damper(-1, -1, V(0, 3), V(0, 4));                             // no current pair at all
    W.damper(V(4, 0), V(4, 1), -1, -1);                             // every vertex fixed
    W.damper(V(2, 0), V(2, 1), V(3, 0), V(3, 1));                   // first vertex fixed: the slot is the second's
    for (int k = 0; k < 5; ++k) {
        W.obs(k, {{V(k, 0), 4}, {V(k, 1), 4}, {V(k, 2), 8}});
        W.obs(k, {{V(k, 1), 2}, {V(k, 3), 6}, {V(k, 1), 3}, {V(k, 5), 5}});   // a node named twice: that pair is skipped
        W.obs(k, {{V(k, 0), 1}, {V(k, 1), 2}, {V(k, 2), 3}, {V(k, 3), 1}, {V(k, 4), 2}, {V(k, 5), 3}, {V(k, 0), 1}, {V(k, 1), 1}, {V(k, 2), 1}, {V(k, 3), 1}, {V(k, 4), 1}});
    }
    W.obs(0, {{V(0, 5), 16}});                                      // one node: no pair
    if (vout) *vout = v;
    return W;
}
static KftReason reason_of(const Win& W, const Rank& R) { View V; make_view(W, R, 1, V); Built B; return build(V, B); }

static void check_one_gpu() {
    Win W1(1);
    VI a;
    for (int j = 0; j < 6; ++j) a.push_back(W1.vtx(0, 2 * j + (j > 2), j == 3));
    W1.spring(a[0], a[1]); W1.spring(a[2], a[1]); W1.spring(a[3], a[4]); W1.damper(-1, -1, a[0], a[5]);
    W1.obs(0, {{a[0], 8}, {a[3], 4}, {a[5], 4}});
    Built B1; check_rank(W1, one_gpu(W1), 1, B1);
    CHECK(B1.pair_lists.size() == 3 && B1.couplings.empty());
    Win W2(2);
    VI b;
    for (int k = 0; k < 2; ++k) for (int j = 0; j < 3; ++j) b.push_back(W2.vtx(k, 5 * j + 1));
    W2.pose_fixed[1] = 1;
    W2.spring(b[0], b[1]); W2.spring(b[4], b[5]); W2.damper(b[0], b[1], b[3], b[4]); W2.damper(b[1], b[2], b[4], b[5]);
    Built B2; check_rank(W2, one_gpu(W2), 1, B2);
    CHECK(B2.num.kf_np[0] == 6 && B2.num.kf_np[1] == 0 && B2.couplings.size() == 7);
    const Win W = big_window();
    Built B, B3; check_rank(W, one_gpu(W), 1, B); check_rank(W, one_gpu(W), 3, B3);
    CHECK(B.num.kf_nf == (VI{6, 5, 5, 6, 0}));
    // springs 20 (one end fixed) and 21 (both): no entry reads either of their slots, the free end's included
    for (const KftEnt& x : B.ed.pe)
        for (int q = 20; q < 22; ++q) CHECK(x.src != kft_src(KFT_SRC_SPRING, sp_slot(q, 0)) && x.src != kft_src(KFT_SRC_SPRING, sp_slot(q, 1)));
    CHECK(W.sp.size() / 2 == 22 && !W.free_v(W.sp[40]) && W.free_v(W.sp[41]) && !W.free_v(W.sp[42]) && !W.free_v(W.sp[43]));
    CHECK(B.buf == B3.buf);                                         // thread counts 1 and 3: the same image
    for (int k = 0; k < W.K; ++k) CHECK(B.kl[k].pp_id == B3.kl[k].pp_id && B.kl[k].pp_ptr == B3.kl[k].pp_ptr && B.kl[k].pe_src == B3.kl[k].pe_src && B.kl[k].pe_w == B3.kl[k].pe_w);
}

// every reason, once, and alike on every rank
static void check_reasons() {
    VI v;
    const Rank ranks[3] = {one_gpu(big_window()), Rank{true, 2, 0, {0, 2, 5}}, Rank{true, 2, 1, {0, 2, 5}}};
    auto V = [&](int k, int j) { return v[6 * k + j]; };
    for (const Rank& R : ranks) {
        Win A = big_window(&v); A.spring(V(0, 0), V(1, 0));
        CHECK(reason_of(A, R) == KFT_SPRING_ACROSS_KEYFRAMES);
        Win B = big_window(&v); B.damper(V(0, 0), V(1, 1), V(1, 0), V(1, 3));
        CHECK(reason_of(B, R) == KFT_DAMPER_ACROSS_PAIR);
        Win C = big_window(&v); C.damper(V(0, 0), V(0, 1), V(2, 1), V(2, 3));
        CHECK(reason_of(C, R) == KFT_DAMPER_NOT_CONSECUTIVE);
        Win D = big_window(&v); D.damper(V(4, 0), V(4, 1), V(2, 1), V(2, 3));    // the current pair is fixed: nothing couples, still eligible
        CHECK(reason_of(D, R) == KFT_ELIGIBLE);
    }
    View X; make_view(big_window(), ranks[0], 1, X);
    KftDims D;
    KftIn in = X.in;
    CHECK(kft_limits(in, KFT_NF_LIMIT, D) == KFT_BLOCK_BEYOND_KEY && kft_limits(in, 0, D) == KFT_NO_FREE_NODE);
    CHECK(kft_limits(in, KFT_NF_LIMIT - 1, D) == KFT_BEYOND_LDS && kft_limits(in, 1705, D) == KFT_BEYOND_LDS && kft_limits(in, 1704, D) == KFT_ELIGIBLE && D.ld == 5120);   // (32 ld bytes against 160 KB)
    in.lds_cap = (size_t)1 << 30;
    CHECK(kft_limits(in, KFT_NF_LIMIT - 1, D) == KFT_ELIGIBLE && D.ld == 12352 && D.nb == 193 && D.nfm == 4117);
    in.embedded_solver = 0;
    CHECK(kft_limits(in, 2000, D) == KFT_PCG_CHEAPER && kft_limits(in, 100, D) == KFT_ELIGIBLE);
    const KftCost t = kft_cost_model(20, 22, 458);                  // C2: 10 inversions of 23 launches at 32.34 us + 1 ms against 14 ms
    CHECK(std::fabs(t.kft_ms - 8.4382) < 1e-9 && t.pcg_ms == 14.0);
    in.panel_lds = in.lds_cap + 1;
    CHECK(kft_limits(in, 100, D) == KFT_BEYOND_LDS);
    in = X.in; in.K = KFT_K_MAX + 1;
    CHECK(kft_window_reason(in) == KFT_KEYFRAME_COUNT);
    in.K = 0;
    CHECK(kft_window_reason(in) == KFT_KEYFRAME_COUNT);
    in = X.in; in.sp_pos = nullptr;
    CHECK(kft_window_reason(in) == KFT_NO_POSITIONS);
    for (int r = 0; r <= KFT_DAMPER_NOT_CONSECUTIVE; ++r) CHECK(kft_reason_name((KftReason)r)[0] != 0);
}

// the key's fields at their limits
static void check_keys() {
    const int ks[3] = {0, 1, KFT_K_MAX}, ns[3] = {0, 1, KFT_NF_LIMIT - 1};
    for (int k : ks) for (int hi : ns) for (int lo : ns) {
        const uint64_t key = kft_key(k, hi, lo);
        CHECK(key <= 0xFFFFFFFFull && kft_key_k(key) == k && kft_key_hi(key) == hi && kft_key_lo(key) == lo);
        CHECK(kft_key_k((uint32_t)key) == k);
    }
    CHECK(kft_key(1, 0, 0) > kft_key(0, KFT_NF_LIMIT - 1, KFT_NF_LIMIT - 1) && kft_key(0, 1, 0) > kft_key(0, 0, KFT_NF_LIMIT - 1));
    CHECK((kft_src(KFT_SRC_BOUNDARY, 5) >> 30) == 3 && (kft_src(KFT_SRC_SKIN, 0x3FFFFFFF) & 0x3FFFFFFFu) == 0x3FFFFFFFu);
}

// sharded: every rank against the restatement; boundary dampers numbered alike with one holder; the ranks' lists, boundary references
// mapped back to slots, together the one-GPU lists entry for entry
static void check_sharded(const VI& kb) {
    const Win W = big_window();
    const int world = (int)kb.size() - 1;
    Built G; check_rank(W, one_gpu(W), 1, G);
    std::vector<Built> B(world);
    for (int r = 0; r < world; ++r) check_rank(W, Rank{true, world, r, kb}, r == 0 ? 3 : 1, B[r]);
    const size_t n_bd = B[0].ed.bd_slot.size();
    CHECK(n_bd > 0);
    VI slot(n_bd, -1);
    for (int r = 0; r < world; ++r) {
        CHECK(B[r].ed.bd_slot.size() == n_bd);
        for (size_t i = 0; i < n_bd; ++i) if (B[r].ed.bd_slot[i] >= 0) { CHECK(slot[i] < 0); slot[i] = B[r].ed.bd_slot[i]; }
    }
    for (size_t i = 0; i < n_bd; ++i) CHECK(slot[i] >= 0);
    const Rank R0{true, world, 0, kb};
    std::map<Key, std::vector<Ent>> all_pairs;
    std::set<uint32_t> seen_bd;
    for (int r = 0; r < world; ++r) {
        for (const auto& x : B[r].pair_lists) {
            CHECK(R0.owner(std::get<0>(x.first)) == r && !all_pairs.count(x.first));
            for (Ent e : x.second) {
                if ((e.first >> 30) == 3) { seen_bd.insert(e.first & 0x3FFFFFFFu); e.first = (1u << 30) | (uint32_t)slot[e.first & 0x3FFFFFFFu]; }
                all_pairs[x.first].push_back(e);
            }
        }
        for (const auto& x : B[r].couplings) {
            std::vector<uint32_t> s = x.second;
            for (uint32_t& e : s) if (e & KFT_BD) { seen_bd.insert(e & (KFT_BD - 1)); e = (e & 0x80000000u) | (uint32_t)slot[e & (KFT_BD - 1)]; }
            CHECK(G.couplings.count(x.first) && G.couplings[x.first] == s);
        }
    }
    CHECK(all_pairs == G.pair_lists);
    CHECK(!seen_bd.empty() && *seen_bd.rbegin() < n_bd);            // (a boundary damper whose other vertices are fixed or absent is numbered and never read)
    for (const auto& x : G.couplings) {
        const int k = std::get<0>(x.first);
        CHECK(B[R0.owner(k)].couplings.count(x.first) && B[R0.owner(k + 1)].couplings.count(x.first));
    }
}

int main() {
    check_keys();
    check_one_gpu();
    check_reasons();
    check_sharded({0, 2, 5});
    check_sharded({0, 2, 3, 5});
    check_sharded({0, 1, 4, 5});
    std::printf("kft_prep_check OK: key helpers at their limits, K = 1, K = 2 with a pose fixed, five keyframes with fixed and padding rows, "
                "fixed-end springs, absent and fixed damper vertices, short observations and a node named twice, a keyframe without free nodes, "
                "layout and cleared regions, every ineligibility reason, worlds 2 and 3 with boundary dampers against one GPU, thread counts 1 and 3\n");
    return 0;
}
