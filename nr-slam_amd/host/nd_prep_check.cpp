// Stand-alone check of the host stages of the direct solver's set-up (csrc/nrs_nd_prep_host.hpp) for a sanitizer build:
// `make nd_prep_check && ./nd_prep_check`.  Hand-made frames of 6-40 vertices go through the stages in the driver's order
// (nrs_engine_nd.hpp nd_prep_run_body); every array they leave is held to a brute-force restatement over ordered maps and sets of
// node pairs, written here without the stages' sorting and merging.  No HIP, no library.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>
#include "../csrc/nrs_nd_prep_host.hpp"

using namespace nrs;
typedef std::vector<int> VI;
typedef std::pair<int, int> PR;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "nd_prep_check: %s:%d: %s\n", __FILE__, __LINE__, #x); std::abort(); } } while (0)

struct Frame {
    std::vector<uint8_t> rflag;
    bool pose_fixed = false;
    VI sp, dm, sk;                                                   // sp_ij (2 per spring), dm_idx (4 per damper), sk_vert (SK_MAX per observation)
    std::vector<double> om, pos;
    explicit Frame(int M) : rflag(M, RF_OBS | RF_REPROJ_ACTIVE), pos(3 * (size_t)M) {
        for (int v = 0; v < M; ++v) { pos[3 * v] = v % 5; pos[3 * v + 1] = v / 5; pos[3 * v + 2] = 0.25 * (v % 3); }
    }
    void spring(int i, int j) { sp.push_back(i); sp.push_back(j); }
    void damper(int i, int j, int c1 = -1, int c2 = -1) { dm.push_back(c1); dm.push_back(c2); dm.push_back(i); dm.push_back(j); }
    void edge(int i, int j) { spring(i, j); damper(i, j); }          // a2's form: a spring and a damper, index for index
    void obs(std::initializer_list<PR> nodes) {                      // (vertex, weight in 16ths)
        size_t k = 0;
        for (const PR& n : nodes) { sk.push_back(n.first); om.push_back(n.second / 16.0); ++k; }
        for (; k < (size_t)SK_MAX; ++k) { sk.push_back(-1); om.push_back(0.0); }
    }
    NdIn in() const {
        NdIn I;
        I.M = (int)rflag.size(); I.rflag = rflag.data(); I.pose_fixed = pose_fixed;
        I.n_sp = (int)sp.size() / 2; I.sp_ij = sp.data(); I.n_dm = (int)dm.size() / 4; I.dm_idx = dm.data();
        I.n_skin = (int)sk.size() / SK_MAX; I.sk_vert = sk.data(); I.sk_om = om.data(); I.vpos = pos.data();
        return I;
    }
};

struct Built { NdPrepData P; NdPlan plan; bool twin = false, plan_ok = false; std::string err; };
static const int LEAF = 4;
// the stages in the driver's order
static void build(const Frame& F, Built& B) {
    const NdIn in = F.in();
    NdPrepData& P = B.P;
    nd_number_nodes(in, P);
    nd_make_key(in, LEAF, ND_SMAXN, P);
    P.st = std::make_shared<NdStruct>();
    std::vector<NdEdgeKey> keys;
    B.twin = nd_edge_keys(in, P.node_of, keys);
    nd_skin_pairs(in, P);
    nd_sort_by_pair(keys, P.n_free);
    const size_t n_coupl = nd_merge_pairs(keys, B.twin, P);
    nd_cut_pairs(P, n_coupl, nd_pose_pairs(in, P, n_coupl));
    const std::vector<double> pos = nd_node_positions(in, P);
    B.plan_ok = nd_build_plan(P.n_nodes, pos.data(), P.last.data(), (int)P.st->pkind.size(), P.st->pairs.data(), B.plan, &B.err, LEAF, ND_SMAXN, false, 0, true);
    if (B.plan_ok && in.n_skin > 0) { nd_prep_ske(P, B.plan); nd_prep_ske_values(P, in.sk_om); }
}

// ---- the brute-force restatement
struct Expect {
    VI node_of, node_vtx;
    std::map<PR, VI> springs, dampers;                               // node pair (low, high) -> its edges, as they arrive
    std::map<PR, std::vector<PR>> obs;                               // node pair -> (place of the low slot, place of the high slot) per observation, in order
    std::set<PR> pairs;
    std::vector<VI> nl;                                              // node -> places of the observations that reach it
};
static Expect expect(const Frame& F) {
    Expect E;
    const int M = (int)F.rflag.size();
    E.node_of.assign(M, -1);
    for (int v = 0; v < M; ++v)
        if (!(F.rflag[v] & RF_FIXED)) { E.node_of[v] = (int)E.node_vtx.size(); E.node_vtx.push_back(v); }
    auto pair_of = [&](int va, int vb, PR& p) {
        const int a = E.node_of[va], b = E.node_of[vb];
        if (a < 0 || b < 0 || a == b) return false;
        p = PR(std::min(a, b), std::max(a, b));
        return true;
    };
    PR p;
    for (size_t q = 0; q < F.sp.size() / 2; ++q) if (pair_of(F.sp[2 * q], F.sp[2 * q + 1], p)) { E.springs[p].push_back((int)q); E.pairs.insert(p); }
    for (size_t q = 0; q < F.dm.size() / 4; ++q) if (pair_of(F.dm[4 * q + 2], F.dm[4 * q + 3], p)) { E.dampers[p].push_back((int)q); E.pairs.insert(p); }
    E.nl.resize(E.node_vtx.size());
    for (size_t i = 0; i < F.sk.size() / SK_MAX; ++i)
        for (int a = 0; a < SK_MAX; ++a) {
            const int va = F.sk[SK_MAX * i + a];
            if (va < 0 || E.node_of[va] < 0) continue;
            E.nl[E.node_of[va]].push_back((int)(SK_MAX * i + a));
            for (int b = a + 1; b < SK_MAX; ++b) {
                const int vb = F.sk[SK_MAX * i + b];
                if (vb >= 0 && pair_of(va, vb, p)) { E.obs[p].push_back(PR((int)(SK_MAX * i + a), (int)(SK_MAX * i + b))); E.pairs.insert(p); }
            }
        }
    return E;
}

// every array of the structure against the restatement; returns what was built for the case's own checks
static Built check_frame(const Frame& F, bool want_twin) {
    Built B;
    build(F, B);
    const Expect E = expect(F);
    const NdPrepData& P = B.P;
    const NdStruct& T = *P.st;
    const int n_free = (int)E.node_vtx.size(), n_coupl = (int)E.pairs.size();
    CHECK(P.node_of == E.node_of && P.node_vtx == E.node_vtx && P.n_free == n_free);
    CHECK(P.pose_free == !F.pose_fixed && P.n_nodes == n_free + (F.pose_fixed ? 0 : 2));
    CHECK(B.twin == want_twin);
    // the pose's pairs: two halves per observed row, in row order, then the one pose-pose pair
    VI pose_pairs;
    if (!F.pose_fixed) {
        for (int a = 0; a < n_free; ++a)
            if (F.rflag[E.node_vtx[a]] & RF_OBS) for (int h = 0; h < 2; ++h) { pose_pairs.push_back(n_free + h); pose_pairs.push_back(a); }
        pose_pairs.push_back(n_free + 1); pose_pairs.push_back(n_free);
    }
    const int np = n_coupl + (int)pose_pairs.size() / 2;
    CHECK((int)T.pairs.size() == 2 * np && (int)T.pkind.size() == np);
    CHECK((int)T.eptr.size() == n_coupl + 1 && (int)P.pair_sk0.size() == n_coupl && (int)P.pair_sk1.size() == n_coupl);
    CHECK(T.eptr[0] == 0 && (int)T.eid.size() == T.eptr[n_coupl]);
    int i = 0, sk_at = 0;
    for (const PR& p : E.pairs) {                                     // (a std::set: sorted and unique)
        CHECK(T.pairs[2 * i] == p.first && T.pairs[2 * i + 1] == p.second && T.pkind[i] == 0);
        VI ids;                                                      // springs before dampers, each as they arrive
        if (E.springs.count(p)) for (int q : E.springs.at(p)) ids.push_back(q << 1);
        if (E.dampers.count(p)) for (int q : E.dampers.at(p)) ids.push_back((q << 1) | 1);
        CHECK(VI(T.eid.begin() + T.eptr[i], T.eid.begin() + T.eptr[i + 1]) == ids);
        const std::vector<PR> none, &ob = E.obs.count(p) ? E.obs.at(p) : none;
        CHECK(P.pair_sk0[i] == sk_at && P.pair_sk1[i] == sk_at + (int)ob.size());
        for (const PR& o : ob) { CHECK(P.skt[sk_at].ia == o.first && P.skt[sk_at].ib == o.second); ++sk_at; }
        ++i;
    }
    CHECK(sk_at == (int)P.skt.size());
    CHECK(VI(T.pairs.begin() + 2 * n_coupl, T.pairs.end()) == pose_pairs);
    for (int k = n_coupl; k < np; ++k) CHECK(T.pkind[k] == (k == np - 1 ? 2 : 1));
    CHECK((int)P.last.size() == P.n_nodes);
    for (int u = 0; u < P.n_nodes; ++u) CHECK(P.last[u] == (u >= n_free ? 1 : 0));
    CHECK((int)P.nl_ptr.size() == n_free + 1 && P.nl_ptr[0] == 0 && (int)P.nl_ix.size() == P.nl_ptr[n_free]);
    for (int u = 0; u < n_free; ++u) CHECK(VI(P.nl_ix.begin() + P.nl_ptr[u], P.nl_ix.begin() + P.nl_ptr[u + 1]) == E.nl[u]);
    CHECK(B.plan_ok == (P.n_nodes > 0));
    return B;
}

// ---- the cases
static Frame mixed_frame(bool pose_fixed, bool swap_dampers) {      // 12 vertices on a 4 x 3 grid, three of them fixed, one unobserved
    Frame F(12);
    F.pose_fixed = pose_fixed;
    F.rflag[1] |= RF_FIXED; F.rflag[6] |= RF_FIXED; F.rflag[7] |= RF_FIXED;
    F.rflag[4] &= (uint8_t)~RF_OBS;
    const int e[][2] = {{0, 4}, {4, 5}, {5, 4}, {0, 4}, {2, 3}, {8, 9}, {9, 10}, {10, 11}, {3, 11}, {5, 9}, {4, 8}, {2, 5}, {0, 5},
                        {6, 7}, {1, 0}, {5, 6}, {3, 3}, {10, 9}};    // with duplicates, both orientations, both ends fixed, one end fixed, a self edge
    const int n = (int)(sizeof(e) / sizeof(e[0]));
    for (int q = 0; q < n; ++q) F.spring(e[q][0], e[q][1]);
    for (int q = 0; q < n; ++q) { const int k = swap_dampers && q < 2 ? 1 - q : q; F.damper(e[k][0], e[k][1]); }
    return F;
}
static void check_mixed_and_twin() {
    for (int pose_fixed = 0; pose_fixed < 2; ++pose_fixed) {
        const Built tw = check_frame(mixed_frame(pose_fixed, false), true), nt = check_frame(mixed_frame(pose_fixed, true), false);
        CHECK(tw.P.st->pairs == nt.P.st->pairs && tw.P.st->eptr == nt.P.st->eptr);
        for (const Built* B : {&tw, &nt})
            for (size_t i = 0; i + 1 < B->P.st->eptr.size(); ++i)
                for (int t = B->P.st->eptr[i]; t + 1 < B->P.st->eptr[i + 1]; ++t) CHECK((B->P.st->eid[t] & 1) <= (B->P.st->eid[t + 1] & 1));
        // (vanishing edges: 6-7 both fixed, 1-0 and 5-6 one end fixed, 3-3 a self edge -- in no pair; 0-4 given twice -- one pair, two springs)
        const Expect E = expect(mixed_frame(pose_fixed, false));
        CHECK(E.pairs.size() == 11 && E.springs.at(PR(E.node_of[0], E.node_of[4])).size() == 2);
    }
    Frame F = mixed_frame(false, false);                             // a four-vertex damper: a BA window
    CHECK(!nd_has_window_dampers(F.in()));
    F.dm[4 * 3] = 2;
    CHECK(nd_has_window_dampers(F.in()));
    F.dm[4 * 3] = -1; F.dm[4 * 3 + 1] = 2;
    CHECK(nd_has_window_dampers(F.in()));
}

// embedded mode: every plan entry's coefficients, scattered into a dense weight matrix, against sum_obs w_a w_b
static void check_embedded() {
    Frame F(14);
    F.rflag[3] |= RF_FIXED; F.rflag[9] |= RF_FIXED;
    F.edge(0, 1); F.edge(1, 2); F.edge(4, 5); F.edge(5, 6); F.edge(10, 11); F.edge(12, 13); F.edge(2, 4);
    F.obs({{0, 4}, {1, 2}, {2, 8}, {3, 2}});                         // 0-1, 1-2: by edges too; 0-2: by observations only; 3: fixed
    F.obs({{5, 1}, {7, 6}, {5, 3}, {8, 6}});                         // node 5 twice; 5-7, 7-8, 5-8: observations only
    F.obs({{9, 16}});                                                // a fixed node alone
    F.obs({{0, 2}, {2, 2}, {7, 4}, {10, 8}, {1, 1}, {4, 1}, {6, 1}, {8, 1}, {11, 1}, {12, 1}, {13, 1}});   // a full row
    const Built B = check_frame(F, true);
    const Expect E = expect(F);
    const NdPrepData& P = B.P;
    const NdStruct& T = *P.st;
    const PR only_obs(E.node_of[0], E.node_of[2]), both(E.node_of[0], E.node_of[1]);
    CHECK(!E.springs.count(only_obs) && E.obs.count(only_obs) && E.springs.count(both) && E.obs.count(both));
    const int n = P.n_nodes, n_free = P.n_free;
    std::vector<double> W((size_t)n * n, 0.0), g(n, 0.0), We((size_t)n * n, 0.0), ge(n, 0.0);
    CHECK(T.ske_ptr.size() == B.plan.ent.size() + 1 && T.ske_pt.size() == P.ske_cf.size());
    for (size_t q = 0; q < B.plan.ent.size(); ++q) {
        const uint32_t kind = B.plan.ent[q].src >> ND_KIND_SHIFT, idx = B.plan.ent[q].src & ND_SRC_MASK;
        double s = 0;
        for (int t = T.ske_ptr[q]; t < T.ske_ptr[q + 1]; ++t) { CHECK(T.ske_pt[t] == T.ske_ia[t] / SK_MAX); s += P.ske_cf[t]; }
        if (kind == 0) W[(size_t)idx * n + idx] += s;
        else if (kind == 2) g[idx] += s;
        else { const int a = T.pairs[2 * idx], b = T.pairs[2 * idx + 1]; W[(size_t)a * n + b] += s; W[(size_t)b * n + a] += s; }
    }
    // brute force: an observation is sum_a w_a x_(node a) -- rows couple by w_a w_b, the pose halves and the gradient take sum_a w_a.
    // A node named twice by one observation (node 5 above) gets w_a^2 + w_b^2 on its diagonal, not (w_a + w_b)^2: the lists square
    // every place on its own and nd_skin_pairs leaves pairs of one node out.  Stated here as the stages behave today.
    for (size_t i = 0; i < F.sk.size() / SK_MAX; ++i)
        for (int a = 0; a < SK_MAX; ++a) {
            const int va = F.sk[SK_MAX * i + a], na = va >= 0 ? E.node_of[va] : -1;
            if (na < 0) continue;
            const double wa = F.om[SK_MAX * i + a];
            ge[na] += wa;
            if (!F.pose_fixed && (F.rflag[va] & RF_OBS)) for (int h = 0; h < 2; ++h) { We[(size_t)(n_free + h) * n + na] += wa; We[(size_t)na * n + n_free + h] += wa; }
            for (int b = 0; b < SK_MAX; ++b) {
                const int vb = F.sk[SK_MAX * i + b], nb = vb >= 0 ? E.node_of[vb] : -1;
                if (nb < 0 || (nb == na && b != a)) continue;
                We[(size_t)na * n + nb] += wa * F.om[SK_MAX * i + b];
            }
        }
    CHECK(W == We && g == ge);                                       // (exact: the weights are small dyadic fractions)
}

static void check_key() {
    const Frame F0 = mixed_frame(false, false);
    Frame E0(14);
    E0.edge(0, 1); E0.obs({{0, 4}, {1, 2}, {2, 8}});
    auto key_of = [](const Frame& F, int leaf, NdPrepData& P) { nd_number_nodes(F.in(), P); nd_make_key(F.in(), leaf, ND_SMAXN, P); };
    auto same = [&](const Frame& A, const Frame& B, int leaf_b = LEAF) {
        NdPrepData a, b;
        key_of(A, LEAF, a); key_of(B, leaf_b, b);
        CHECK((a.key == b.key) == (a.hash == b.hash));                // (no collision among these)
        return a.key == b.key;
    };
    Frame F = F0, E = E0;
    F.pos[5] += 1.0; E.om[1] = 0.5;
    CHECK(same(F0, F) && same(E0, E));                               // positions and skinning weights are not in the key
    F = F0; F.rflag[2] ^= RF_REPROJ_ACTIVE; CHECK(same(F0, F));
    F = F0; F.rflag[2] ^= 0x40; CHECK(same(F0, F));
    F = F0; F.rflag[2] ^= RF_FIXED; CHECK(!same(F0, F));
    F = F0; F.rflag[2] ^= RF_OBS; CHECK(!same(F0, F));
    F = F0; F.sp[5] = 6; CHECK(!same(F0, F));
    F = F0; F.dm[4 * 2 + 3] = 6; CHECK(!same(F0, F));
    F = F0; F.pose_fixed = true; CHECK(!same(F0, F));
    CHECK(!same(F0, F0, LEAF + 1));
    E = E0; E.sk[2] = 3; CHECK(!same(E0, E));
}

static void check_value_descriptors() {
    const Frame F = mixed_frame(false, true);
    const Built B = check_frame(F, false);
    const NdPrepData& P = B.P;
    const NdStruct& T = *P.st;
    const int M = (int)F.rflag.size(), n_free = P.n_free;
    VI vrow(M), sp_pos(F.sp.size()), dm_pos(F.dm.size(), -7);
    for (int v = 0; v < M; ++v) vrow[v] = (5 * v + 3) % M + 20;      // (5 and 12 are coprime: a permutation, behind 20 rows of something else)
    for (size_t q = 0; q < F.sp.size() / 2; ++q) { sp_pos[2 * q] = 100 + 3 * (int)q; sp_pos[2 * q + 1] = -9; }
    for (size_t q = 0; q < F.dm.size() / 4; ++q) dm_pos[4 * q + 2] = 500 + 5 * (int)q;
    NdValDesc V;
    CHECK(nd_value_descriptors(T, P, vrow.data(), sp_pos.data(), dm_pos.data(), V));
    CHECK((int)V.nrow.size() == P.n_nodes && (int)V.node_out.size() == P.n_nodes && V.pd.size() == T.pkind.size() && V.src.size() == T.eid.size());
    for (int a = 0; a < n_free; ++a) CHECK(V.nrow[a] == vrow[P.node_vtx[a]] && V.node_out[a] == 3 * V.nrow[a]);
    CHECK(V.nrow[n_free] == -1 && V.nrow[n_free + 1] == -2 && V.node_out[n_free] == -1 && V.node_out[n_free + 1] == -4);
    for (size_t t = 0; t < T.eid.size(); ++t) {
        const int id = T.eid[t] >> 1, kind = T.eid[t] & 1;
        CHECK(V.src[t] == (((kind ? 500 + 5 * id : 100 + 3 * id) << 1) | kind));
    }
    for (size_t i = 0; i < T.pkind.size(); ++i) {
        const NdPairD& d = V.pd[i];
        const int a = T.pairs[2 * i], b = T.pairs[2 * i + 1];
        if (T.pkind[i] == 0) CHECK(d.kind == 0 && d.a == V.nrow[a] && d.b == V.nrow[b] && d.src0 == T.eptr[i] && d.nsrc == T.eptr[i + 1] - T.eptr[i]);
        else if (T.pkind[i] == 1) CHECK(d.kind == 1 && d.a == a - n_free && d.b == V.nrow[b] && d.src0 == 0 && d.nsrc == 0);
        else CHECK(d.kind == 2 && d.a == 0 && d.b == 0 && d.src0 == 0 && d.nsrc == 0);
    }
    sp_pos[2 * 4] = -1;                                              // spring 4 (2-3) has no slot here: another rank's incidence
    CHECK(!nd_value_descriptors(T, P, vrow.data(), sp_pos.data(), dm_pos.data(), V));
    sp_pos[2 * 4] = 112; dm_pos[4 * 5 + 2] = -1;
    CHECK(!nd_value_descriptors(T, P, vrow.data(), sp_pos.data(), dm_pos.data(), V));
}

static void check_empty() {
    for (int pose_fixed = 0; pose_fixed < 2; ++pose_fixed) {
        Frame A(6);                                                  // nothing free
        A.pose_fixed = pose_fixed;
        for (uint8_t& f : A.rflag) f |= RF_FIXED;
        A.edge(0, 1); A.edge(2, 3); A.obs({{0, 8}, {4, 8}});
        const Built a = check_frame(A, true);
        CHECK(a.P.n_free == 0 && a.P.st->eid.empty() && a.P.st->eptr == VI(1, 0) && a.P.skt.empty() && a.P.nl_ix.empty() && a.P.nl_ptr == VI(1, 0));
        CHECK((int)a.P.st->pkind.size() == (pose_fixed ? 0 : 1));
        Frame N(8);                                                  // free vertices, no edge at all
        N.pose_fixed = pose_fixed;
        N.rflag[5] |= RF_FIXED;
        const Built b = check_frame(N, true);
        CHECK(b.P.st->eid.empty() && b.P.st->eptr == VI(1, 0) && b.P.pair_sk0.empty() && (int)b.P.st->pkind.size() == (pose_fixed ? 0 : 2 * 7 + 1));
        NdValDesc V;
        const VI vrow = {0, 1, 2, 3, 4, 5, 6, 7};
        CHECK(nd_value_descriptors(*b.P.st, b.P, vrow.data(), nullptr, nullptr, V) && V.src.empty() && V.pd.size() == b.P.st->pkind.size());
    }
}

static void check_large() {                                         // 40 vertices, more than one leaf and several fronts: kNN-like edges over a 8 x 5 grid
    Frame F(40);
    for (int v = 0; v < 40; ++v) { F.pos[3 * v] = v % 8; F.pos[3 * v + 1] = v / 8; if (v % 9 == 4) F.rflag[v] |= RF_FIXED; if (v % 7 == 3) F.rflag[v] &= (uint8_t)~RF_OBS; }
    for (int v = 0; v < 40; ++v) {
        if (v % 8 != 7) F.edge(v, v + 1);
        if (v + 8 < 40) F.edge(v + 8, v);
        if (v % 8 != 7 && v + 9 < 40) F.edge(v, v + 9);
    }
    for (int i = 0; i < 6; ++i) F.obs({{6 * i, 8}, {6 * i + 1, 4}, {6 * i + 9, 2}, {(6 * i + 17) % 40, 1}, {(6 * i + 4) % 40, 1}});
    check_frame(F, true);
    F.pose_fixed = true;
    check_frame(F, true);
}

int main() {
    check_mixed_and_twin();
    check_embedded();
    check_key();
    check_value_descriptors();
    check_empty();
    check_large();
    std::printf("nd_prep_check OK: mixed fixed/free with pose free and fixed, twin vs non-twin, vanishing edges, four-vertex damper, embedded lists and "
                "weights, key, value descriptors, nothing free and no edges, plan built on every frame\n");
    return 0;
}
