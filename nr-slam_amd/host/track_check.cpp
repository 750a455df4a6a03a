// Stand-alone check of the host half of a2 (csrc/nrs_track_host.hpp) for a sanitizer build: `make track_check && ./track_check`.
// Hand-made lists go through the frame index, the two walks, the statistics and the stage-2 compaction; every expected value below is
// worked out by hand.  The frames are as small as a case allows (the walk's 12th candidate needs 13 points).
#include <cassert>
#include <cfloat>
#include <cstdio>
#include "../csrc/nrs_track_host.hpp"

using namespace nrs_track;
typedef std::vector<int> VI;
typedef std::vector<float> VF;

struct Entry { int col; float w, d0; int st; };
struct Lists {                                                    // GetEdges lists of n map points, rows added in ascending order
    VI beg, end, col, st;
    VF w, d0;
    std::vector<char> trunc;
    explicit Lists(int n) : beg(n, 0), end(n, 0), trunc(n, 0) {}
    void row(int p, std::initializer_list<Entry> es, bool truncated = false) {
        beg[p] = (int)col.size();
        for (const Entry& e : es) { col.push_back(e.col); w.push_back(e.w); d0.push_back(e.d0); st.push_back(e.st); }
        end[p] = (int)col.size();
        trunc[p] = truncated;
    }
    ListView view() const { return {beg.data(), end.data(), col.data(), w.data(), d0.data(), st.data(), trunc.data()}; }
    const Entry find(int p, int o) const { for (int a = beg[p]; a < end[p]; ++a) if (col[a] == o) return {o, w[a], d0[a], st[a]}; assert(false); return {}; }
};
static const int G = NRS_GRAPH_NEIGHBOR, B = NRS_GRAPH_BAD, T3 = NRS_TRACKED_WITH_3D;

// what the device walk would hand back for these lists: the accepted connections of the host walk, with the lists' weights
static WalkOut walk_out_of(const FrameIndex& x, const EdgeSet& e, const Lists& L) {
    WalkOut wo;
    wo.n_acc.assign(x.N, 0); wo.acc.assign(11 * (size_t)x.N, -1); wo.w.assign(11 * (size_t)x.N, 0.f); wo.d0.assign(11 * (size_t)x.N, 0.f);
    wo.ended.assign(x.N, 1); wo.lost.assign(e.lost_flag.begin(), e.lost_flag.end());
    for (int idx = 0; idx < x.N; ++idx) {
        VI io;
        if (x.node_of[idx] >= 0) io.assign(e.acc.begin() + 11 * idx, e.acc.begin() + 11 * idx + e.n_acc[idx]);
        else if (e.sk_of[idx] >= 0)
            for (int k = 0; k < 11 && e.sk_node[11 * e.sk_of[idx] + k] >= 0; ++k) io.push_back(x.node_idx[e.sk_node[11 * e.sk_of[idx] + k]]);
        wo.n_acc[idx] = (int)io.size();
        for (size_t k = 0; k < io.size(); ++k) {
            const Entry en = L.find(x.ids[idx], x.ids[io[k]]);
            wo.acc[11 * idx + k] = io[k]; wo.w[11 * idx + k] = en.w; wo.d0[11 * idx + k] = en.d0;
        }
    }
    return wo;
}
static void same_edges(const FrameIndex& x, const Lists& L) {      // the read-out of the device walk makes the host walk's edge set
    EdgeSet h, d;
    h.init(x); d.init(x);
    assert(host_walk(x, L.view(), h).what == DONE);
    assert(edges_from_walk(x, walk_out_of(x, h, L), L.trunc.data(), d).what == DONE);
    assert(h.dm_idx == d.dm_idx && h.sp_ij == d.sp_ij && h.dm_w == d.dm_w && h.sp_d0 == d.sp_d0 && h.ne == d.ne);
    assert(h.sk_node == d.sk_node && h.sk_om == d.sk_om && h.sk_of == d.sk_of && h.sk_idx == d.sk_idx && h.lost_flag == d.lost_flag);
}

static void check_frame_index() {
    FrameIndex e, r, n;
    const int32_t none[1] = {0}, far[2] = {0, 3}, st[2] = {T3, T3};
    const uint8_t no_node[2] = {0, 0};
    assert(frame_index(e, 3, 0, none, none, nullptr).what == EMPTY);
    assert(frame_index(r, 3, 2, far, st, nullptr).what == F_MAP_RANGE);                   // 3 map points: index 3 is out of range
    assert(frame_index(n, 4, 2, far, st, no_node).what == NO_NODE);
}

// every point a node; the io < idx rule, codes -1 / -2
static void check_parity_walk() {
    // map points 0..6; the frame sees 0..5: 0..3 optimised, 4 just triangulated (-1), 5 tracked without 3D (lost, -2); 6 is not in the frame (-1)
    const int32_t f_map[6] = {0, 1, 2, 3, 4, 5}, f_st[6] = {T3, T3, T3, T3, NRS_JUST_TRIANGULATED, NRS_TRACKED};
    FrameIndex x;
    assert(frame_index(x, 7, 6, f_map, f_st, nullptr).what == DONE);
    assert(x.N == 4 && x.M == 4 && (x.walk_code == VI{0, 1, 2, 3, -1, -2, -1}) && x.no_vertex.empty() && x.is_node.empty());
    assert((x.ids == VI{0, 1, 2, 3}) && (x.node_of == VI{0, 1, 2, 3}) && (x.id_to_idx == VI{0, 1, 2, 3, -1, -1, -1}));
    Lists L(7);
    L.row(0, {{4, .9f, 9.f, G}, {1, .5f, 1.f, G}, {5, .4f, 8.f, G}, {6, .3f, 7.f, G}, {2, .25f, 2.f, G}});
    L.row(1, {{0, .5f, 1.f, G}, {2, .125f, 3.f, G}});             // 0 accepted 1 already: no second edge
    L.row(2, {{0, .25f, 2.f, G}, {1, .125f, 3.f, G}});            // both accepted 2 already
    L.row(3, {{0, .0625f, 4.f, G}});                              // 0's list does not hold 3: the edge is made from 3's side
    EdgeSet e;
    e.init(x);
    assert(host_walk(x, L.view(), e).what == DONE);
    assert(e.ne == 4 && (e.sp_ij == VI{0, 1, 0, 2, 1, 2, 3, 0}) && (e.dm_idx == VI{-1, -1, 0, 1, -1, -1, 0, 2, -1, -1, 1, 2, -1, -1, 3, 0}));
    assert((e.dm_w == VF{.5f, .25f, .125f, .0625f}) && (e.sp_d0 == VF{1.f, 2.f, 3.f, 4.f}));
    assert((e.n_acc == std::vector<uint8_t>{2, 1, 0, 1}) && e.acc[0] == 1 && e.acc[1] == 2 && e.acc[11] == 2 && e.acc[33] == 0);
    assert((e.lost_flag == std::vector<uint8_t>{0, 0, 0, 0, 0, 1, 0}) && (e.lost_ids() == VI{5}));   // -2 sets the flag, -1 does nothing
    assert(e.sk_idx.empty() && e.sk_node.empty() && e.sk_om.empty() && (e.sk_of == VI{-1, -1, -1, -1}));
    same_edges(x, L);
}

// the walk ends at the 12th candidate and at the first BAD status; a truncated list counts only if the walk did not end
static void check_walk_ends() {
    int32_t f_map[13], f_st[13];
    for (int i = 0; i < 13; ++i) { f_map[i] = i; f_st[i] = T3; }
    FrameIndex x;
    assert(frame_index(x, 13, 13, f_map, f_st, nullptr).what == DONE);
    Lists L(13);
    L.row(0, {{1, 1.f, 1.f, G}, {2, 1.f, 1.f, G}, {3, 1.f, 1.f, G}, {4, 1.f, 1.f, G}, {5, 1.f, 1.f, G}, {6, 1.f, 1.f, G}, {7, 1.f, 1.f, G}, {8, 1.f, 1.f, G},
              {9, 1.f, 1.f, G}, {10, 1.f, 1.f, G}, {11, 1.f, 1.f, G}, {12, 1.f, 1.f, G}}, true);   // 11 accepted, ended at the 12th: not "ran off"
    L.row(1, {{2, .5f, 2.f, G}, {3, .5f, 2.f, B}, {4, .5f, 2.f, G}}, true);                         // ended at the BAD one
    EdgeSet e;
    e.init(x);
    assert(host_walk(x, L.view(), e).what == DONE);
    assert(e.ne == 12 && e.n_acc[0] == 11 && e.n_acc[1] == 1 && e.sp_ij[20] == 0 && e.sp_ij[21] == 11 && e.sp_ij[22] == 1 && e.sp_ij[23] == 2);
    same_edges(x, L);
    // map ids that are not frame indices: the walk of map point 4 takes both entries of a truncated list and is reported by its map id
    const int32_t g_map[3] = {4, 2, 5}, g_st[3] = {T3, T3, T3};
    FrameIndex y;
    assert(frame_index(y, 6, 3, g_map, g_st, nullptr).what == DONE && (y.ids == VI{4, 2, 5}) && (y.id_to_idx == VI{-1, -1, 1, -1, 0, 2}));
    Lists K(6);
    K.row(2, {});
    K.row(4, {{2, .5f, 1.f, G}, {5, .5f, 1.f, G}}, true);
    K.row(5, {});
    EdgeSet f;
    f.init(y);
    const Status s = host_walk(y, K.view(), f);
    assert(s.what == RAN_OFF && s.point == 4);
    WalkOut wo;                                                   // ... and so is the device walk's
    wo.n_acc = {2, 0, 0}; wo.acc.assign(33, -1); wo.acc[0] = 1; wo.acc[1] = 2; wo.w.assign(33, .5f); wo.d0.assign(33, 1.f);
    wo.ended = {0, 1, 1}; wo.lost.assign(6, 0);
    const Status t = edges_from_walk(y, wo, K.trunc.data(), f);
    assert(t.what == RAN_OFF && t.point == 4);
    wo.ended[0] = 1;
    assert(edges_from_walk(y, wo, K.trunc.data(), f).what == DONE && (f.sp_ij == VI{0, 1, 0, 2}));
    assert(edges_from_walk(y, wo, nullptr, f).what == DONE);       // (a source without truncation)
}

// embedded mode: nodes 0 and 2, skinned points 1 and 3
static void check_skinning() {
    const int32_t f_map[4] = {0, 1, 2, 3}, f_st[4] = {T3, T3, T3, T3};
    const uint8_t f_node[4] = {1, 0, 1, 0};
    FrameIndex x;
    assert(frame_index(x, 4, 4, f_map, f_st, f_node).what == DONE);
    assert(x.N == 4 && x.M == 2 && (x.node_of == VI{0, -1, 1, -1}) && (x.node_idx == VI{0, 2}) && (x.walk_code == VI{0, -1, 2, -1}));
    assert((x.no_vertex == std::vector<uint8_t>{0, 1, 0, 1}) && (x.is_node == std::vector<uint8_t>{1, 0, 1, 0}));
    Lists L(4);
    L.row(0, {{1, .75f, 5.f, G}, {2, .5f, 1.f, G}});              // the skinned point 1 is passed over
    L.row(1, {{0, .5f, 6.f, G}, {3, .4f, 6.f, G}, {2, .25f, 7.f, G}});
    L.row(2, {{0, .5f, 1.f, G}});
    L.row(3, {{1, .4f, 6.f, G}});                                 // meets no node: no slot
    EdgeSet e;
    e.init(x);
    assert(host_walk(x, L.view(), e).what == DONE);
    assert(e.ne == 1 && (e.sp_ij == VI{0, 1}) && (e.dm_idx == VI{-1, -1, 0, 1}) && (e.dm_w == VF{.5f}) && (e.sp_d0 == VF{1.f}));
    assert((e.sk_idx == VI{1}) && (e.sk_of == VI{-1, 0, -1, -1}) && e.sk_node.size() == 22 && e.sk_om.size() == 22);
    assert(e.sk_node[0] == 0 && e.sk_node[1] == 1 && e.sk_om[0] == 0.5 / 0.75 && e.sk_om[1] == 0.25 / 0.75);
    assert(std::fabs(e.sk_om[0] + e.sk_om[1] - 1.0) <= DBL_EPSILON);
    for (int k = 2; k < 22; ++k) assert(e.sk_node[k] == -1 && e.sk_om[k] == 0.0);   // the rest of slot 0, and the slot point 3 did not take
    same_edges(x, L);
}

// a frame that is a permuted, partial view of the map: slot, map id, index among the optimised points and vertex are four different numbers.
// Map points 0..8; slots: 6, none, 2, 7 (tracked without 3D: lost), 0, 4 (just triangulated), 3; map points 1, 5, 8 are not in the frame
static void check_permuted_frame() {
    const int32_t f_map[7] = {6, -1, 2, 7, 0, 4, 3}, f_st[7] = {T3, NRS_TRACKED, T3, NRS_TRACKED, T3, NRS_JUST_TRIANGULATED, T3};
    Lists L(9);
    L.row(0, {{6, .75f, 2.f, G}, {2, .25f, 5.f, G}, {3, .125f, 6.f, B}, {7, .0625f, 9.f, B}});
    L.row(2, {{6, .875f, 1.f, G}, {3, .5f, 4.f, G}, {4, .375f, 9.f, G}, {0, .25f, 5.f, G}});
    L.row(3, {{6, .625f, 3.f, G}, {2, .5f, 4.f, G}, {8, .3125f, 9.f, G}, {0, .125f, 6.f, B}});
    L.row(6, {{2, .875f, 1.f, G}, {7, .8125f, 9.f, G}, {1, .78125f, 9.f, G}, {0, .75f, 2.f, G}, {3, .625f, 3.f, G}});
    L.row(7, {{1, .9f, 9.f, G}, {3, .8f, 9.f, G}, {6, .7f, 9.f, G}, {4, .6f, 9.f, G}, {2, .5f, 9.f, G}});
    {   // every optimised point a node: the optimised points are map points 6, 2, 0, 3 in that order
        FrameIndex x;
        assert(frame_index(x, 9, 7, f_map, f_st, nullptr).what == DONE && x.N == 4 && x.M == 4);
        assert((x.opt_f == VI{0, 2, 4, 6}) && (x.ids == VI{6, 2, 0, 3}) && (x.map_to_frame == VI{4, -1, 2, 6, 5, -1, 0, 3, -1}));
        assert((x.id_to_idx == VI{2, -1, 1, 3, -1, -1, 0, -1, -1}) && (x.walk_code == VI{2, -1, 1, 3, -1, -1, 0, -2, -1}));
        EdgeSet e;
        e.init(x);
        assert(host_walk(x, L.view(), e).what == DONE);
        // 6 takes 2, 0 and 3 (7 is lost, 1 is nothing); 2 is paired with 6 already and takes 3 and 0; 0 and 3 are paired with both and end at their BAD entry
        assert(e.ne == 5 && (e.sp_ij == VI{0, 1, 0, 2, 0, 3, 1, 3, 1, 2}) && (e.dm_w == VF{.875f, .75f, .625f, .5f, .25f}) && (e.sp_d0 == VF{1.f, 2.f, 3.f, 4.f, 5.f}));
        assert((e.n_acc == std::vector<uint8_t>{3, 2, 0, 0}) && (e.lost_ids() == VI{7}));
        same_edges(x, L);
        Stage2 s;
        s.lost_ids = e.lost_ids();
        stage2_vertices(x, s);
        assert(s.NV == 4 && lost_walk(x, L.view(), s).what == DONE && (s.un_ij == VI{4, 3, 4, 0, 4, 1}) && (s.un_w == VF{.8f, .7f, .5f}));
    }
    {   // embedded: f_node is laid out per SLOT -- slots 0, 4, 6 (map points 6, 0, 3) are nodes, map point 2 is skinned; read per map id it would make 3 a non-node
        const uint8_t f_node[7] = {1, 0, 0, 0, 1, 0, 1};
        FrameIndex x;
        assert(frame_index(x, 9, 7, f_map, f_st, f_node).what == DONE && x.N == 4 && x.M == 3);
        assert((x.node_of == VI{0, -1, 1, 2}) && (x.node_idx == VI{0, 2, 3}) && (x.walk_code == VI{2, -1, -1, 3, -1, -1, 0, -2, -1}));
        assert((x.no_vertex == std::vector<uint8_t>{0, 0, 1, 0, 0, 0, 0, 0, 0}) && (x.is_node == std::vector<uint8_t>{1, 0, 1, 1}));
        EdgeSet e;
        e.init(x);
        assert(host_walk(x, L.view(), e).what == DONE);
        assert(e.ne == 2 && (e.sp_ij == VI{0, 1, 0, 2}) && (e.dm_w == VF{.75f, .625f}) && (e.sp_d0 == VF{2.f, 3.f}) && (e.lost_ids() == VI{7}));
        assert((e.sk_idx == VI{1}) && (e.sk_of == VI{-1, 0, -1, -1}) && e.sk_node[0] == 0 && e.sk_node[1] == 2 && e.sk_node[2] == 1 && e.sk_node[3] == -1);
        assert(e.sk_om[0] == .875 / 1.625 && e.sk_om[1] == .5 / 1.625 && e.sk_om[2] == .25 / 1.625 && e.sk_om[3] == 0.0);
        same_edges(x, L);
        Stage2 s;                                                 // vertices: the nodes (6, 0, 3), then the skinned point 2, then the lost point
        s.lost_ids = e.lost_ids();
        stage2_vertices(x, s);
        assert(s.NV == 4 && (s.vert_of == VI{0, 3, 1, 2}) && (s.others == VI{1}));
        assert(lost_walk(x, L.view(), s).what == DONE && (s.un_ij == VI{4, 2, 4, 0, 4, 3}) && (s.un_w == VF{.8f, .7f, .5f}));
    }
}

static void check_statistics() {
    // all magnitudes equal (5): th = 0, every point sits at q3 + th -- status TRACKED, nothing moved, nothing fixed.  N = 1, 3, 4: the
    // order statistics' indices are (0, 0), (0, 2), (1, 3)
    for (int N : {1, 3, 4}) {
        std::vector<int32_t> f_map(N), f_st(N, T3);
        for (int i = 0; i < N; ++i) f_map[i] = i;
        FrameIndex x;
        assert(frame_index(x, N, N, f_map.data(), f_st.data(), nullptr).what == DONE);
        EdgeSet e;
        e.init(x);
        std::vector<double> delta(3 * N), chi(N, 0.0);
        for (int i = 0; i < N; ++i) { delta[3 * i] = 3.0; delta[3 * i + 1] = 0.0; delta[3 * i + 2] = -4.0; }
        std::vector<uint8_t> rflag(N, 3);
        std::vector<char> inl(N, 1);
        VF f_pos(3 * N, 1.f), map_pos(3 * N, 2.f);
        assert(deformation_statistics(x, e, delta.data(), chi.data(), nullptr, rflag.data(), inl.data(), f_st.data(), f_pos.data(), map_pos.data()) == 5.f);
        for (int i = 0; i < N; ++i) assert(f_st[i] == NRS_TRACKED && rflag[i] == 3 && inl[i] == 1);
        assert(f_pos == VF(3 * N, 1.f) && map_pos == VF(3 * N, 2.f));
    }
    // magnitudes 1, 2, 3, 100: q1 = 2, q3 = 100, th = 147: nobody reaches 247 -- all four move and are fixed; point 0 fails the chi2 gate
    const int32_t f_map[4] = {3, 2, 1, 0};
    int32_t f_st[4] = {T3, T3, T3, T3};
    FrameIndex x;
    assert(frame_index(x, 4, 4, f_map, f_st, nullptr).what == DONE);
    EdgeSet e;
    e.init(x);
    const double delta[12] = {1, 0, 0, 0, 2, 0, 0, 0, 3, 100, 0, 0}, chi[4] = {6.0, 5.0, 0, 0};
    uint8_t rflag[4] = {1, 1, 1, 1};
    char inl[4] = {1, 1, 1, 1};
    float f_pos[12] = {0}, map_pos[12] = {0};
    for (int i = 0; i < 12; ++i) f_pos[i] = .5f;
    assert(deformation_statistics(x, e, delta, chi, nullptr, rflag, inl, f_st, f_pos, map_pos) == 3.f);
    assert(inl[0] == 0 && inl[1] == 1 && f_st[0] == NRS_TRACKED && f_st[1] == T3 && f_st[2] == T3 && f_st[3] == T3);
    for (int i = 0; i < 4; ++i) assert(rflag[i] == (1 | VERTEX_FIXED));
    assert(f_pos[0] == 1.5f && f_pos[4] == 2.5f && f_pos[8] == 3.5f && f_pos[9] == 100.5f && f_pos[1] == .5f);
    assert(map_pos[9] == 1.5f && map_pos[7] == 2.5f && map_pos[5] == 3.5f && map_pos[0] == 100.5f);   // (frame point i is map point 3 - i)
}

// stage 2 in embedded mode: nodes 0..3, point 4 without a vertex, lost points 5 and 6, map point 7 not in the frame
static void check_stage2() {
    const int32_t f_map[7] = {0, 1, 2, 3, 4, 5, 6}, f_st[7] = {T3, T3, T3, T3, T3, NRS_TRACKED, NRS_TRACKED};
    const uint8_t f_node[7] = {1, 1, 1, 1, 0, 0, 0};
    FrameIndex x;
    assert(frame_index(x, 8, 7, f_map, f_st, f_node).what == DONE && x.N == 5 && x.M == 4);
    EdgeSet e;
    e.init(x);
    e.reset(3);
    e.connect(0, 1, .5f, 10.f); e.connect(1, 2, .25f, 20.f); e.connect(0, 3, .125f, 30.f);
    e.close();
    e.lost_flag[5] = e.lost_flag[6] = 1;
    Stage2 s;
    s.lost_ids = e.lost_ids();
    assert((s.lost_ids == VI{5, 6}));
    stage2_vertices(x, s);
    assert(s.NV == 5 && (s.vert_of == VI{0, 1, 2, 3, 4}) && (s.others == VI{4}));
    Lists L(8);
    L.row(5, {{4, .9f, 1.f, G}, {7, .8f, 1.f, G}, {6, .7f, 1.f, G}, {2, .6f, 1.f, G}});   // 7 and 6 are not optimised
    L.row(6, {{1, .3f, 1.f, G}}, true);
    const Status off = lost_walk(x, L.view(), s);
    assert(off.what == RAN_OFF && off.point == 6);                // one entry of a truncated list: not ended
    L.trunc[6] = 0;
    assert(lost_walk(x, L.view(), s).what == DONE && (s.un_ij == VI{5, 4, 5, 2, 6, 1}) && (s.un_w == VF{.9f, .6f, .3f}));
    // the statistics fixed nodes 0, 1 and 3: edge 0-1 and edge 0-3 lie between fixed vertices, edge 1-2 keeps the fixed vertex 1
    const uint8_t rflag[4] = {1 | VERTEX_FIXED, VERTEX_FIXED, 1, VERTEX_FIXED}, dm_active[3] = {1, 0, 1};
    double delta_v[12], delta[15], X0[12];
    float uv[8];
    for (int i = 0; i < 12; ++i) { delta_v[i] = 100 + i; X0[i] = 200 + i; }
    for (int i = 0; i < 15; ++i) delta[i] = 300 + i;
    for (int i = 0; i < 8; ++i) uv[i] = 400.f + i;
    Compact o;
    compact_stage2(x, s, e, rflag, dm_active, delta_v, delta, X0, uv, o);
    assert(o.M == 5 && (o.newid == VI{-1, 0, 1, -1, 2, 3, 4}));    // dense, in the old order
    assert((o.sp_ij == VI{0, 1}) && (o.dm_idx == VI{-1, -1, 0, 1}) && (o.sp_d0 == VF{20.f}) && (o.dm_w == VF{.25f}) && (o.dm_active == std::vector<uint8_t>{0}));
    assert((o.un_ij == VI{3, 2, 3, 1, 4, 0}) && (o.lm_pose == VI{0, 0, 0, 0, 0}));
    assert((o.rflag == std::vector<uint8_t>{VERTEX_FIXED, 1, VERTEX_FIXED, 0, 0}));   // (the point without a vertex is a constant)
    assert((o.x == std::vector<double>{103, 104, 105, 106, 107, 108, 312, 313, 314, 0, 0, 0, 0, 0, 0}));   // its interpolated deformation: delta of point 4
    assert((o.X0 == std::vector<double>{203, 204, 205, 206, 207, 208, 0, 0, 0, 0, 0, 0, 0, 0, 0}));
    assert((o.uv == VF{402.f, 403.f, 404.f, 405.f, 0, 0, 0, 0, 0, 0}));
}

static void check_empty() {
    const int32_t f_map[2] = {0, 1}, f_st[2] = {T3, T3};
    FrameIndex x;
    assert(frame_index(x, 2, 2, f_map, f_st, nullptr).what == DONE);
    Lists L(2);                                                   // no entry at all
    EdgeSet e;
    e.init(x);
    assert(host_walk(x, L.view(), e).what == DONE && e.ne == 0 && e.dm_idx.empty() && e.sp_ij.empty() && e.dm_w.empty() && e.sp_d0.empty());
    assert(e.lost_ids().empty());
    same_edges(x, L);
    Stage2 s;                                                     // no lost point, no edge: the free vertex alone
    stage2_vertices(x, s);
    assert(lost_walk(x, L.view(), s).what == DONE && s.un_ij.empty() && s.NV == 2);
    const uint8_t rflag[2] = {VERTEX_FIXED, 0};
    const double d[6] = {1, 2, 3, 4, 5, 6};
    const float uv[4] = {1, 2, 3, 4};
    Compact o;
    compact_stage2(x, s, e, rflag, nullptr, d, d, d, uv, o);
    assert(o.M == 1 && (o.newid == VI{-1, 0}) && o.sp_ij.empty() && o.dm_idx.empty() && o.un_ij.empty() && (o.x == std::vector<double>{4, 5, 6}));
}

int main() {
#ifdef NDEBUG
#error "track_check checks with assert: build it without NDEBUG"
#endif
    check_frame_index();
    check_parity_walk();
    check_walk_ends();
    check_skinning();
    check_permuted_frame();
    check_statistics();
    check_stage2();
    check_empty();
    std::printf("track_check OK: frame index, host walk, device-walk read-out, statistics, stage-2 walk and compaction\n");
    return 0;
}
