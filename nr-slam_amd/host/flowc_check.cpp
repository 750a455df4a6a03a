// Stand-alone check of the host half of nrs_dbscan_nd / nrs_flow_tracks_cluster (csrc/nrs_flowc_host.hpp) under AddressSanitizer + UBSan:
// `make flowc_check` (builds and runs it).  No HIP, no library.  `./flowc_check --texts` prints the refusals' formats, one per line
// (tests/test_flow_cluster_cases_cpu.py looks for them in the library).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../csrc/nrs_flowc_host.hpp"

using namespace nrs;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "--texts") == 0) {
        for (const char* t : {FLOWC_MSG_N, FLOWC_MSG_DIM, FLOWC_MSG_LENGTH, FLOWC_MSG_NULL, FLOWC_MSG_EPS, FLOWC_MSG_MIN_POINTS}) printf("%s\n", t);
        return 0;
    }
    char msg[256];
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- nrs_dbscan_nd's checks (a refusal reads no array: one float stands for every size)
    {
        float data[1] = {0};
        int32_t label[1], counts[2];
        auto ok = [&](int n, int dim, const void* d, double eps, int mp, const void* l, const void* c) { return dbscan_nd_check_args(n, dim, d, eps, mp, l, c, msg, sizeof msg); };
        CHECK(ok(1, 1, data, 1.0, 10, label, counts) == 0);
        CHECK(ok(0, 7, nullptr, 1.0, 10, nullptr, counts) == 0);                                       // an empty set is a valid call
        CHECK(ok(FLOWC_MAX_POINTS, FLOWC_MAX_DIM, data, 1.0, 1, label, counts) == 0);
        CHECK(ok(-1, 3, data, 1.0, 10, label, counts) != 0 && strcmp(msg, "nrs_dbscan_nd: n = -1 (0 .. 16384)") == 0);
        CHECK(ok(FLOWC_MAX_POINTS + 1, 3, data, 1.0, 10, label, counts) != 0 && strstr(msg, "n = 16385"));
        CHECK(ok(2, 0, data, 1.0, 10, label, counts) != 0 && strcmp(msg, "nrs_dbscan_nd: dim = 0 (1 .. 64)") == 0);
        CHECK(ok(2, 65, data, 1.0, 10, label, counts) != 0 && strstr(msg, "dim = 65"));
        CHECK(ok(0, 0, nullptr, 1.0, 10, nullptr, counts) != 0);                                       // (dim is checked on an empty set too)
        CHECK(ok(2, 3, nullptr, 1.0, 10, label, counts) != 0 && strcmp(msg, "nrs_dbscan_nd: null pointer") == 0);
        CHECK(ok(2, 3, data, 1.0, 10, nullptr, counts) != 0);
        CHECK(ok(2, 3, data, 1.0, 10, label, nullptr) != 0);
        CHECK(ok(0, 3, nullptr, 1.0, 10, nullptr, nullptr) != 0);
        for (double e : {0.0, -1.0, inf, -inf, nan}) CHECK(ok(2, 3, data, e, 10, label, counts) != 0 && strstr(msg, "eps") && strstr(msg, "not a positive finite number"));
        CHECK(ok(2, 3, data, 1.0, 0, label, counts) != 0 && strcmp(msg, "nrs_dbscan_nd: min_points = 0 (at least 1)") == 0);
    }
    // ---- nrs_flow_tracks_cluster's checks
    {
        float xy[4] = {0, 0, 1, 1};
        int32_t label[1], counts[2];
        auto ok = [&](int n, int len, const void* t, const void* l, const void* c) { return flow_tracks_check_args(n, len, t, l, c, msg, sizeof msg); };
        CHECK(ok(1, 2, xy, label, counts) == 0);
        CHECK(ok(0, 33, nullptr, nullptr, counts) == 0);
        CHECK(ok(FLOWC_MAX_POINTS, 33, xy, label, counts) == 0);
        CHECK(ok(-1, 2, xy, label, counts) != 0 && strcmp(msg, "nrs_flow_tracks_cluster: n = -1 (0 .. 16384)") == 0);
        CHECK(ok(FLOWC_MAX_POINTS + 1, 2, xy, label, counts) != 0);
        CHECK(ok(1, 1, xy, label, counts) != 0 && strcmp(msg, "nrs_flow_tracks_cluster: length = 1 keypoints (2 .. 33)") == 0);
        CHECK(ok(1, 34, xy, label, counts) != 0 && strstr(msg, "length = 34"));
        CHECK(ok(1, 0, xy, label, counts) != 0 && ok(1, -5, xy, label, counts) != 0);
        CHECK(ok(1, 2, nullptr, label, counts) != 0 && strcmp(msg, "nrs_flow_tracks_cluster: null pointer") == 0);
        CHECK(ok(1, 2, xy, nullptr, counts) != 0);
        CHECK(ok(1, 2, xy, label, nullptr) != 0);
    }
    // ---- the dimension and length arithmetic, the eps rule
    CHECK(FLOWC_MIN_LENGTH == 2 && FLOWC_MAX_LENGTH == 33 && FLOWC_MIN_POINTS == 10);
    CHECK(flowc_dim(2) == 2 && flowc_dim(11) == 20 && flowc_dim(31) == 60 && flowc_dim(FLOWC_MAX_LENGTH) == FLOWC_MAX_DIM);
    for (int len = FLOWC_MIN_LENGTH; len <= FLOWC_MAX_LENGTH; ++len) {
        const int dim = flowc_dim(len);
        CHECK(dim >= 1 && dim <= FLOWC_MAX_DIM && dim % 2 == 0);
        const float stored = (float)(0.1 * (double)dim);                  // the reference's `float eps = 0.1 * dim`
        CHECK(flowc_eps(dim) == (double)stored);
    }
    CHECK(flowc_eps(10) == 1.0);                                          // 0.1 * 10 rounds to 1 in double already
    CHECK(flowc_eps(2) == (double)0.2f && flowc_eps(2) != 0.2);           // the float's value, not the double product
    CHECK(flowc_eps(60) == 6.0);
    // ---- the rows: seven pieces on 256-byte boundaries, in order, none overlapping; the sum the stereo start has always reserved
    for (size_t cap : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1100, (size_t)FLOWC_MAX_POINTS}) {
        const DbRowsLayout L(cap);
        CHECK(L.W == (cap + 63) / 64 && L.adj == 0);
        const size_t off[8] = {L.adj, L.coremask, L.core, L.lab, L.rawid, L.size, L.rank, L.bytes};
        const size_t need[7] = {8 * cap * L.W, 8 * 256, 4 * cap, 4 * cap, 4 * cap, 4 * (cap + 1), 4 * (cap + 1)};
        for (int k = 0; k < 7; ++k) CHECK(off[k] % 256 == 0 && off[k + 1] >= off[k] + need[k] && off[k + 1] - off[k] < need[k] + 256);
        auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
        CHECK(L.bytes == pad(8 * cap * L.W) + pad(8 * 256) + 3 * pad(4 * cap) + 2 * pad(4 * (cap + 1)));
    }
    CHECK(DbRowsLayout(FLOWC_MAX_POINTS).coremask == (size_t)32 << 20);   // 16384 rows of 256 words: 32 MiB
    // ---- a call's scratch: upload, download and rows follow each other without overlap; the flows lie inside the download
    for (size_t n : {(size_t)1, (size_t)5, (size_t)65, (size_t)1100, (size_t)FLOWC_MAX_POINTS})
        for (size_t len : {(size_t)0, (size_t)2, (size_t)31, (size_t)33}) {
            const size_t dim = len ? (size_t)flowc_dim((int)len) : 60;
            const FlowcScratch S(n, dim, len);
            CHECK(S.m == 0 && S.in == 256 && S.in_floats == (len ? n * len * 2 : n * dim) && S.up_bytes == 256 + 4 * S.in_floats);
            CHECK(S.out % 256 == 0 && S.out >= S.up_bytes && S.flows_word == 4 + n && S.out_words == 4 + n + (len ? n * dim : 0));
            CHECK(S.rows % 256 == 0 && S.rows >= S.out + 4 * S.out_words && S.bytes == S.rows + DbRowsLayout(n).bytes);
            CHECK((S.out + 4 * S.flows_word) % 4 == 0);
        }
    // ---- the tile and the queries of a workgroup
    CHECK(FLOWC_TILE == 64 && FLOWC_TILE_STRIDE % 2 == 1 && FLOWC_TILE_STRIDE >= FLOWC_TILE);
    CHECK((size_t)FLOWC_MAX_DIM * FLOWC_TILE_STRIDE * 4 + (size_t)FLOWC_MAX_DIM * 16 * 8 <= 64 * 1024);      // tile + the widest query block, bytes of LDS
    CHECK(flowc_queries_per_wave(1) == 1 && flowc_queries_per_wave(1024) == 1 && flowc_queries_per_wave(1025) == 2 && flowc_queries_per_wave(4096) == 2 &&
          flowc_queries_per_wave(4097) == 4 && flowc_queries_per_wave(FLOWC_MAX_POINTS) == 4);
    printf(fails ? "flowc_check: %d check(s) FAILED\n" : "flowc_check OK\n", fails);
    return fails ? 1 : 0;
}
