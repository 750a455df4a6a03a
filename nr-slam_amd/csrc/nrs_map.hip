// Mapping::FrameMapping = Mapping::LandmarkTriangulation (reference modules/mapping/mapping.cc:65-236) in one call on the flat
// TemporalBuffer of f2 (nrs_triang.hip), uploaded once:
//   k_map_candidates  one workgroup: GetTriangulationCandidatesIds (temporal_buffer.cc:62-74) -- the ids whose last status is TRACKED,
//                     ascending, by a workgroup scan
//   k_map_close       one wave per candidate: the two bits of the "close features" test, read by both legs
//   k_map_rigid       one lane per candidate: CheckRigidity (temporal_buffer.cc:218-227) and the rigid
//                     mid-point triangulation with its gates (mapping.cc:117-190)
//   k_triangulate     (nrs_triang.hip, one wave per candidate) the deformable leg (:97-115) on the same device buffer and list
//   k_map_vote        one workgroup: "NaN." (:101-102), the two counts, the rigid / deformable vote (:192-209) and the accepted list
//                     (:211-236) compacted in candidate order by a workgroup scan -- no atomics, the order is the reference's
// and one download of the packed result (nrs_map_host.hpp).  Everything behind the upload is map_run, which nrs_map_frame_tbuf
// (nrs_tbuf.hip) calls on the tables it rebuilds from the resident buffer; k_map_row_ids then turns its two id lists into keypoint ids.  The fp32 steps use the operation order of oracle/triang_oracle.py
// (contraction off); every comparison is written as the reference writes it, so a NaN passes the gates it passes there.
#include <cmath>
#include <vector>
#include "nrs_ctx.hpp"
#include "nrs_device.hpp"
#include "nrs_geom_f32.hpp"
#include "nrs_map_host.hpp"
#include "nrs_triang_dev.hpp"

namespace nrs {

constexpr int MAP_T = 1024;                 // threads of the two single-workgroup kernels
constexpr int MAP_W = MAP_T / 64;

struct MapArgs {
    TriArgs T;                              // the device buffer, the candidate list and the deformable leg's outputs
    const float* deform_mag;                // F
    float rpp, rigidity_th;
    int index_snapshot;
    int* hdr; int* cand; int* r_st; float* r_xyz; int* a_id; float* a_xyz;
    uint8_t* close_bits;                    // n_cand: tb_scan_close, computed once for both legs
};

// exclusive scan of one int per thread over the workgroup (ascending thread order); total = the sum
__device__ inline int map_excl_scan(int v, int* sm, int& total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int y = __shfl_up(x, off, 64); if (lane >= off) x += y; }
    __syncthreads();                                              // (sm may still be read from an earlier scan)
    if (lane == 63) sm[w] = x;
    __syncthreads();
    if (tid == 0) { int acc = 0; for (int i = 0; i < MAP_W; ++i) { const int t = sm[i]; sm[i] = acc; acc += t; } sm[MAP_W] = acc; }
    __syncthreads();
    total = sm[MAP_W];
    return sm[w] + x - v;
}

__global__ __launch_bounds__(MAP_T) void k_map_candidates(MapArgs A, int n_cand) {
    __shared__ int sm[MAP_W + 1];
    const int n = A.T.n, tid = threadIdx.x;
    const int chunk = (n + MAP_T - 1) / MAP_T;
    const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
    int cnt = 0;
    for (int i = lo; i < hi; ++i) cnt += A.T.status[i] == NRS_TRACKED;
    int total;
    int pos = map_excl_scan(cnt, sm, total);
    for (int i = lo; i < hi; ++i)
        if (A.T.status[i] == NRS_TRACKED) { if (pos < n_cand) A.cand[pos] = i; ++pos; }
    if (tid == 0) A.hdr[0] = total;                                // (== n_cand: the host counted the same flags)
}

// the close-features scan of every candidate, one wave each: both legs read the two bits from here
__global__ __launch_bounds__(64) void k_map_close(MapArgs A) {
    const int ci = blockIdx.x;
    if (ci >= A.T.n_cand) return;
    const int bits = tb_scan_close(A.T, A.T.cand[ci], threadIdx.x, 64);
    const int b0 = __any(bits & 1), b1 = __any(bits & 2);
    if (threadIdx.x == 0) A.close_bits[ci] = (uint8_t)((b0 ? 1 : 0) | (b1 ? 2 : 0));
}

__global__ __launch_bounds__(64) void k_map_rigid(MapArgs A) {
#pragma clang fp contract(off)
    const int ci = blockIdx.x * 64 + threadIdx.x;
    if (ci >= A.T.n_cand) return;
    const TriArgs& T = A.T;
    const int cand = T.cand[ci], n = T.n;
    auto finish = [&](int code, float x, float y, float z) {
        A.r_st[ci] = code;
        A.r_xyz[3 * ci] = x; A.r_xyz[3 * ci + 1] = y; A.r_xyz[3 * ci + 2] = z;
    };
    // mapping.cc:90-95: only the emptiness of GetClosestMapPointsToFeature(id, 10, 20, 500) is used
    const int bits = A.close_bits[ci];
    if ((bits & 1) || !(bits & 2)) { finish(NRS_MAP_CLOSE, 0, 0, 0); return; }
    // GetFeatureTrack: front() = the OLDEST snapshot holding the id (the reference's `current_`), back() = the NEWEST (`previous_`)
    int first = -1, lastf = -1;
    for (int f = 0; f < T.F; ++f)
        if (T.has_kp[(size_t)f * n + cand]) { if (first < 0) first = f; lastf = f; }
    // CheckRigidity(front, back, th): every snapshot between the two, whether or not it holds the feature
    bool rigid = true;
    for (int f = first; f <= lastf; ++f)
        if (A.deform_mag[f] > A.rigidity_th) rigid = false;
    if (!rigid) { finish(NRS_MAP_NOT_RIGID, 0, 0, 0); return; }
    auto pose_of = [&](int f) { Se3f P; for (int k = 0; k < 4; ++k) P.q[k] = T.poses[7 * f + k]; for (int k = 0; k < 3; ++k) P.t[k] = T.poses[7 * f + 4 + k]; return P; };
    const float* kc = T.kp_xy + 2 * ((size_t)first * n + cand);
    const float* kp = T.kp_xy + 2 * ((size_t)lastf * n + cand);
    float cr[3], pr[3];
    unproject_f32(T.cam, kc[0], kc[1], cr);
    unproject_f32(T.cam, kp[0], kp[1], pr);
    float nn = normf3(cr); cr[0] /= nn; cr[1] /= nn; cr[2] /= nn;
    nn = normf3(pr); pr[0] /= nn; pr[1] /= nn; pr[2] /= nn;
    const Se3f Tc = pose_of(first), Tp = pose_of(lastf);
    float X[3];
    triangulate_mid_point_f32(pr, cr, Tp, Tc, X);                  // TriangulateMidPoint(previous_ray, current_ray, previous_T, current_T): never fails
    const Se3f Tci = se3_inv(Tc), Tpi = se3_inv(Tp);
    const float n1[3] = {X[0] - Tci.t[0], X[1] - Tci.t[1], X[2] - Tci.t[2]}, n2[3] = {X[0] - Tpi.t[0], X[1] - Tpi.t[1], X[2] - Tpi.t[2]};
    const float par = rays_parallax_f32(n1, n2);
    if (par < A.rpp * 10.f || par > A.rpp * 20.f) { finish(NRS_MAP_PARALLAX, 0, 0, 0); return; }
    float pc[3], u, v;
    se3_point(Tp, X, pc);
    if (pc[2] < 0) { finish(NRS_MAP_DEPTH_PREVIOUS, 0, 0, 0); return; }
    project_f32(T.cam, pc[0], pc[1], pc[2], u, v);
    float ex = kp[0] - u, ey = kp[1] - v;
    if ((double)(ex * ex + ey * ey) > 5.991) { finish(NRS_MAP_REPROJ_PREVIOUS, 0, 0, 0); return; }
    se3_point(Tc, X, pc);
    if (pc[2] < 0) { finish(NRS_MAP_DEPTH_CURRENT, 0, 0, 0); return; }
    project_f32(T.cam, pc[0], pc[1], pc[2], u, v);
    ex = kc[0] - u; ey = kc[1] - v;
    if ((double)(ex * ex + ey * ey) > 5.991) { finish(NRS_MAP_REPROJ_CURRENT, 0, 0, 0); return; }
    finish(NRS_MAP_OK, X[0], X[1], X[2]);
}

__device__ inline bool map_has_nan(const float* p) { return p[0] != p[0] || p[1] != p[1] || p[2] != p[2]; }

__global__ __launch_bounds__(MAP_T) void k_map_vote(MapArgs A) {
    __shared__ int sm[MAP_W + 1];
    const int nc = A.T.n_cand, tid = threadIdx.x;
    const int chunk = (nc + MAP_T - 1) / MAP_T;
    const int lo = min(nc, tid * chunk), hi = min(nc, lo + chunk);
    int n_r = 0, n_d = 0;
    for (int i = lo; i < hi; ++i) {
        if (A.T.o_status[i] == TR_OK && map_has_nan(A.T.o_xyz + 3 * i)) A.T.o_status[i] = TR_NAN;     // mapping.cc:101-102 "NaN."
        n_r += A.r_st[i] == NRS_MAP_OK;
        n_d += A.T.o_status[i] == TR_OK;
    }
    int n_rigid, n_def;
    map_excl_scan(n_r, sm, n_rigid);
    map_excl_scan(n_d, sm, n_def);
    // mapping.cc:195, 201: int against double (1.5 * int)
    const int mode = (double)n_rigid > 1.5 * (double)n_def ? MAP_MODE_RIGID : ((double)n_def >= 1.5 * (double)n_rigid ? MAP_MODE_DEFORMABLE : MAP_MODE_NONE);
    const int snap = A.index_snapshot < 0 ? A.T.F - 1 : A.index_snapshot;
    auto accepted = [&](int i) -> bool {
        if (mode == MAP_MODE_NONE) return false;
        const bool ok = mode == MAP_MODE_RIGID ? A.r_st[i] == NRS_MAP_OK : A.T.o_status[i] == TR_OK;
        const float* p = mode == MAP_MODE_RIGID ? A.r_xyz + 3 * i : A.T.o_xyz + 3 * i;
        // :214 hasNaN, :219 GetLandmarkIndexInFrame(current_frame_id, candidate)
        return ok && !map_has_nan(p) && A.T.has_kp[(size_t)snap * A.T.n + A.T.cand[i]];
    };
    int cnt = 0;
    for (int i = lo; i < hi; ++i) cnt += accepted(i);
    int n_acc;
    int pos = map_excl_scan(cnt, sm, n_acc);
    for (int i = lo; i < hi; ++i)
        if (accepted(i)) {
            const float* p = mode == MAP_MODE_RIGID ? A.r_xyz + 3 * i : A.T.o_xyz + 3 * i;
            A.a_id[pos] = A.T.cand[i];
            A.a_xyz[3 * pos] = p[0]; A.a_xyz[3 * pos + 1] = p[1]; A.a_xyz[3 * pos + 2] = p[2];
            ++pos;
        }
    if (tid == 0) { A.hdr[1] = n_rigid; A.hdr[2] = n_def; A.hdr[3] = mode; A.hdr[4] = n_acc; A.hdr[5] = 0; A.hdr[6] = 0; A.hdr[7] = 0; }
}

// the ids of the resident buffer's callers: rows -> keypoint ids, in place, once nothing reads the two lists as rows any more
__global__ __launch_bounds__(256) void k_map_row_ids(int n_cand, const int* __restrict__ hdr, const int* __restrict__ row_id, int* cand, int* a_id) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cand) return;
    cand[i] = row_id[cand[i]];
    if (i < hdr[4]) a_id[i] = row_id[a_id[i]];
}

size_t map_ws_bytes(int nc) { return 4 * MapLayout((size_t)nc).words + (size_t)nc + 1024; }

// Everything of nrs_map_frame behind the upload, for both of its forms: T holds the camera, the sizes and the device-side flat buffer,
// ws (256-byte aligned, map_ws_bytes(nc) bytes) takes the close bits and the packed result.  row_id (device, T.n ints) or null: the two id
// lists leave as row_id[row] (nrs_map_frame_tbuf).
int map_run(nrs_ctx* c, const char* who, const TriArgs& T, const float* d_deform_mag, char* ws, int nc, float rad_per_pixel, float rigidity_th,
            int index_snapshot, const int* d_row_id, const MapOut& out) {
    const MapLayout L((size_t)nc);
    StageTimer tm{c, who, true};                                   // (NRS_TIMING only: the marks wait for the stream)
    MapArgs A;
    A.T = T;
    A.deform_mag = d_deform_mag;
    char* p = ws;
    A.close_bits = reinterpret_cast<uint8_t*>(p);
    p += ((size_t)nc + 255) / 256 * 256;
    int* pk = reinterpret_cast<int*>(p);                           // the packed result
    A.hdr = pk; A.cand = pk + L.cand; A.r_st = pk + L.r_st; A.r_xyz = reinterpret_cast<float*>(pk + L.r_xyz);
    A.a_id = pk + L.a_id; A.a_xyz = reinterpret_cast<float*>(pk + L.a_xyz);
    A.T.n_cand = nc; A.T.cand = A.cand; A.T.o_status = pk + L.d_st; A.T.o_xyz = reinterpret_cast<float*>(pk + L.d_xyz); A.T.o_dbg = nullptr;
    A.rpp = rad_per_pixel; A.rigidity_th = rigidity_th; A.index_snapshot = index_snapshot;
    NRS_HIP(c, hipMemsetAsync(pk, 0, 4 * L.words, c->stream));
    hipLaunchKernelGGL(k_map_candidates, dim3(1), dim3(MAP_T), 0, c->stream, A, nc);
    A.T.close_bits = A.close_bits;
    hipLaunchKernelGGL(k_map_close, dim3(nc), dim3(64), 0, c->stream, A);
    hipLaunchKernelGGL(k_map_rigid, dim3((nc + 63) / 64), dim3(64), 0, c->stream, A);
    NRS_HIP(c, hipGetLastError());
    NRS_TRY(tri_launch(c, A.T));
    hipLaunchKernelGGL(k_map_vote, dim3(1), dim3(MAP_T), 0, c->stream, A);
    if (d_row_id) hipLaunchKernelGGL(k_map_row_ids, dim3((nc + 255) / 256), dim3(256), 0, c->stream, nc, A.hdr, d_row_id, A.cand, A.a_id);
    NRS_HIP(c, hipGetLastError());
    tm("mapping kernels");
    std::vector<int32_t> h(L.words);
    NRS_HIP(c, hipMemcpyAsync(h.data(), pk, 4 * L.words, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (map_unpack(h.data(), nc, out) != 0) return c->fail(NRS_ERR_STATE, "%s: the device's result header does not match the %d candidates counted", who, nc);
    tm("download");
    return NRS_OK;
}

}  // namespace nrs

using namespace nrs;

extern "C" int nrs_map_frame(nrs_ctx* c, const nrs_camera* cam, int32_t n_frames, const float* poses, int32_t n_ids, const uint8_t* has_kp,
                             const float* kp_xy, const uint8_t* has_lm, const float* lm_xyz, const int32_t* last_status, const float* deform_mag,
                             float rad_per_pixel, float rigidity_th, int32_t min_track, int32_t index_snapshot, int32_t* n_cand,
                             int32_t* cand_ids, int32_t* rigid_status, float* rigid_xyz, int32_t* deform_status, float* deform_xyz,
                             int32_t counts[3], int32_t* n_accepted, int32_t* accepted_ids, float* accepted_xyz) {
    if (!c) return NRS_ERR_INVALID;
    MapIn in{cam, cam ? cam->model : 0, n_frames, n_ids, poses, has_kp, kp_xy, has_lm, lm_xyz, last_status, deform_mag, rad_per_pixel, rigidity_th,
             index_snapshot, {n_cand, cand_ids, rigid_status, rigid_xyz, deform_status, deform_xyz, counts, n_accepted, accepted_ids, accepted_xyz}};
    int nc = 0;
    char msg[256];
    if (map_check_args(in, &nc, msg, sizeof(msg)) != 0) return c->fail(NRS_ERR_INVALID, "%s", msg);
    const MapOut out{n_cand, cand_ids, rigid_status, rigid_xyz, deform_status, deform_xyz, counts, n_accepted, accepted_ids, accepted_xyz};
    if (nc == 0) {                                                 // no candidates: 0 / 0 votes deformable (mapping.cc:201) and nothing is launched
        *n_cand = 0; *n_accepted = 0;
        counts[0] = 0; counts[1] = 0; counts[2] = MAP_MODE_DEFORMABLE;
        return NRS_OK;
    }
    const size_t fbytes = (sizeof(float) * (size_t)n_frames + 255) / 256 * 256;
    DevBuf big;                                                    // (freed when the call returns)
    TriArgs T;
    char* p = nullptr;
    StageTimer tm{c, "nrs_map_frame", true};
    NRS_TRY(tri_upload(c, big, fbytes + map_ws_bytes(nc), cam, n_frames, poses, n_ids, has_kp, kp_xy, has_lm, lm_xyz, last_status, min_track, T, &p));
    const float* d_mag = reinterpret_cast<float*>(p);
    NRS_HIP(c, hipMemcpyAsync(p, deform_mag, sizeof(float) * (size_t)n_frames, hipMemcpyHostToDevice, c->stream));
    p += fbytes;
    tm("upload");
    return map_run(c, "nrs_map_frame", T, d_mag, p, nc, rad_per_pixel, rigidity_th, index_snapshot, nullptr, out);
}

extern "C" int nrs_map_grow_graph(nrs_ctx* c, nrs_rgraph* g, const float* pos, int32_t n_new, const int32_t* new_ids, int32_t n_other,
                                  const int32_t* other_ids) {
    if (!c) return NRS_ERR_INVALID;
    if (!g) return c->fail(NRS_ERR_INVALID, "nrs_map_grow_graph: null graph");
    return nrs_rgraph_add_edges(g, pos, n_new, new_ids, n_other, other_ids);
}
