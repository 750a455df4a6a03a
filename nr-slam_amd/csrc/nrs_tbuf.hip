// TemporalBuffer (reference modules/map/temporal_buffer.cc:28-74) as a device-resident object: InsertSnapshotFromFrame is ONE upload of
// the frame's kept entries into a ring slot (pinned staging, nrs_tbuf_host.hpp), and frame mapping reads the buffer where it lies.
// The dense table the mapping kernels take (nrs_triang_dev.hpp TriArgs) is rebuilt per call on the device from the compact slots:
//   (one fill)      the presence table over the id span and everything under a flag cleared
//   k_tb_presence   one lane per (snapshot, entry): presence[id - lowest] = 1 -- plain word stores; ids are unique per snapshot and a
//                   second snapshot writes the same word, so no atomics
//   k_tb_rows       one workgroup: exclusive scan of the presence table in trips of 1024, in place: id -> row (ascending ids, the
//                   order of TemporalBuffer.flat); last_status filled with BAD; the poses and deformation magnitudes in snapshot order
//   k_tb_scatter    one lane per (snapshot, entry): coalesced reads of the slot's sections, has_kp / kp_xy / has_lm / lm_xyz at
//                   [snapshot][row]; for the last snapshot the status and the row -> id table
// and then the launches of nrs_map_frame, unchanged (map_run, nrs_map.hip), whose two id lists leave as keypoint ids.
// The host knows the number of distinct ids (reference counts), the span and the candidate count: nothing is read back before the result.
#include <type_traits>
#include <new>
#include <vector>
#include "nrs_ctx.hpp"
#include "nrs_device.hpp"
#include "nrs_map_host.hpp"
#include "nrs_tbuf_host.hpp"
#include "nrs_triang_dev.hpp"

struct nrs_tbuf {
    nrs_ctx* c = nullptr;
    nrs::TbufHost h;
    nrs::DevBuf slots;               // n_slots x tb_slot_words(h.cap) words
    nrs::DevBuf ws;                  // the dense tables (TbLayout) + the mapping call's work area
    nrs::PinBuf pin;                 // pinned staging of one snapshot
    nrs::Event ev_up;                // behind the last upload from `pin`
    bool up_pending = false;
    std::vector<uint64_t> seen;      // scratch of the duplicate check
};

namespace nrs {

constexpr int TB_T = 1024;
constexpr int TB_BAD = 3;            // LandmarkStatus::BAD: an id the last snapshot does not hold

struct TbSnaps { int F; int m[MAP_MAXF]; int off[MAP_MAXF + 1]; int slot[MAP_MAXF]; };
struct TbFlat {
    TbSnaps S;
    const uint32_t* slots; size_t slot_words;
    int id_lo, span, n;
    int* row; uint8_t* has_kp; float* kp_xy; uint8_t* has_lm; float* lm_xyz; int* status; int* row_id; float* poses; float* mag;
};
static_assert(std::is_trivially_copyable_v<TbFlat>, "passed to kernels by value: plain pointers, never an owner");

// entry e of the concatenated snapshots -> (snapshot f, entry j); false past the end
__device__ inline bool tb_entry(const TbSnaps& S, int e, int& f, int& j) {
    if (e >= S.off[S.F]) return false;
    f = 0;
    while (f + 1 < S.F && e >= S.off[f + 1]) ++f;
    j = e - S.off[f];
    return true;
}

__global__ __launch_bounds__(256) void k_tb_presence(TbFlat A) {
    int f, j;
    if (!tb_entry(A.S, blockIdx.x * 256 + threadIdx.x, f, j)) return;
    const uint32_t* s = A.slots + (size_t)A.S.slot[f] * A.slot_words + TBUF_HEAD;
    const unsigned k = (unsigned)((int)s[j] - A.id_lo);
    if (k < (unsigned)A.span) A.row[k] = 1;
}

__global__ __launch_bounds__(TB_T) void k_tb_rows(TbFlat A) {
    __shared__ int sm[TB_T / 64 + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int carry = 0;
    for (int base = 0; base < A.span; base += TB_T) {
        const int i = base + tid;
        const int v = i < A.span ? A.row[i] : 0;
        int x = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int y = __shfl_up(x, off, 64); if (lane >= off) x += y; }
        __syncthreads();                                           // (sm is still read by the trip before)
        if (lane == 63) sm[w] = x;
        __syncthreads();
        if (tid == 0) { int acc = 0; for (int q = 0; q < TB_T / 64; ++q) { const int t = sm[q]; sm[q] = acc; acc += t; } sm[TB_T / 64] = acc; }
        __syncthreads();
        if (i < A.span) A.row[i] = carry + sm[w] + x - v;
        carry += sm[TB_T / 64];
    }
    for (int i = tid; i < A.n; i += TB_T) A.status[i] = TB_BAD;
    if (tid < A.S.F * TBUF_HEAD) {
        const int f = tid / TBUF_HEAD, k = tid % TBUF_HEAD;
        const float v = __uint_as_float(A.slots[(size_t)A.S.slot[f] * A.slot_words + k]);
        if (k < 7) A.poses[7 * f + k] = v;
        else A.mag[f] = v;
    }
}

__global__ __launch_bounds__(256) void k_tb_scatter(TbFlat A) {
    int f, j;
    if (!tb_entry(A.S, blockIdx.x * 256 + threadIdx.x, f, j)) return;
    const size_t m = (size_t)A.S.m[f];
    const uint32_t* id = A.slots + (size_t)A.S.slot[f] * A.slot_words + TBUF_HEAD;
    const uint32_t* fl = id + m;
    const float* xy = reinterpret_cast<const float*>(fl + m);
    const float* xyz = xy + 2 * m;
    const int kid = (int)id[j];
    const unsigned k = (unsigned)(kid - A.id_lo);
    if (k >= (unsigned)A.span) return;
    const int r = A.row[k];
    if ((unsigned)r >= (unsigned)A.n) return;                      // (cannot happen: the host counted the same ids)
    const uint32_t flags = fl[j];
    const size_t at = (size_t)f * A.n + r;
    A.has_kp[at] = 1;
    A.kp_xy[2 * at] = xy[2 * j]; A.kp_xy[2 * at + 1] = xy[2 * j + 1];
    if (flags & TBUF_HAS_LM) {
        A.has_lm[at] = 1;
        A.lm_xyz[3 * at] = xyz[3 * j]; A.lm_xyz[3 * at + 1] = xyz[3 * j + 1]; A.lm_xyz[3 * at + 2] = xyz[3 * j + 2];
    }
    A.row_id[r] = kid;                                             // (every snapshot holding the id writes the same word)
    if (f == A.S.F - 1) A.status[r] = (int)(flags & 0xFF);
}

// the pinned staging area holds a snapshot of `words` words; an upload still reading it is waited for first
static int tb_stage(nrs_tbuf* tb, size_t words) {
    nrs_ctx* c = tb->c;
    if (tb->up_pending) { NRS_HIP(c, hipEventSynchronize(tb->ev_up.get())); tb->up_pending = false; }
    if (c->ensure_pinned(tb->pin, 4 * words, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return c->fail(NRS_ERR_ALLOC, "nrs_tbuf: %zu bytes of pinned host memory", 4 * words);
    }
    return NRS_OK;
}

// slots of new_cap entries each, the held blocks moved over on the device; a failure leaves the buffer as it was
static int tb_grow_slots(nrs_tbuf* tb, int new_cap) {
    nrs_ctx* c = tb->c;
    const size_t ow = tb_slot_words(tb->h.cap), nw = tb_slot_words(new_cap);
    DevBuf nb;
    NRS_TRY(c->ensure(nb, 4 * nw * (size_t)tb->h.n_slots()));
    hipError_t e = hipSuccess;
    if (tb->slots.p && !tb->h.snaps.empty())
        e = hipMemcpy2DAsync(nb.p, 4 * nw, tb->slots.p, 4 * ow, 4 * ow, (size_t)tb->h.n_slots(), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return c->fail(NRS_ERR_HIP, "nrs_tbuf: moving the slots: %s", hipGetErrorString(e));   // (nb frees the new slots)
    tb->slots = std::move(nb);                                     // the old slots are freed here
    return NRS_OK;
}

// The dense tables of the held snapshots in tb->ws (grown to hold `extra` more bytes behind them), enqueued on the context's stream.
// n = 0 (no snapshot holds an id): nothing is launched and only L is set.
static int tb_flatten(nrs_tbuf* tb, size_t extra, TbFlat& A, TbLayout& L) {
    nrs_ctx* c = tb->c;
    const TbufHost& h = tb->h;
    const int F = (int)h.snaps.size(), n = h.n_ids();
    int32_t lo = 0, hi = -1;
    const bool held = tb_span(h, &lo, &hi);
    const size_t span = held ? (size_t)((int64_t)hi - lo + 1) : 0;
    L = TbLayout((size_t)F, (size_t)n, span);
    size_t want = 4096;                                            // sized in doubled steps: a steady state allocates nothing
    while (want < L.bytes + extra) want *= 2;
    NRS_TRY(c->ensure(tb->ws, want));
    char* b = tb->ws.as<char>();
    A.S.F = F;
    A.S.off[0] = 0;
    for (int f = 0; f < MAP_MAXF; ++f) {
        A.S.m[f] = f < F ? (int)h.snaps[f].ids.size() : 0;
        A.S.slot[f] = f < F ? h.snaps[f].slot : 0;
        A.S.off[f + 1] = A.S.off[f] + A.S.m[f];
    }
    A.slots = tb->slots.as<uint32_t>(); A.slot_words = tb_slot_words(h.cap);
    A.id_lo = lo; A.span = (int)span; A.n = n;
    A.row = reinterpret_cast<int*>(b + L.row);
    A.has_kp = reinterpret_cast<uint8_t*>(b + L.has_kp); A.has_lm = reinterpret_cast<uint8_t*>(b + L.has_lm);
    A.kp_xy = reinterpret_cast<float*>(b + L.kp_xy); A.lm_xyz = reinterpret_cast<float*>(b + L.lm_xyz);
    A.status = reinterpret_cast<int*>(b + L.status); A.row_id = reinterpret_cast<int*>(b + L.row_id);
    A.poses = reinterpret_cast<float*>(b + L.poses); A.mag = reinterpret_cast<float*>(b + L.mag);
    if (n == 0) return NRS_OK;
    const int E = A.S.off[F];
    NRS_HIP(c, hipMemsetAsync(b, 0, L.zero_end, c->stream));
    hipLaunchKernelGGL(k_tb_presence, dim3((E + 255) / 256), dim3(256), 0, c->stream, A);
    hipLaunchKernelGGL(k_tb_rows, dim3(1), dim3(TB_T), 0, c->stream, A);
    hipLaunchKernelGGL(k_tb_scatter, dim3((E + 255) / 256), dim3(256), 0, c->stream, A);
    NRS_HIP(c, hipGetLastError());
    return NRS_OK;
}

}  // namespace nrs

using namespace nrs;

extern "C" int nrs_tbuf_create(nrs_ctx* c, int32_t max_buffer_size, nrs_tbuf** out) {
    if (!c || !out) return NRS_ERR_INVALID;
    *out = nullptr;
    char msg[256];
    if (tb_check_create(max_buffer_size, msg, sizeof(msg)) != 0) return c->fail(NRS_ERR_INVALID, "%s", msg);
    NRS_HIP(c, hipSetDevice(c->device));
    nrs_tbuf* tb = new (std::nothrow) nrs_tbuf();
    if (!tb) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    tb->c = c;
    tb_reset(tb->h, max_buffer_size);
    int rc = tb_grow_slots(tb, tb->h.cap);
    if (rc == NRS_OK) rc = tb_stage(tb, tb_slot_words(tb->h.cap));
    if (rc == NRS_OK && event_create(tb->ev_up) != hipSuccess) rc = c->fail(NRS_ERR_HIP, "nrs_tbuf_create: hipEventCreate failed");
    if (rc != NRS_OK) { nrs_tbuf_destroy(tb); return rc; }
    *out = tb;
    return NRS_OK;
}

extern "C" void nrs_tbuf_destroy(nrs_tbuf* tb) {
    if (!tb) return;
    nrs_ctx* c = tb->c;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    delete tb;
}

extern "C" int nrs_tbuf_clear(nrs_tbuf* tb) {
    if (!tb) return NRS_ERR_INVALID;
    tb_reset(tb->h, tb->h.max_size);                               // (the slots keep their size; a block is rewritten before it is read again)
    return NRS_OK;
}

extern "C" int nrs_tbuf_insert(nrs_tbuf* tb, int32_t n, const int32_t* kp_id, const float* kp_xy, const float* lm_xyz, const int32_t* status,
                               const uint8_t* has_lm, const float pose_qt[7], float deform_mag) {
    if (!tb) return NRS_ERR_INVALID;
    nrs_ctx* c = tb->c;
    const TbInsertIn in{n, kp_id, kp_xy, lm_xyz, status, has_lm, pose_qt, deform_mag};
    TbPlan plan;
    char msg[256];
    if (tb_plan_insert(tb->h, in, &plan, tb->seen, msg, sizeof(msg)) != 0) return c->fail(NRS_ERR_INVALID, "%s", msg);
    NRS_HIP(c, hipSetDevice(c->device));
    if (plan.new_cap > tb->h.cap) { NRS_TRY(tb_grow_slots(tb, plan.new_cap)); tb->h.cap = plan.new_cap; }
    const size_t words = (size_t)TBUF_HEAD + (size_t)TBUF_ENTRY * (size_t)plan.m;
    NRS_TRY(tb_stage(tb, tb_slot_words(tb->h.cap)));
    tb_pack(in, plan, tb->pin.as<uint32_t>());
    NRS_HIP(c, hipMemcpyAsync(tb->slots.as<uint32_t>() + (size_t)plan.slot * tb_slot_words(tb->h.cap), tb->pin.p, 4 * words, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipEventRecord(tb->ev_up.get(), c->stream));
    tb->up_pending = true;
    tb_commit(tb->h, in, plan);
    return NRS_OK;
}

extern "C" int nrs_tbuf_info(const nrs_tbuf* tb, int32_t* n_frames, int32_t* n_ids, int32_t* n_candidates) {
    if (!tb) return NRS_ERR_INVALID;
    if (n_frames) *n_frames = (int32_t)tb->h.snaps.size();
    if (n_ids) *n_ids = tb->h.n_ids();
    if (n_candidates) *n_candidates = tb->h.n_candidates();
    return NRS_OK;
}

extern "C" int nrs_tbuf_flat(nrs_tbuf* tb, int32_t* ids, uint8_t* has_kp, float* kp_xy, uint8_t* has_lm, float* lm_xyz, int32_t* last_status,
                             float* poses, float* deform_mag) {
    if (!tb) return NRS_ERR_INVALID;
    nrs_ctx* c = tb->c;
    const size_t F = tb->h.snaps.size(), n = (size_t)tb->h.n_ids();
    if (!poses || !deform_mag || (n > 0 && (!ids || !has_kp || !kp_xy || !has_lm || !lm_xyz || !last_status)))
        return c->fail(NRS_ERR_INVALID, "nrs_tbuf_flat: null output");
    for (size_t f = 0; f < F; ++f) {                               // (the host's copies; with ids held, the device's own tables below)
        memcpy(poses + 7 * f, tb->h.snaps[f].pose, 28);
        deform_mag[f] = tb->h.snaps[f].mag;
    }
    if (n == 0) return NRS_OK;
    NRS_HIP(c, hipSetDevice(c->device));
    TbFlat A;
    TbLayout L(0, 0, 0);
    NRS_TRY(tb_flatten(tb, 0, A, L));
    NRS_HIP(c, hipMemcpyAsync(ids, A.row_id, 4 * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(has_kp, A.has_kp, F * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(kp_xy, A.kp_xy, 8 * F * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(has_lm, A.has_lm, F * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(lm_xyz, A.lm_xyz, 12 * F * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(last_status, A.status, 4 * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(poses, A.poses, 28 * F, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(deform_mag, A.mag, 4 * F, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    return NRS_OK;
}

extern "C" int nrs_map_frame_tbuf(nrs_ctx* c, const nrs_camera* cam, nrs_tbuf* tb, float rad_per_pixel, float rigidity_th, int32_t min_track,
                                  int32_t index_snapshot, int32_t* n_cand, int32_t* cand_ids, int32_t* rigid_status, float* rigid_xyz,
                                  int32_t* deform_status, float* deform_xyz, int32_t counts[3], int32_t* n_accepted, int32_t* accepted_ids,
                                  float* accepted_xyz) {
    if (!c) return NRS_ERR_INVALID;
    if (!tb) return c->fail(NRS_ERR_INVALID, "nrs_map_frame_tbuf: null buffer");
    if (tb->c != c) return c->fail(NRS_ERR_INVALID, "nrs_map_frame_tbuf: the buffer belongs to another context");
    const void* const outs[10] = {n_cand, cand_ids, rigid_status, rigid_xyz, deform_status, deform_xyz, counts, n_accepted, accepted_ids, accepted_xyz};
    bool state = false;
    char msg[256];
    if (tb_check_map(tb->h, cam, cam ? cam->model : 0, rad_per_pixel, rigidity_th, index_snapshot, outs, &state, msg, sizeof(msg)) != 0)
        return c->fail(state ? NRS_ERR_STATE : NRS_ERR_INVALID, "%s", msg);
    const int nc = tb->h.n_candidates();
    if (nc == 0) {                                                 // no candidates: 0 / 0 votes deformable (mapping.cc:201) and nothing is launched
        *n_cand = 0; *n_accepted = 0;
        counts[0] = 0; counts[1] = 0; counts[2] = MAP_MODE_DEFORMABLE;
        return NRS_OK;
    }
    NRS_HIP(c, hipSetDevice(c->device));
    StageTimer tm{c, "nrs_map_frame_tbuf", true};
    TbFlat A;
    TbLayout L(0, 0, 0);
    NRS_TRY(tb_flatten(tb, map_ws_bytes(nc), A, L));
    tm("flatten");
    TriArgs T;
    T.cam.model = cam->model;
    for (int i = 0; i < 8; ++i) T.cam.p[i] = cam->params[i];
    T.F = A.S.F; T.n = A.n; T.n_cand = 0; T.min_track = min_track;
    T.poses = A.poses; T.has_kp = A.has_kp; T.kp_xy = A.kp_xy; T.has_lm = A.has_lm; T.lm_xyz = A.lm_xyz; T.status = A.status;
    T.cand = nullptr; T.o_status = nullptr; T.o_xyz = nullptr; T.o_dbg = nullptr; T.close_bits = nullptr;
    const MapOut out{n_cand, cand_ids, rigid_status, rigid_xyz, deform_status, deform_xyz, counts, n_accepted, accepted_ids, accepted_xyz};
    return map_run(c, "nrs_map_frame_tbuf", T, A.mag, tb->ws.as<char>() + L.bytes, nc, rad_per_pixel, rigidity_th, index_snapshot, A.row_id, out);
}
