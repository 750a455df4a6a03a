// Context shared by the C-ABI entry points: one HIP stream, growable device buffers, last-error text.  The buffers, the pinned words, the
// streams and the events are owners (nrs_own.hpp): they free themselves when the context, or the state that holds them, is deleted.
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "../../include/nrs.h"
#include "nrs_own.hpp"
#include "nrs_switches.hpp"

namespace nrs {

struct Engine;       // nrs_engine.hip
struct EmbWindow;    // nrs_engine.hpp: the lists of an embedded window built in one call
struct RgWindow;     // nrs_engine.hpp: what nrs_dba_solve_window_rg leaves next to its resident window
struct KltState;     // nrs_klt.hip
struct ShiState;     // nrs_shi.hip
struct FrontState;   // nrs_front.hip
struct PlanWorker;   // nrs_engine_nd.hpp
struct NdCache;      // nrs_engine_nd.hpp

// Exchange steps of a sharded solve (nrs_comm.hip): one process per GPU, every call is ordered on the
// context's stream.  Two primitives are all the engine needs:
//   allreduce : element-wise sum of n doubles over the ranks, the same bits on every rank
//   exchange  : boundary rows of a replicated-layout row vector with rank-1 / rank+1 (offsets in doubles)
// and one for the sharded keyframe-block factorisation (nrs_engine_kft.hpp):
//   handover  : one point-to-point move: rank `from` sends n doubles, rank `to` receives them.  COLLECTIVE in the sense that every
//               rank calls it at the same point of the schedule with the same (from, to, n); the others move nothing
struct HaloPlan { size_t lo_send = 0, lo_send_n = 0, hi_send = 0, hi_send_n = 0, lo_recv = 0, lo_recv_n = 0, hi_recv = 0, hi_recv_n = 0; };
struct Comm {
    int rank = 0, world = 1;
    virtual ~Comm() {}
    virtual int allreduce(nrs_ctx* c, const double* send, double* recv, size_t n) = 0;
    virtual int exchange(nrs_ctx* c, double* vec, const HaloPlan& h, hipStream_t stream) = 0;   // ordered on `stream`
    virtual int handover(nrs_ctx* c, const double* send, double* recv, size_t n, int from, int to) = 0;   // ordered on the context's stream
};
struct Arena { DevBuf mem; size_t off = 0; };   // one device allocation that an engine's arrays are carved from (nrs_engine_plan.hpp)

}  // namespace nrs

struct nrs_ctx {
    int device = 0;
    // Streams and events come first: members are destroyed in reverse order, so every buffer below is freed while they still exist.
    nrs::Stream main_stream;         // the context's own stream ...
    hipStream_t stream = nullptr;    // ... and the stream launches are ordered on: main_stream, but for the time a shadow set's view swaps it (nrs_engine.hip)
    nrs::Event ev0, ev1;
    nrs::Stream comm_stream;         // boundary-row exchanges run here, next to the interior tiles on `stream`
    nrs::Event ev_vec, ev_halo;
    // speculative LM trials of the single-frame engines (nrs_engine_types.hpp SpecSet): streams and events of the shadow sets
    nrs::Stream spec_stream[3];
    nrs::Event spec_fork, spec_join[3];
    nrs::Event spec_back[4];         // behind the back pass of the batch's k-th trial (they run one after the other: nd_solve_enqueue)
    hipDeviceProp_t prop;
    nrs_options opt;
    nrs::DebugOpts dbg;              // debug / A-B switches (nrs_switches.hpp): read once at nrs_create, changed by nrs_debug_set only
    char err[512];
    nrs_profile prof;
    // scratch for a1
    nrs::DevBuf po_uv, po_X, po_err, po_level, po_out, po_trace, po_multi;   // (po_multi: state + partial slots of the multi-workgroup form)
    // resident BA problem (a3) and per-call tracking problems (a2): one reusable arena each
    nrs::Engine* dba = nullptr;
    nrs::Arena arena_dba, arena_trk;
    nrs::KltState* klt = nullptr;
    nrs::ShiState* shi = nullptr;
    nrs::FrontState* front = nullptr;   // image front end: configuration + the resident grey / CLAHE / Global mask of the last frame
    nrs::Comm* comm = nullptr;       // set by nrs_comm_init_*: BA problems uploaded afterwards are sharded over its ranks
    nrs::DevBuf tap;                 // residual taps (edge lists by vertex + outputs) of the engine `tap_serial`: built on first use
    unsigned long long tap_serial = 0, engine_serial = 0;
    nrs::DevBuf pack_ws, pack_ws2, pack_ws3, pack_ws4;   // device-side problem construction (scratch plans: nrs_devpack_host.hpp): raw inputs + intermediates, window-edge scratch and output
    nrs::DevBuf dba_skin;            // ... and of the resident BA window (N2b)
    nrs::DevBuf fused_snap;          // NRS_CHECK_FUSED: the state a fused iteration is launched from twice (nrs_engine_probes.hpp)
    nrs::DevBuf dba_kft;             // embedded BA window: the keyframe-block factorisation (nrs_engine_kft.hpp)
    bool kft_attr_done = false;      // ... its kernels' dynamic-LDS attributes are set on this context's device (kft_kernel_attributes)
    nrs::EmbWindow* dba_embwin = nullptr;   // lists of the resident window when nrs_dba_solve_window_embedded made it (dropped by dba_free)
    nrs::RgWindow* dba_rgwin = nullptr;     // statistics (and host-packed lists) of the resident window when nrs_dba_solve_window_rg made it (dropped by dba_free)
    nrs::PinBuf embwin_pin;          // pinned host staging of the device-built lists (nrs_engine_embwin.hpp), kept for the context's lifetime
    nrs::DevBuf nd_skin;             // embedded mode (nrs_engine_skin.hpp): the skinned observations of the tracking engine
    nrs::PlanWorker* plan_worker = nullptr;   // the helper thread of the direct solver's symbolic phase (one for the context's lifetime)
    nrs::NdCache* nd_cache = nullptr;         // direct solver of the tracking engines (kernels: nrs_nd_kernels.hpp): the last few plans with their device arrays
    nrs::DevBuf comm_flag;           // one double: status word the ranks agree on after a sharded upload
    nrs::DevBuf gather_ws;           // sharded download / taps: two full-length row vectors for the gather (a rank holds its own rows only); released after use
    bool err_local = true;           // last set-up failure may be specific to this rank (allocation, HIP, rank-dependent checks)
    nrs::PinBuf pin_scal, pin_flags; // pinned host mirrors of the engine's scalars (doubles) / flags (ints)
    int seq = 0;                     // sequence number of the last publication the host waited for (pin_flags[7])
    nrs::PinBuf pin_spec_scal, pin_spec_flags;   // ... and of the shadow sets
    int spec_run = 4;                // rejections of the last completed run of an LM iteration (sizes the next batch)

    int fail(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, sizeof(err), fmt, ap);
        va_end(ap);
        return code;
    }
    // exactly `bytes` of device memory in b, what it held freed first; the caller words the failure
    hipError_t alloc(nrs::DevBuf& b, size_t bytes) {
        b.reset();
        const hipError_t e = hipMalloc(&b.p, bytes);
        if (e == hipSuccess) b.cap = bytes; else b.p = nullptr;
        return e;
    }
    int ensure(nrs::DevBuf& b, size_t bytes) {
        if (bytes <= b.cap && b.p) return NRS_OK;
        const size_t want = nrs::grown_bytes(bytes);
        const hipError_t e = alloc(b, want);
        if (e != hipSuccess) return fail(NRS_ERR_ALLOC, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        if (dbg.is_set(nrs::SW_POISON)) { (void)hipMemset(b.p, 0xFF, want); (void)hipDeviceSynchronize(); }     // (debug: a read of memory nobody wrote shows up as NaN)
        return NRS_OK;
    }
    // pinned host memory: kept when it holds `bytes`, else freed first and allocated anew as exactly `bytes` (a site that grows in
    // larger steps asks for its step); the caller words the failure
    hipError_t ensure_pinned(nrs::PinBuf& b, size_t bytes, unsigned flags) {
        if (bytes <= b.cap && b.p) return hipSuccess;
        b.reset();
        const hipError_t e = hipHostMalloc(&b.p, bytes, flags);
        if (e == hipSuccess) b.cap = bytes; else b.p = nullptr;
        return e;
    }
};

namespace nrs {
// a non-blocking stream / an event into its owner
inline hipError_t stream_create(Stream& s) { hipStream_t h = nullptr; const hipError_t e = hipStreamCreateWithFlags(&h, hipStreamNonBlocking); s.reset(h); return e; }
inline hipError_t event_create(Event& ev, unsigned flags = hipEventDisableTiming) { hipEvent_t h = nullptr; const hipError_t e = hipEventCreateWithFlags(&h, flags); ev.reset(h); return e; }
}  // namespace nrs

#define NRS_HIP(ctx, call)                                                                     \
    do {                                                                                       \
        hipError_t e__ = (call);                                                               \
        if (e__ != hipSuccess)                                                                 \
            return (ctx)->fail(NRS_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                               __FILE__, __LINE__);                                            \
    } while (0)

#define NRS_TRY(expr)                \
    do {                             \
        int rc__ = (expr);           \
        if (rc__ != NRS_OK) return rc__; \
    } while (0)

namespace nrs {
// NRS_TIMING: one "[nrs] <who> <stage> <ms>" line per stage on stderr, the stage name padded to `width` (tools/shard_pack_probe.py,
// shard_rank_setup_probe.py and embedded_window_probe.py read them).  sync: the stage's launches are waited for before its time is taken
// (host stages are not waited for; synced() waits for one stage only); by_rank: the line names the rank of a sharded context.
struct StageTimer {
    nrs_ctx* c; const char* who; bool sync; int width = 18; bool by_rank = sync;
    bool on = c->dbg.is_set(SW_TIMING);
    std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        if (!on) return;
        if (sync) (void)hipStreamSynchronize(c->stream);
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - t_prev).count();
        if (by_rank && c->comm) fprintf(stderr, "[nrs] rank %d/%d %s %-*s %.2f ms\n", c->comm->rank, c->comm->world, who, width, what, ms);
        else fprintf(stderr, "[nrs] %s %-*s %.2f ms\n", who, width, what, ms);
        t_prev = now;
    }
    void synced(const char* what) { if (on) (void)hipStreamSynchronize(c->stream); (*this)(what); }
};

void dba_free(nrs_ctx* ctx);
void nd_cache_free(nrs_ctx* ctx);
void comm_free(nrs_ctx* ctx);
int comm_agree(nrs_ctx* ctx, int rc);    // collective: 0 if every rank passed 0, else an error on every rank
void klt_free(nrs_ctx* ctx);
void shi_free(nrs_ctx* ctx);
void front_free(nrs_ctx* ctx);
// nrs_front.hip, for the *_front entry points of the tracker and the extractor: the resident image (NRS_FRONT_IMAGE_*) and, when asked for,
// the Global mask of the last nrs_front_process -- packed w x h bytes on the device; NRS_ERR_STATE when there is none or its size differs
int front_resident(nrs_ctx* ctx, const char* who, int w, int h, int image, int use_global_mask, const uint8_t** img, const uint8_t** mask);
// ... and for the *_front entry points of the stereo stages: the same image of both eyes after nrs_front_process_stereo; NRS_ERR_STATE when
// no pair is resident (a one-image nrs_front_process invalidates the right eye) or its size differs
int front_resident_pair(nrs_ctx* ctx, const char* who, int w, int h, int image, const uint8_t** left, const uint8_t** right);
// nrs_eval.hip, for nrs_stereo_match_pattern and nrs_init_stereo (nrs_sinit.hip): the pattern matcher's refusals under the caller's name,
// the bytes of its intermediates, and its launches on packed w x h images and n keypoints that are already on the device (n > 0; ws:
// stereo_match_ws_bytes bytes, 256-byte aligned; d_score / d_match as long as the entry point's outputs, never null here)
int stereo_match_check(nrs_ctx* ctx, const char* who, const nrs_camera* cam, const uint8_t* left, const uint8_t* right, int w, int h, int stride_l,
                       int stride_r, int n, bool arrays_ok);
size_t stereo_match_ws_bytes(nrs_ctx* ctx, int w, int h, int n);
int stereo_match_enqueue(nrs_ctx* ctx, const nrs_camera* cam, float bf, int w, int h, int n, const uint8_t* d_left, const uint8_t* d_right,
                         const float* d_xy, char* ws, float* d_xyz, int* d_status, double* d_score, int* d_match);
// mask bytes under n device-side keypoints (x, y floats, truncated), downloaded to host_out
int front_mask_at(nrs_ctx* ctx, const uint8_t* d_mask, int w, int h, const float* d_xy, int n, uint8_t* host_out);
}
